// swg_host_internal.h -- host-side object definitions behind the opaque handles
// of include/swg.h.  Not part of the public ABI.
#pragma once
#include "../../include/swg.h"
#include "swg_internal.h"

#include <algorithm>
#include <functional>
#include <map>
#include <memory>
#include <new>
#include <string>
#include <utility>
#include <vector>

// Allocator whose resize() leaves new elements uninitialised: the big residue arrays are filled
// by parallel loops, and pages should be first touched by the threads that fill them instead of by
// one thread writing zeros (a 10M-sequence database is 8 GB of them).
template <class T> struct SwgNoInit {
    using value_type = T;
    SwgNoInit() = default;
    template <class U> SwgNoInit(const SwgNoInit<U> &) {}
    T *allocate(size_t n) { return static_cast<T *>(::operator new(n * sizeof(T))); }
    void deallocate(T *p, size_t) { ::operator delete(p); }
    template <class U> void construct(U *p) noexcept { ::new ((void *)p) U; }
    template <class U, class A0, class... A> void construct(U *p, A0 &&a0, A &&...a)
    {
        ::new ((void *)p) U(std::forward<A0>(a0), std::forward<A>(a)...);
    }
    template <class U> bool operator==(const SwgNoInit<U> &) const { return true; }
    template <class U> bool operator!=(const SwgNoInit<U> &) const { return false; }
};

// Stream layout of the diagonal engine: pairs of adjacent sorted ranks, dealt to
// n_streams lane groups longest first; tokens are stored stream-major.
struct SwgDiagLayout {
    uint32_t n_streams = 0;
    uint32_t streams_per_wg = 0;
    uint64_t pair_begin = 0, pair_end = 0; // pairs of the sorted order laid out here
    uint64_t total_blocks = 0;      // 4-row token blocks over all streams
    uint64_t max_stream_blocks = 0;
    uint64_t pair_rows_total = 0;   // sum over pairs of (2 + longer length), unpadded
    std::vector<uint64_t> stream_off;      // [n_streams+1]
    std::vector<uint32_t> stream_pairs;    // pair ids, stream-major
    std::vector<uint32_t> stream_pair_off; // [n_streams+1]
    std::vector<uint32_t> tok;             // 4 dwords per block (one 32-bit token per row)
    // device image
    uint4 *d_tok = nullptr;
    uint64_t *d_stream_off = nullptr;
    uint32_t *d_stream_pairs = nullptr;
    uint32_t *d_stream_pair_off = nullptr;
    uint2 *d_scratch = nullptr;
    uint64_t d_scratch_rows = 0;
};

// Per-search device counters (swg_db::Bufs::d_counters; the first 32 words come back with every search, SwgSlot::h_counters):
// the single words below, then the sharded pair queues of the diagonal engine's two classes and their per-SIMD
// wavefront-rank counters.  The kernels receive pointers and never see the indices.
#define SWG_WORD_WORK_QUEUE 0u      // work queue of the bin-based fills
#define SWG_WORD_SATURATED 1u       // sequences that saturated the last 16-bit level (the int32 re-score's list length)
#define SWG_WORD_RESCORE_QUEUE 2u   // work queue of the bin-based int32 re-score
#define SWG_WORD_TOPK_COUNT 3u      // top-K: candidates kept,
#define SWG_WORD_TOPK_THR 4u        // the threshold its histogram gave,
#define SWG_WORD_TOPK_OVERFLOW 5u   // and whether that lay beyond the histogram
#define SWG_WORD_FLAGGED_ROWS 6u    // rows of the flagged pairs / sequences, in units of 16 (the f16 veto's input)
#define SWG_WORD_STAMPS(c) (8u + 4u * (uint32_t)(c)) // start / end wall-clock stamps of class c's single-pass launch (two 64-bit words)
#define SWG_WORD_FLAGGED_SEQS 16u   // sequences the f16 fill flagged
#define SWG_WORD_FLAGGED_PAIRS 17u  // ... and their pairs (the int16 re-run's list length)
// (18 .. 25: SWG_PRUNE_WORD_*, SWG_ABOVE_WORD_COUNT below)
#define SWG_QUEUE_WORD(c) (32u + (uint32_t)(c) * SWG_DYN_SHARDS * SWG_DYN_SHARD_STRIDE)
#define SWG_RANK_WORD(c) (SWG_QUEUE_WORD(2) + (uint32_t)(c) * SWG_DYN_SIMD_SLOTS)
#define SWG_COUNTER_BYTES ((size_t)SWG_RANK_WORD(2) * 4u)

// Pair-major tokens for the work-queue form of the diagonal engine: pair p of the sorted
// order owns blocks [pair_off[p], pair_off[p+1]); independent of the launch geometry.
struct SwgPairTokens {
    bool tried = false, ok = false;
    bool host_built = false; // diagnostics: tokens came from the host builder (option "host_tokens")
    uint64_t total_blocks = 0;
    uint4 *d_tok = nullptr;
    uint32_t *d_pair_off = nullptr;
    uint2 *d_edge[2] = {nullptr, nullptr};    // multi-pass: (M,B) per row between consecutive passes, ping-pong
    int2 *d_edge32[2] = {nullptr, nullptr};   // the same for the int32 work-queue kernel: per row and per sequence of the pair
    int32_t *d_edge32d[2] = {nullptr, nullptr}; // ... and the third edge value of its exact cells (gap scores of any sign)
    uint64_t edge_blocks = 0, edge32_blocks = 0, edge32d_blocks = 0; // token blocks the edge buffers were allocated for (a re-filled database may have grown)
    std::vector<uint32_t> pair_blocks_prefix; // host copy of pair_off
};

struct SwgDiagPlan {
    int variant = 0, K = 0, G = 0, npass = 0, W = 0, workgroups = 0;
    int wide = 0; // scores to 65535 (values biased by -32768)
    int f16 = 0;  // packed-f16 cells with three-operand maxima: scores below 4096, anything above flagged and re-scored
    // wide && f16_from > 0: both forms in one class -- the pairs before f16_from (the longest: sorted order) on the wide
    // form, those from it on on the f16 cells (same geometry, a launch each per pass)
    uint32_t f16_from = 0;
    // Several passes: the last one covers what is left of the query with the fewest columns per lane that do
    // (its own kernel instantiation and profile layout; edges do not depend on the geometry).  -1: as the others.
    int last_variant = -1, last_K = 0;
    // f16 cells (form 2): the fma pairing (CellsDiag FMA: (score, 1.0) profile of twice the size, 7.5 instructions per
    // column pair) instead of v_perm_b32 (8.5); ignored on the other cells
    int fma = 0;
    int gapless = 0; // f16 != 0: the gapless cells (CellsGapless, kernel form 3) instead of the three-state f16 cells
    uint32_t n_streams = 0;
    size_t lds_bytes = 0;
    double est_ms = 0.0;
};
// The diagonal engine's work split: class 0 = the bulk of the pairs, class 1 = the few
// longest ones, which would otherwise be the serial tail of the whole search.  The long
// class runs beside the bulk on a second HIP stream with 64 lanes per pair and as few
// columns per lane as cover the query, i.e. with the shortest possible chain per row.
struct SwgDiagWork {
    int n_classes = 0;
    SwgDiagPlan plan[2];
    uint64_t pair_begin[2] = {0, 0}, pair_end[2] = {0, 0};
};

// What the autotuner keeps per query length: the engine and its geometry.
struct SwgTuned {
    int engine = 2;    // 1 systolic, 2 diagonal
    int systolic_K = 0; // engine 1: columns per wavefront of the chosen instantiation
    double ms = 0;
    SwgDiagWork wk;    // engine 2
};

struct swg_db {
    // host image: what swg_db_pack builds and swg_db_save writes.  Sequences by sorted rank (length
    // descending, stable); 128 consecutive ranks form a bin (the unit of sharding and of the systolic
    // engine); the last bin of a shard may have empty slots (order = ~0, length 0).
    size_t n_total = 0;             // sequences of the whole database
    size_t n_local = 0;             // sequences of this shard
    uint32_t n_bins = 0;            // bins of this shard
    uint32_t max_nblk = 0;          // row-blocks of the longest bin
    uint64_t residues = 0;          // sum of lengths (this shard)
    uint64_t rows_padded = 0;       // sum over bins of nblk*4*128 (rows the bin-based kernels walk)
    std::vector<uint64_t> bin_off;  // [n_bins] dword offset of a bin in the device bin image
    std::vector<uint32_t> bin_nblk; // [n_bins]
    std::vector<uint32_t> order;    // [n_bins*128] original index of each slot, ~0u = empty
    std::vector<uint32_t> lens;     // [n_bins*128]
    // residue bytes (index<<3) by sorted rank; every sequence starts on a 4-byte boundary and is
    // filled up to one with the padding residue 0, so that a sequence is a run of whole dwords
    std::vector<uint8_t, SwgNoInit<uint8_t>> codes;
    std::vector<uint64_t> code_off; // [n_bins*128+1] byte offsets into codes (multiples of 4)
    SwgPairTokens ptok;             // pair-major tokens (work-queue form of the diagonal engine)
    SwgDiagLayout diag[2];          // stream layouts of the diagonal engine: [0] bulk, [1] long pairs
    std::vector<uint64_t> pair_rows_prefix; // rows of the pairs before pair p (swg_db_pair_rows: built on first use)
    // swg_plan_diag_work's last answer and what it was asked (the model is a pure function of the lengths and of
    // these): a search that repeats the previous one's question does not rank the geometries again
    std::vector<double> plan_key;
    SwgDiagWork plan_last;
    int plan_last_n = 0;
    std::map<uint64_t, SwgTuned> tuned; // query length -> engine + geometry that measured fastest on this device
    // What the last finished search of this database saw (plans of later searches only: results never depend
    // on it).  sat_hint: sequences its 16-bit fill flagged for the re-score (-1: no search yet), by which
    // the re-score's lane-group width is picked without reading the count back in the middle of a search;
    // f16_veto_epoch: the (query, scoring) epoch for which the packed-f16 cells flagged so many rows (a
    // database full of close relatives of the query) that the int16 cells are the faster first step.
    long long sat_hint = -1;
    uint64_t f16_veto_epoch = 0;
    // both 16-bit forms in one search (plan_search): for the last length threshold asked about, the first pair
    // of the sorted order whose sequences are all shorter, and the residues from it on
    uint32_t split_rows = 0, split_pair = 0;
    uint64_t split_residues = 0;
    // a database whose pair tokens were built straight from reference-shaped 16-lane batches
    // (swg_fill_batches16): there are no residue bytes by sorted rank, so nothing that needs them can run
    bool tokens_only = false;
    // a masked copy (swg_db_mask): what it was made with and what the kernels covered (swg_db_mask_info)
    bool masked = false;
    swg_mask_info mask_info = {};
    // a six-frame translation (swg_db_translate): what it was made with and what the kernel wrote (swg_db_translate_info)
    bool translated = false;
    swg_translate_info translate_info = {};
    // A view (swg_db_view): a database of its own whose slots are some of `root`'s sequences.  Its residue bytes are the
    // root's on the host and on the device -- codes is empty, code_off[s] is the ROOT's byte offset of slot s's sequence
    // (so consecutive slots are not adjacent in memory: a sequence ends at code_off[s] + its length, never at
    // code_off[s + 1]), d_codes is the root's pointer -- and everything else (lens, order, bins, pair tokens, plans,
    // hints, output buffers) is its own.  root_slot[s] = the root's slot of this view's slot s (ascending: the root's
    // sorted order is kept).  A root lives as long as its caller's handle or any view of it: refs counts both.
    swg_db *root = nullptr;
    std::vector<uint32_t> root_slot; // view: [n_local]
    size_t refs = 1;                 // root: the caller's handle (while handle_live) + the views alive
    bool handle_live = true;         // root: swg_db_free has not been called on it yet
    std::vector<uint32_t> slot_of;   // root: [n_total] slot of each original index, ~0u = not in this shard (built by the first view)
    // device image (valid after swg_db_upload): the residue bytes and three words per slot; the pair
    // tokens (ptok) and the bin image are built FROM them on the device, the bins only when an
    // engine that reads them is used (swg_ensure_bins)
    int device = -1;
    uint32_t *d_codes = nullptr;    // codes as dwords
    uint64_t *d_code_off = nullptr; // [n_slots+1] DWORD offsets into d_codes
    uint32_t *d_lens = nullptr;     // [n_slots]
    uint32_t *d_order = nullptr;    // [n_slots]
    uint32_t *d_packed = nullptr;   // bin image (systolic engine, int32 kernels): lazily built
    uint64_t *d_bin_off = nullptr;
    uint32_t *d_bin_nblk = nullptr;
    uint64_t upload_bytes = 0;      // bytes the last swg_db_upload copied over PCIe
    // per-search output buffers, one set per in-flight slot (allocated on first use); the
    // plain members below point at the set of the search being queued
    struct Bufs {
        int32_t *d_scores = nullptr;    // [n_bins*128] by sorted rank
        uint32_t *d_list = nullptr;     // [2*n_bins*128]: flagged pairs of the f16 fill, then (second half) saturated ranks
        uint32_t *d_counters = nullptr; // SWG_WORD_*, SWG_QUEUE_WORD, SWG_RANK_WORD
        uint64_t *d_keys = nullptr;     // top-K candidate keys (SWG_TOPK_CAND_CAP)
        uint32_t *d_hist = nullptr;     // top-K score histogram
        // a pruned search's score bound per pair and what follows it (swg_prune_layout; allocated by the first one)
        uint32_t *d_pair_bound = nullptr;
        size_t pair_bound_cap = 0;        // pairs it has room for
        // swg_search_above's keys once a search met more than SWG_ABOVE_KEYS_FLOOR of them (until then d_keys serves)
        uint64_t *d_above = nullptr;
        size_t above_cap = 0;             // keys it has room for
    } bufs[4];
    int32_t *d_scores = nullptr;
    uint32_t *d_list = nullptr;
    uint32_t *d_counters = nullptr;
    uint64_t *d_keys = nullptr;
    uint32_t *d_hist = nullptr;
    uint32_t *d_pair_bound = nullptr;
    std::vector<uint32_t> prune_stages; // {begin, end} of the stages cut pair by pair in the pruned search last launched (tests)
};

// The score ceilings of the cell forms, and the largest gap magnitude the packed-f16 cells hold as an exact integer.
// A score that reaches a form's ceiling is flagged and handed to the next form.
#define SWG_F16_GAP_MAX 2048
#define SWG_F16_CEILING 4096
#define SWG_I16_CEILING 32767 // (also the largest gap magnitude of the packed int16 cells)
#define SWG_WIDE_CEILING 65535
// gap magnitudes (of non-positive gap scores go = open + extend, ge = extend) fit the f16 cells
inline bool swg_f16_gaps_ok(int go, int ge) { return -go <= SWG_F16_GAP_MAX && -ge <= SWG_F16_GAP_MAX; }

// LDS of one CU, and the workgroups of W wavefronts and `lds` bytes each that a CU holds: `wave_budget` (an
// instantiation's max_waves, which is also the wave budget of one CU for its register allocation) is one limit, LDS the
// other; never fewer than one.
#define SWG_LDS_PER_CU ((size_t)160 * 1024)
inline int swg_workgroups_per_cu(int wave_budget, int W, size_t lds)
{
    return std::max(1, std::min<int>(wave_budget / W, (int)(SWG_LDS_PER_CU / lds)));
}

// The largest score a query can reach against sequences of at most `longest` rows: not above the query's best possible
// total (every column paired with its best-scoring residue of 1 .. 31: qbound) nor above min(lq, longest) times the
// largest entry (smax).  idx != NULL: rows is the 32 x 32 table and idx the query's lq residue indices; idx == NULL: rows
// are the lq x 32 rows of a PSSM, whose largest entry is the largest of its positions' best ones.
struct SwgScoreBound {
    uint64_t qbound = 0, bound = 0;
    int smax = 0;
};
SwgScoreBound swg_score_bound(const int8_t *rows, const int8_t *idx, size_t lq, uint64_t longest);
// test hook: out[0..2] = qbound, smax, bound
extern "C" int swg_debug_score_bound(const int8_t *rows, const int8_t *idx, size_t lq, uint64_t longest, uint64_t *out);

// Hits-only pruning (swg_diag_host.cpp, host only): the table of the score bound (rows / idx as
// swg_score_bound takes them), U of one sequence of table indices, and what a search decides about it.
SwgColMax swg_prune_colmax(const int8_t *rows, const int8_t *idx, size_t lq);
uint64_t swg_prune_bound(const SwgColMax &cm, const int8_t *seq, size_t len);
struct SwgPruneAsk {
    int mode = 1; // option "prune": 0 off, 1 auto, 2 wherever it is structurally possible (diagnostic)
    size_t k = 0;
    bool want_scores = false;
    int gap_open = 0, gap_extend = 0;
    int bits = 16;
    bool use_diag = true;
    int n_classes = 1;
    bool work_queue = true;  // the class runs off the lane groups' work queue
    bool both_forms = false; // the wide / int16 + f16 split of one class
    bool gapless = false;
    bool batch = false;      // one query of swg_search_multi* / swg_search_gapless_multi* / a list's fall-back
    uint64_t range_pairs = 0, groups = 0; // the class's pairs, the lane groups resident on the device
    long prune_head = 4;     // option "prune_head"
    size_t n_segments = 1;   // launches per pass (token_segments)
    // a caller's threshold (swg_search_above): T is min_score from the first launch on, so there is no head and k,
    // want_scores, n_segments and prune_head decide nothing
    bool fixed = false;
};
// What a stage of a pruned fill queues in front of its fill launches (swg_prune_stages below has the rules in words).
enum : uint32_t {
    SWG_STAGE_THRESHOLD = 1u, SWG_STAGE_PREFIX_CUT = 2u, SWG_STAGE_GATE = 4u, SWG_STAGE_REFINE = 8u, SWG_STAGE_LIST = 16u, SWG_STAGE_REFINE3 = 32u,
    SWG_STAGE_REFINE4 = 64u, SWG_STAGE_BOUND = 128u, SWG_STAGE_REFINE5 = 256u
};
// The refinement levels behind the first, the second to the fifth: one row each, [level - 2], in the order
// their walks are queued.  Everything on the host that touches a level walks this table -- the options (swg_set_option),
// the choice (swg_prune_refine_choices), the stage list (swg_prune_stages), the tables (prepare_prune, reserve_refine_table,
// swg_destroy), the launches (enqueue_pruned_fill) and the test hooks.  A further level is a row here, its launch
// (launch_refine_level, swg_api.cpp) and the few lines of its own in swg_prune_refine_choices.
// A level's walk takes the pairs the levels in front of it left at or above the threshold word and keeps the lesser bound.
#define SWG_REFINE_LEVELS 4
struct SwgRefineLevel {
    const char *option;       // its option: 0 automatic, 1 off, or one of `forced`
    const char *option_error; // ... and what swg_set_option says to any other value
    const char *table_error;  // what prepare_prune says to segments or a width the level does not walk (%d: the segments)
    // the option values that force the level, the segments each stands for, and what the automatic rule books for it: the
    // share of the headline's rows kept behind the level in front less that kept behind this one (value 0: no such entry)
    struct Forced {
        long value;
        int segments;
        double gain;
    } forced[2];
    uint32_t stage_bit; // SWG_STAGE_*: a stage that queues the level's walk
    int k;              // its table (swg_ctx::kmer_refine[level - 2]): blocks of k residues in the level's segments,
    bool spans;         // ... of the second entries, built with the spans credited (swg_kmer_table5_kernel<E, true>)
    int reads;          // the row of another level whose table its walk reads as well (-1: none)
    bool reserved;      // the table is a buffer of fixed size reserved in front of the search, whose allocation may be refused (reserve_refine_table)
    double bound_row;   // the automatic rule: seconds of its walk per pair row of the range; its table costs swg_kmer_table_cells(k) cells per query column
};
constexpr SwgRefineLevel SWG_REFINE_LEVEL[SWG_REFINE_LEVELS] = {
    // the second: k = 4 in 64 or 128 segments.  profiles/prune_refine_ab.txt -- rows kept 0.2677 / 0.2443 / 0.2249 (section 2); the
    // refine kernel at 128 segments 4.11 ms per search over 1 938 193 684 pair rows (section 3), which 64 segments, not traced
    // singly and half the bytes, is charged too
    {"prune_refine", "prune_refine must be 0 (auto), 1 (off), 64 or 128 (the segments of the second-level bound's table)",
     "the second-level bound's table: %d segments (64 or 128)", {{64, 64, 0.0234}, {128, 128, 0.0428}}, SWG_STAGE_REFINE, 4, false, -1, false, 2.1e-12},
    // the third: k = 4 in 256 segments of bytes.  profiles/prune_bytes_ab.txt -- rows kept 0.2249 at 128 segments, 0.2098 at 256
    // (section 2); the walk at 256 segments over byte tables 3.37 ms per search over 1 938 193 684 pair rows (section 3)
    {"prune_refine3", "prune_refine3 must be 0 (auto), 1 (off) or 256 (the segments of the third-level bound's table)",
     "the third-level bound's table: %d segments (256)", {{256, 256, 0.0151}, {0, 0, 0.0}}, SWG_STAGE_REFINE3, 4, false, -1, false, 1.74e-12},
    // the fourth: k = 5 in 256 segments of bytes, 1.32 GB; its option names (k, S) as 1000 k + S.  profiles/prune_deep_ab.txt -- the
    // rows kept behind the third level less those behind the fourth, the fourth walk per pair row of the range
    {"prune_refine4", "prune_refine4 must be 0 (auto), 1 (off) or 5256 (the fourth-level bound's table: k = 5 in 256 segments)",
     "the fourth-level bound's table: %d segments (256) of bytes", {{5256, 256, 0.0374}, {0, 0, 0.0}}, SWG_STAGE_REFINE4, 5, false, -1, true, 1.31e-12},
    // the fifth: the fourth's table and its own of the second entries.  profiles/prune_adjacent_ab.txt -- the rows kept behind the
    // fourth level less those behind the fifth (the host model, section 0), the fifth walk per pair row of the range
    {"prune_refine5", "prune_refine5 must be 0 (auto), 1 (off) or 5256 (the fifth-level bound: both k = 5 tables in 256 segments)",
     "the fifth-level bound's tables: %d segments (256) of bytes", {{5256, 256, 0.0254}, {0, 0, 0.0}}, SWG_STAGE_REFINE5, 5, true, 2, true, 4.0e-12},
};
// the segments an option value forces on level row i (0: the value forces nothing), and whether it is a value of the option at all
constexpr int swg_refine_forced_segments(int i, long v)
{
    return v != 0 && v == SWG_REFINE_LEVEL[i].forced[0].value ? SWG_REFINE_LEVEL[i].forced[0].segments
           : v != 0 && v == SWG_REFINE_LEVEL[i].forced[1].value ? SWG_REFINE_LEVEL[i].forced[1].segments
                                                               : 0;
}
constexpr bool swg_refine_value_ok(int i, long v) { return v == 0 || v == 1 || swg_refine_forced_segments(i, v) != 0; }
struct SwgPrunePlan {
    bool on = false;
    uint32_t head_pairs = 0; // one segment: pairs of the first stage; 0: the stages are the segments
    int kmer = 0;            // the bound: 1 colmax, 4 / 5 the k-mer table of that k (swg_prune_kmer_choice); 0 while off
    int segments = 0;        // ... and the segments of that table (1: the unordered sum of swg_pair_bound_kmer_kernel)
    int refine[SWG_REFINE_LEVELS] = {}; // the segments of the levels behind the first, [level - 2] (swg_prune_refine_choices): 0 without the level
    bool prefix_cut = false; // option "prune_cut" = 1: a stage's list is the prefix up to its last pair that reaches T
    bool gate = false;       // the first level's launch is gated by T and queued with a stage (swg_prune_gate_choice)
    bool fixed = false;      // a caller's threshold: every stage, the first included, is a list launch cut at fixed_T
    uint32_t fixed_T = 0;    // ... written once to the threshold word and never recomputed
};
// swg_db::Bufs::d_pair_bound for n pairs: the bounds, the pair ids in order, the lists (a cut stage's kept pairs, from its
// first pair's word), one tile count per SWG_PRUNE_TILE pairs, and {T, kept pairs} of the first SWG_PRUNE_STAGE_RECS cut
// stages (tests read them back).  The allocation, the launch and the read-back hook all take it from here.
#define SWG_PRUNE_STAGE_RECS 256u
struct SwgPruneLayout {
    uint32_t *bounds, *ids, *lists, *tiles, *recs;
    size_t words; // of the whole buffer
};
inline SwgPruneLayout swg_prune_layout(uint32_t *base, size_t n_pairs)
{
    const size_t tiles = 3 * n_pairs, recs = tiles + n_pairs / SWG_PRUNE_TILE + 2;
    auto at = [base](size_t word) { return base ? base + word : nullptr; }; // (no buffer yet: the total alone is asked for)
    return SwgPruneLayout{base, at(n_pairs), at(2 * n_pairs), at(tiles), at(recs), recs + 2 * SWG_PRUNE_STAGE_RECS};
}
SwgPrunePlan swg_prune_plan(const SwgPruneAsk &a);
// The stages of a pruned fill over the pair ranges `segments` (token_segments), and what is queued in front of each: the
// one place that decides it (enqueue_pruned_fill in swg_api.cpp walks the list).  The stages are the segments, or the
// head and the rest of a lone segment whose head is shorter than it.  Every stage but the first is cut at the K-th best
// score so far, which a threshold kernel computes in front of it; under a caller's threshold (plan.fixed) the first is
// cut too and no threshold kernel runs.  A cut is the prefix cut (plan.prefix_cut), or pair by pair: the refine pass
// where there is a second level (plan.refine[0]) -- behind the gate on the first of several stages under a caller's
// threshold --, then the walk of every further level the plan has, in the order of SWG_REFINE_LEVEL and under the same
// threshold word, then the list.  With the gate in front of the first level (plan.gate) the stage that first has a threshold --
// the second of several, or the first under a caller's threshold -- also queues the first level's launch, behind the
// threshold kernel and in front of everything else: gated by that threshold, over all pairs from the stage's first to the
// range's last.  A fill whose list holds no such stage bounds every pair before its first stage, ungated.
struct SwgPruneStage {
    uint32_t begin, end; // pairs
    uint32_t segment;    // index into `segments`
    uint32_t queued;     // SWG_STAGE_*: the kernels in front of the stage's fill launches, in that order (0: none, an uncut stage)
};
std::vector<SwgPruneStage> swg_prune_stages(const SwgPrunePlan &plan, const std::vector<std::pair<uint32_t, uint32_t>> &segments);
// What the first level's launch takes under a stage list: `stage` the stage that queues it (SWG_STAGE_BOUND), or
// stages.size() where none does -- the pairs [begin, end) = [0, n_pairs) are then bounded, ungated, before the first
// stage.  Queued with a stage, the launch takes [begin, end) from that stage's first pair to the last stage's last, and
// the pairs [skip_begin, skip_end) of the stages in front of it, which are launched unpruned, have their words set to
// SWG_PRUNE_NOT_BOUNDED.
#define SWG_PRUNE_NOT_BOUNDED 0xFFFFFFFFu
struct SwgPruneBoundRange {
    size_t stage;
    uint32_t begin, end, skip_begin, skip_end;
};
SwgPruneBoundRange swg_prune_bound_range(const std::vector<SwgPruneStage> &stages, uint32_t n_pairs);
// test hook: in[0..4] = head_pairs, fixed, refine, prefix_cut, the number of segments n, then n x {begin, end}; out: four
// words per stage {begin, end, segment, queued}, copied while they fit cap stages; *n_out = the number of stages
extern "C" int swg_debug_prune_stages(const int64_t *in, int64_t *out, size_t cap, size_t *n_out);
// ... with the third level: in[0..5] = head_pairs, fixed, refine, prefix_cut, refine3, n, then the n segments
extern "C" int swg_debug_prune_stages3(const int64_t *in, int64_t *out, size_t cap, size_t *n_out);
// ... and the fourth: in[0..6] = head_pairs, fixed, refine, prefix_cut, refine3, refine4, n, then the n segments
extern "C" int swg_debug_prune_stages4(const int64_t *in, int64_t *out, size_t cap, size_t *n_out);
// ... and the gate: in[0..7] = head_pairs, fixed, refine, prefix_cut, refine3, refine4, gate, n, then the n segments
extern "C" int swg_debug_prune_stages5(const int64_t *in, int64_t *out, size_t cap, size_t *n_out);
// ... and the fifth level: in[0..8] = head_pairs, fixed, refine, prefix_cut, refine3, refine4, gate, refine5, n, then the n segments
extern "C" int swg_debug_prune_stages6(const int64_t *in, int64_t *out, size_t cap, size_t *n_out);
// The automatic rule of a caller's threshold ("A caller's threshold"; profiles/search_above_ab.txt): the
// bound, list and tally kernels of a stage cost tens of microseconds whatever the range holds, a list launch one
// dependent load per claim; a range with at least SWG_PRUNE_ABOVE_AUTO_PAIRS pairs per resident lane group has fills
// long enough for both to vanish in them.
#define SWG_PRUNE_ABOVE_AUTO_PAIRS 16u
inline bool swg_prune_above_auto(uint64_t range_pairs, uint64_t groups) { return range_pairs >= SWG_PRUNE_ABOVE_AUTO_PAIRS * std::max<uint64_t>(1, groups); }
// How swg_search_above_multi* searches a batch ("A caller's threshold, per query of a batch"): 1 the one
// launch per class with the per-row read-out, 2 one query after another, each a plain swg_search_above.  option: "above_batch"
// (0 automatic, 1 the launch wherever plan_batch admits the batch, 2 always one by one); admitted: plan_batch's answer;
// single_pruned: whether swg_search_above of the batch's longest query on this database would be pruned under the
// context's "prune".  The automatic rule takes the launch where it is admitted and that search would not be pruned:
// the launch fills every pair for every query, a pruned search only the pairs whose bound reaches its threshold.
inline int swg_above_multi_route(long option, bool admitted, bool single_pruned)
{
    if (option == 2 || !admitted) return 2;
    if (option == 1) return 1;
    return single_pruned ? 2 : 1;
}
// test hook: the route (1 | 2), or SWG_ERR_ARG for an option outside 0..2
extern "C" int swg_debug_above_multi_route(long option, int admitted, int single_pruned);
extern "C" int swg_debug_prune_bound(const int8_t *rows, const int8_t *idx, size_t lq, const int8_t *flat, const uint64_t *offsets, size_t n,
                                     uint8_t *colmax_out, uint64_t *u_out);
extern "C" int swg_debug_prune_plan(const int64_t *in, int64_t *out);
extern "C" int swg_debug_prune_plan_above(const int64_t *in, int64_t *out);
// The k-mer form of the bound (swg_internal.h has the classes): its host restatement, and the choice of k.
void swg_kmer_cprof(const int8_t *rows, const int8_t *idx, size_t lq, int8_t *cprof);                 // cprof[lq][22]
// ... over S segments of the query's columns, the blocks taken in order (S = 1: the unordered sum over the whole query)
void swg_kmer_table_seg(const int8_t *cprof, size_t lq, int g, int e, int k, size_t S, uint16_t *table); // table[22^k][S]
uint64_t swg_kmer_bound_seg(const uint16_t *table, int k, size_t S, const SwgColMax &cm, const int8_t *seq, size_t len);
// The two rates the automatic choice weighs, measured on one MI355X (profiles/prune_kmer_ab.txt): the table
// kernel's cell updates per second (k = 5 at 3000 columns: 7.73e10 cells in 16.6 ms a thread per block; 1.83e10 in 4.0 ms
// a thread per prefix, profiles/prune_deep_ab.txt: the same rate), and the fill's pair rows per second
// -- a pair row costs one step of a 16-lane group per pass of 512 query columns (the headline unpruned: 1.938e9 pair rows
// x 6 passes in 1237.7 ms).
#define SWG_KMER_TABLE_RATE 4.6e12
#define SWG_KMER_FILL_PASS_RATE 9.4e9
// the table kernels' cell updates per query column: a thread per block and k cells each (k = 4), or a thread per 4-class
// prefix -- its four rows once, then the 22 fifth rows (k = 5: swg_kmer_table5_kernel, 4.2 times fewer than 22^5 x 5)
inline double swg_kmer_table_cells(int k)
{
    return k == 5 ? (double)swg_kmer_entries(4) * (4 + SWG_KMER_CLASSES) : (double)swg_kmer_entries(k) * k;
}
inline double swg_kmer_fill_rate(size_t lq) { return SWG_KMER_FILL_PASS_RATE / (double)std::max<size_t>(1, (lq + 511) / 512); }
struct SwgKmerAsk {
    long forced = 0;     // option "prune_kmer": 0 automatic, 1, 4, 5
    long forced_segments = 0; // option "prune_segments": 0 automatic, 1..SWG_KMER_MAX_SEGMENTS
    long forced_refine[SWG_REFINE_LEVELS] = {}; // the levels' options, [level - 2]: 0 automatic, 1 off, or a value that forces the level (SWG_REFINE_LEVEL)
    bool refine5_ok = false;  // swg_kmer_refine5_admitted for this query and scoring: e > 0 and second entries that are bytes
    bool fixed = false;       // a caller's threshold (swg_search_above): the fifth level is then forced or off
    long forced_gate = 0;     // option "prune_gate": 0 automatic, 1 off, 2 wherever the first level is a segmented k-mer bound
    int table_bits5 = 8;      // ... and of the k = 5 tables' (the fourth level takes bytes only)
    int table_bits = 8;       // the width of the k = 4 tables' entries for this query and scoring (swg_kmer_table_bits, "prune_table_bits")
    bool pruned = false; // swg_prune_plan's answer
    size_t lq = 0;
    uint64_t pair_rows = 0; // rows of the range's pairs
    double table_rate = SWG_KMER_TABLE_RATE, fill_rate = 0;
};
// whether a context builds the first-level table of (k, S): within SWG_KMER_TABLE_BUDGET at 16 bits an entry, whatever
// width the table takes (prepare_prune refuses the others)
inline bool swg_kmer_table_admitted(int k, long S)
{
    return S >= 1 && S <= (long)SWG_KMER_MAX_SEGMENTS && swg_kmer_entries(k) * (uint64_t)S * sizeof(uint16_t) <= SWG_KMER_TABLE_BUDGET;
}
int swg_prune_kmer_choice(const SwgKmerAsk &a, int *segments = nullptr); // 0 (not pruned: nothing is built), 1, 4 or 5; *segments: its S
extern "C" int swg_debug_prune_kmer(const int8_t *rows, const int8_t *idx, size_t lq, int gap_open, int gap_extend, int k, const int8_t *flat,
                                    const uint64_t *offsets, size_t n, uint16_t *table_out, uint64_t *u_out);
extern "C" int swg_debug_prune_kmer_seg(const int8_t *rows, const int8_t *idx, size_t lq, int gap_open, int gap_extend, int k, int S,
                                        const int8_t *flat, const uint64_t *offsets, size_t n, uint16_t *table_out, uint64_t *u_out);
extern "C" int swg_debug_prune_kmer_choice(const int64_t *in, int64_t *out);
extern "C" int swg_debug_prune_kmer_choice_seg(const int64_t *in, int64_t *out);
// The levels behind a first-level bound of (k, S), chosen in their order: out[level - 2] = the segments of
// the level's walk, or 0 without it.  A level is forced by its option behind whatever the others are, or off; left
// automatic it is taken only behind a chain of automatic choices, where its table's build and its walk cost at most half
// of what its tighter cut saves (swg_diag_host.cpp has each level's own conditions).
void swg_prune_refine_choices(const SwgKmerAsk &a, int k, int S, int out[SWG_REFINE_LEVELS]);
// test hooks: the chain up to one level.  in[0..5] = forced (option "prune_kmer"), pruned, lq, pair rows, table cells per
// second, fill pair rows per second (0, 0: the library's own rates for this lq), in[6] = option "prune_segments", in[7] =
// option "prune_refine" -> out[0..2] = k, S, S2 (0: no second level)
extern "C" int swg_debug_prune_refine_choice(const int64_t *in, int64_t *out);
extern "C" int swg_debug_prune_kmer_refine(const int8_t *rows, const int8_t *idx, size_t lq, int gap_open, int gap_extend, int S2, const int8_t *flat,
                                           const uint64_t *offsets, size_t n, uint16_t *table_out, uint64_t *u_out);
// test hooks: in[0..7] as swg_debug_prune_refine_choice, in[8] = option "prune_refine3", in[9] = the tables' entry width
// (0: bytes) -> out[0..3] = k, S, S2, S3; the mirror of the third level's bound (S3 = 256); and the entry width of the
// k-mer tables of a query (rows / idx as the mirrors take them) -> 8 or 16
extern "C" int swg_debug_prune_refine3_choice(const int64_t *in, int64_t *out);
extern "C" int swg_debug_prune_kmer_refine3(const int8_t *rows, const int8_t *idx, size_t lq, int gap_open, int gap_extend, int S3, const int8_t *flat,
                                            const uint64_t *offsets, size_t n, uint16_t *table_out, uint64_t *u_out);
extern "C" int swg_debug_prune_table_bits(const int8_t *rows, const int8_t *idx, size_t lq, int k);
// test hook: in[0..9] as swg_debug_prune_refine3_choice, in[10] = option "prune_refine4", in[11] = the k = 5 tables' entry
// width (0: bytes) -> out[0..4] = k, S, S2, S3, S4
extern "C" int swg_debug_prune_refine4_choice(const int64_t *in, int64_t *out);
// ... the mirror of the fourth level's bound: k = 5 over S4 = 128 or 256 segments.  It has no table to hand out: it
// computes the entries of the blocks the sequences hold.
extern "C" int swg_debug_prune_kmer_refine4(const int8_t *rows, const int8_t *idx, size_t lq, int gap_open, int gap_extend, int S4, const int8_t *flat,
                                            const uint64_t *offsets, size_t n, uint64_t *u_out);
// ... and of a fifth level's bound ("a fifth level"): the fourth level's blocks in S5 = 256 segments, with the
// query columns jumped over between two blocks charged.  *on_out = 0 and u_out unwritten where the level is off
// (swg_kmer_refine5_admitted); n_explicit: the walk's N, 0 for SWG_REFINE5_EXPLICIT, S5 or more for the exact form.
extern "C" int swg_debug_prune_kmer_refine5(const int8_t *rows, const int8_t *idx, size_t lq, int gap_open, int gap_extend, int S5, int n_explicit,
                                            const int8_t *flat, const uint64_t *offsets, size_t n, uint64_t *u_out, int *on_out);
// test hook: in[0..11] as swg_debug_prune_refine4_choice, in[12] = option "prune_refine5", in[13] = whether the query and
// scoring admit the level (swg_kmer_refine5_admitted), in[14] = whether the threshold is a caller's -> out[0..5] = k, S, S2,
// S3, S4, S5
extern "C" int swg_debug_prune_refine5_choice(const int64_t *in, int64_t *out);
// The gate in front of the first level: whether the first level's launch, of (k, S), waits for a threshold
// and leaves out the pairs whose colmax bound is below it.  Forced ("prune_gate" = 2) wherever the first level is a
// segmented k-mer bound; off ("prune_gate" = 1); automatic only where k and S were both chosen automatically and the range
// is one the third level's walk pays on.
bool swg_prune_gate_choice(const SwgKmerAsk &a, int k, int S);
inline bool swg_prune_gate_value_ok(long v) { return v == 0 || v == 1 || v == 2; }
// test hook: in[0..7] as swg_debug_prune_refine_choice, in[8] = option "prune_gate" -> out[0..2] = k, S, gate (0 | 1)
extern "C" int swg_debug_prune_gate_choice(const int64_t *in, int64_t *out);
// the words of a search's counter block (swg_db::Bufs::d_counters) a pruned search uses: the threshold so far and the
// threshold kernel's status word, then what swg_launch_prune_cut or swg_launch_prune_list writes: the pairs the stage
// takes, the pairs skipped so far, their token blocks (64 bits)
#define SWG_PRUNE_WORD_T 18u
#define SWG_PRUNE_WORD_CUT 20u
// ... and the word swg_above_compact_kernel counts in: every slot at or above a caller's threshold (swg_search_above)
#define SWG_ABOVE_WORD_COUNT 24u
// ... and the threshold word of the second level on its first of several stages (swg_prune_refine_gate_kernel)
#define SWG_PRUNE_WORD_GATE 25u
// keys the read-out of swg_search_above has room for before its buffer grows: the top-K's candidate buffer serves
#define SWG_ABOVE_KEYS_FLOOR SWG_TOPK_CAND_CAP

// Geometry of the systolic engine (bin-based kernels) for one query length.
struct SwgSystolicPlan {
    int bits = 0, variant = 0, K = 0, W = 0, npass = 0, workgroups = 0;
    SwgKernelInfo info = {};
    int f16 = 0; // int16 plan on the packed-f16 cells (one pass, no score of the search can reach their ceiling)
};

// Everything a search decides before it queues anything (swg_api.cpp: plan_search writes it, the stages that allocate
// and launch only read it, and swg_search_end reports from it).
struct SwgSearchPlan {
    int bits = 0;          // 16 / 32; 0: nothing queued (an empty database)
    bool fast_ok = false;  // the gap scores fit the packed forms (non-positive, magnitude within int16)
    int go = 0, ge = 0;    // gap_open + gap_extend, gap_extend
    int go32 = 0, ge32 = 0; // the same for the int32 level behind the 16-bit ones (they differ in a gapless search only)
    bool gapless = false;       // a gapless search (swg_search_gapless): go / ge are priced out, not the context's
    bool gapless_cells = false; // ... on the gapless cells (route 1); else the gapped machinery with those gaps (route 0)
    uint64_t score_bound = ~0ull, qbound = 0; // swg_score_bound of this query against this database
    uint64_t epoch = 0;    // the context's (query, scoring) epoch the plan was made under
    // the first level's cells, and where their flags go
    bool use_f16 = false;  // every class on the packed-f16 cells
    bool wide = false;     // the wide int16 form (scores to SWG_WIDE_CEILING)
    uint32_t split_at = 0, split_rows = 0; // both forms in one class: first pair of the f16 part, the length threshold
    uint64_t split_residues = 0;           // ... and the residues that run on the f16 cells
    bool rerun_wide = false;   // what the f16 cells flag is run again on the wide form (else plain int16)
    int32_t ceiling = 0;       // what the first level saturates at
    int32_t level_ceiling = 0; // ... and the last 16-bit level (the re-run's, when f16 cells came first)
    bool may_saturate = false; // a second level is queued
    bool int32_level = false;  // an int32 level follows the last 16-bit one,
    bool q32_ok = false;       // on the work-queue kernel,
    bool bin32 = false;        // or on the bin-based one (also a whole 32-bit fill without the work queue)
    bool some_f16() const { return use_f16 || split_at != 0u; } // some pairs run on the f16 cells: their flags are collected and re-run
    // engines
    bool use_diag = false, use_diag32 = false, use_q32 = false, exact32 = false;
    SwgDiagWork wk, wk32;            // lane groups: the 16-bit fill; the int32 work-queue fill of the whole database
    SwgSystolicPlan main_pl, re_pl;  // systolic engine: the fill; the int32 re-score
    int npass32 = 0;                 // passes of the bin-based int32 kernel
    SwgPrunePlan prune;              // hits-only pruning of the 16-bit fill
};

// Everything a query batch (swg_search_multi, swg_search_multi_pssm) decides before it queues anything: plan_batch
// (swg_api.cpp) writes it once, the stages that allocate, launch and deliver only read it, and the batch's swg_stats are
// reported from it.  The queries go through the launches in chunks of at most chunk_queries; the buffers are allocated
// once, for the first chunk, which is the largest.
struct SwgBatchPlan {
    bool one_launch = false; // else the queries are searched one after another, and nothing below is set
    int go = 0, ge = 0;      // gap_open + gap_extend, gap_extend
    int form = 0;            // the cells: 0 packed int16, 2 packed f16
    bool qq = false;         // two queries per lane (swg_diag_qq_kernel): row y of the grid is the query pair (2y, 2y + 1)
    SwgDiagWork wk;          // the classes, each with the W it is launched with
    int qq_per_cu = 1;       // qq: the bulk's workgroups per CU (LDS decides)
    uint64_t bound_max = 0;  // the largest score any query of the batch can reach
    size_t lq_max = 0;
    bool dev_topk = false;   // the top-K is selected on the device (no score array asked for, k within its capacity)
    size_t n_slots = 0;      // scores per query: the database's slots
    size_t chunk_queries = 0, first_chunk = 0;
    // What a chunk of Qb queries indexes, in the units the kernels index by: rows of the grid (profiles, queues), and rows
    // of n_slots scores.  With qq an odd chunk indexes ONE SCORE ROW MORE than it has queries -- the absent partner of its
    // last query has a row of its own everywhere (nothing reads it back).
    size_t grid_rows(size_t Qb) const { return qq ? (Qb + 1) / 2 : Qb; }
    size_t score_rows(size_t Qb) const { return qq ? 2 * grid_rows(Qb) : Qb; }
    // what the buffers hold
    size_t score_rows_cap = 0, grid_rows_cap = 0; // score_rows / grid_rows of the first chunk
    size_t order_entries = 0;                     // query offsets and (qq) query order of a chunk: one more than its queries
    uint32_t class_queue_dwords = 0;              // queue dwords of one class of one grid row (a row's stride is twice that)
    size_t rank_word_base = 0, queue_dwords = 0;  // the per-SIMD rank words of the two classes follow the queues
    size_t prof_row_bytes[2] = {0, 0};            // profile bytes of one grid row, per class
};

// A k-mer table on the device and what it was built with; one buffer per table, so searches that alternate between
// two of them build each once per epoch.
struct SwgKmerTable {
    uint8_t *d = nullptr;
    size_t cap = 0;     // bytes allocated
    uint64_t epoch = 0; // the (query, scoring) epoch it holds (0: nothing; a re-allocated table loses it)
    int k = 0, segments = 0;
    int bits = 0;       // of an entry: 8 or 16 (swg_kmer_table_bits, or 16 under option "prune_table_bits")
    bool holds(uint64_t e, int k_, int S, int bits_) const { return d && epoch == e && k == k_ && segments == S && bits == bits_; }
};
// The bound a pruned search cuts by: k (0: not pruned), its segments S, and the segments of the levels behind it,
// [level - 2] (0: none)
struct SwgPruneChoice {
    int kmer = 0, segments = 0;
    int refine[SWG_REFINE_LEVELS] = {};
    int gate = 0; // 1: the first level's launch is gated (swg_prune_gate_choice)
};

// One search in flight: its timing events, host-side landing buffers and what swg_search_end
// needs to finish it.  Device buffers are shared: everything of one context runs in stream
// order, so search i+1 cannot touch them before search i has copied its results out.
#define SWG_MAX_INFLIGHT 4
struct SwgSlot {
    hipEvent_t ev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev_done = nullptr; // polled from user space instead of a blocking stream sync
    SwgSearchPlan plan;           // what the search decided (launch_diag reads its score_bound: f16_wipe)
    bool side = false;            // this search's top-K and read-out were queued on the read-out stream (stream3)
    bool busy = false;
    swg_db *db = nullptr;
    swg_db::Bufs bufs; // the output buffers this search writes
    size_t k = 0, first_chunk = 0;
    bool want_scores = false, dev_topk = false, need_scores = false, two_ends = false;
    int fill_launches = 0; // launches of the bulk class's fill kernel (passes x segments)
    bool pruned = false;   // the fill was launched stage by stage with cuts (launch_diag)
    int32_t above_min = 0; // swg_search_above: the caller's threshold (0: a top-K / score-array search)
    size_t above_cap = 0;  // ... and the keys its read-out's device buffer had room for
    int fill_f16_launches = 0; // both forms in one class: those of them that ran the f16 cells
    swg_stats st;
    uint64_t *h_cand = nullptr;     // pinned, SWG_TOPK_CAND_CAP keys
    uint32_t *h_counters = nullptr; // pinned, 32 words
    int32_t *h_scores = nullptr;    // pinned landing buffer of the score read-out, grown on demand
    size_t h_scores_cap = 0;        // entries
};

// What swg_fill_batches16 keeps between calls (the reference calls it once per macro-batch with buffers of
// recurring size, src/alignment_cmdline.c:459-509): pinned staging for the batches as they are, their device
// copy, and a database object whose device buffers are re-filled, grown only when a call needs more.
struct SwgBatch16Cache {
    swg_db *db = nullptr;
    size_t slots_cap = 0, pairs_cap = 0, stage_cap = 0;
    uint64_t blocks_cap = 0;
    uint8_t *h_stage = nullptr, *d_stage = nullptr;   // the batches' [max_len][16] bytes, end to end
    uint8_t *h_meta = nullptr;                        // pinned: pair sources, pair lengths, pair offsets, lengths, order
    uint64_t *d_pair_src = nullptr;
    uint32_t *d_pair_len = nullptr;
};

struct swg_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr; // long-pair kernel runs beside the bulk kernel
    hipStream_t stream3 = nullptr; // top-K and read-out of a finished fill, beside the next search's fill
    int n_cu = 0;
    unsigned long n_begun = 0; // searches queued so far (the read-out stream is made for the second)
    std::string err;
    // scoring
    bool have_scoring = false;
    int8_t sub[32][32];
    int gap_open = 0, gap_extend = 0;
    // query: the host copy, and pinned staging buffers for the copy to the device (a buffer is not
    // written again before the copy that reads it has completed, so set_query / search_begin can be
    // streamed without a wait)
    std::vector<int8_t> query;
    int8_t *h_query_stage[4] = {nullptr, nullptr, nullptr, nullptr};
    size_t h_query_stage_cap[4] = {0, 0, 0, 0};
    hipEvent_t ev_query_stage[4] = {nullptr, nullptr, nullptr, nullptr};
    int query_stage_next = 0;
    // a position-specific query (swg_set_query_pssm): pssm[i*32 + b] scores query position i against residue b.  While
    // query_pssm is set it is the query (and `query` is empty); swg_set_query clears it again.
    std::vector<int8_t> pssm;
    bool query_pssm = false;
    bool gapless = false; // set for the duration of a swg_search_gapless call: plan_search prices the gaps out
    int32_t above_min = 0; // set for the duration of a swg_search_above call: the caller's threshold
    // query length of either form: what every lq of the planner, the profiles and the traceback is
    size_t query_len() const { return query_pssm ? pssm.size() / 32 : query.size(); }
    // options
    long opt_force_bits = 0, opt_cols = 0, opt_max_waves = 0, opt_workgroups = 0, opt_engine = 0, opt_group = 0, opt_long_split = 0, opt_autotune = 1, opt_dynamic = 1, opt_prio_share = 150, opt_long_helps = 0, opt_wide = 1, opt_side_readout = 1, opt_f16 = 1, opt_qq = 1, opt_last_pass = 1, opt_f16_pair = 0;
    long opt_batch_geometry = 0; // 1: a batch (swg_search_multi*, swg_search_lists*) takes options cols_per_wave / group_lanes instead of going one by one (tests)
    long opt_wave_budget = 0, opt_q32_waves = 0;
    long opt_bounds_groups = 0; // lane groups of a bounds launch (swg_align_bounds*), 0: auto (option "bounds_groups": tests)
    uint32_t bounds_last[4] = {0, 0, 0, 0}; // the last bounds call: pairs on its kernel, pairs on the fallback, its launches, its column limit
    long opt_batch = 8, opt_batch_blocks = 0; // work queue: pairs one request claims where pairs are short (blocks; 0: about 40 us of work, from the geometry)
    long opt_prune = 1, opt_prune_head = 4; // hits-only pruning (options "prune", "prune_head": swg.h)
    bool in_batch = false;                  // a batch call is searching its queries one after another: never pruned
    long opt_above_batch = 0;               // option "above_batch": the route of swg_search_above_multi* (swg_above_multi_route)
    swg_prune_info prune_last = {}; // what the search last ended on this context left out (swg_prune_last)
    SwgPruneChoice prune_choice;    // the bound of the search last begun on this context (plan_prune; tests)
    SwgColMax prune_colmax;                 // the bound's table for the current (query, scoring) ...
    uint64_t prune_colmax_epoch = 0;        // ... epoch (0: not built)
    // the k-mer form of the bound (option "prune_kmer": 0 auto, 1 colmax, 4, 5): the class profile and the tables -- the
    // first level's of k = 4 and k = 5, the second level's of k = 4 in 64 or 128 segments --, device buffers built on the
    // fill's stream in front of the first pruned search of an epoch that wants them (ensure_kmer_table)
    long opt_prune_kmer = 0;
    long opt_prune_segments = 0; // option "prune_segments": 0 auto, 1..32
    long opt_prune_refine[SWG_REFINE_LEVELS] = {}; // options "prune_refine" .. "prune_refine5", [level - 2]: 0 auto, 1 off, or a forcing value (SWG_REFINE_LEVEL)
    long opt_prune_gate = 0;    // option "prune_gate": 0 auto, 1 off, 2 wherever the first level is segmented
    long opt_prune_table_bits = 0; // option "prune_table_bits": 0 auto (bytes where they hold every entry), 16
    long opt_prune_cut = 0;      // option "prune_cut": 0 pair by pair, 1 the prefix of the length order
    int8_t *d_kmer_cprof = nullptr;
    size_t d_kmer_cprof_cap = 0;
    SwgKmerTable kmer_first[2];                     // [k - 4]
    SwgKmerTable kmer_refine[SWG_REFINE_LEVELS];    // the table each level behind the first owns, [level - 2]
    uint64_t kmer_builds = 0, kmer_refine_builds[SWG_REFINE_LEVELS] = {}; // builds queued so far: the first level's, and level by level (tests)
    bool kmer_refine_refused[SWG_REFINE_LEVELS] = {}; // a reserved table's allocation failed once: this context searches without the level
    uint32_t opt_seg_blocks = SWG_DYN_SEG_BLOCKS; // token blocks per launch of the multi-pass fill (option "segment_blocks": tests)
    // device state
    int8_t *d_sub = nullptr;
    int8_t *d_query = nullptr;
    size_t d_query_cap = 0;
    int8_t *d_pssm = nullptr; // [lq][32], the device copy of pssm
    size_t d_pssm_cap = 0;
    // [0] int16, whole 4-column chunks per lane; [1] int32 (bin-based kernels); [2] / [3] int16 in per-lane
    // slices padded to whole chunks, long class / bulk; [4] / [5] int32 in 2-column chunks (work-queue
    // int32 kernel), bulk or list / long class
    // int32 kernel), bulk or list / long class; [6] int16, the re-run of the pairs the f16 cells flagged
    uint8_t *d_profile[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    size_t d_profile_cap[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t profile_tag[8] = {0, 0, 0, 0, 0, 0, 0, 0}; // identifies (query, scoring, geometry) currently built
    uint64_t epoch = 1;               // bumps whenever scoring or query change
    uint32_t *d_scratch = nullptr;
    size_t d_scratch_cap = 0; // dwords
    SwgBatch16Cache b16;
    // swg_calibrate*: options "calib_seqs", "calib_len", "calib_seed", and the random database of the last (normalised
    // freq, seqs, len, seed) asked for -- generated, packed and uploaded on first use, released by swg_destroy
    long opt_calib_seqs = 8192, opt_calib_len = 384, opt_calib_seed = 1;
    struct {
        swg_db *db = nullptr;
        double freq[32] = {};
        long seqs = 0, len = 0, seed = 0;
    } calib;
    std::vector<int32_t> calib_iters; // Newton steps of each query's fit in the last swg_calibrate* call (tests)
    long opt_pssm_msa_mb = 1024; // swg_pssm_build*: MiB of device rows (sum rows x lq) one group of queries may take (option "pssm_msa_mb")
    SwgSlot slots[SWG_MAX_INFLIGHT];
    SwgSlot *cur = nullptr; // slot whose events the launch helpers record into
    int next_slot = 0;
    long opt_pssm_blocks = 0;    // swg_pssm_build*: 1: per-column alignment blocks (option "pssm_blocks"); 0: the whole query is every column's block
    long opt_pssm_purge = 0;     // swg_pssm_build*: percent identity at which a hit is dropped, 50..100 (option "pssm_purge"); 0: no purge
    long opt_comp_scale = 32;    // swg_comp_adjust*: the scale F of the rescaled scores, 1..64 (option "comp_scale")
    uint32_t comp_last[12] = {}; // the last swg_comp_adjust* call (swg_debug_comp_last)
};

// Internal status (positive: never a public SWG_ERR_*): a database built from 16-lane batches has pair tokens only, and
// this search needs residue bytes by rank (the bin image, fixed streams); swg_fill_batches16 then takes its host route.
#define SWG_TAKE_HOST_ROUTE 1
int swg_set_global_error(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
int swg_set_ctx_error(swg_ctx *ctx, int code, const char *fmt, ...)
    __attribute__((format(printf, 3, 4)));
void swg_db_release_device(swg_db *db);
// everything a search built or allocated for this database on the device (layouts, output buffers); the uploaded image stays
void swg_db_release_search_state(swg_db *db);
// the residue bytes a database's code_off points into: its own, or for a view its root's
inline const uint8_t *swg_db_codes(const swg_db *db) { return (db->root ? db->root : db)->codes.data(); }
// The slot tables of the six-frame translation of `parent` (swg_db_translate; swg_pack.cpp, no GPU): everything of db's
// host image but the residue bytes (sized, not written), built from the parent's lengths and original indices alone the
// way swg_db_pack builds them from the frames given in index order; dst[6 s + g] = the slot of frame g of the parent's
// slot s (~0u for an empty slot).  Throws what the containers throw.
void swg_translate_slots(const swg_db *parent, swg_db *db, std::vector<uint32_t> *dst);
// *out = *p, or genetic code 1 for p NULL; SWG_ERR_ARG (global error, naming `what`) for an entry outside 1..31
// (swg_translate_host.cpp)
int swg_translate_params_get(const char *what, const swg_translate_params *p, swg_translate_params *out);
// length of frame f or 3 + f of a sequence of L nucleotides
inline uint32_t swg_frame_len(uint32_t L, uint32_t f) { return L >= f + 3u ? (L - f) / 3u : 0u; }
// Views, host side (swg_pack.cpp; no GPU).  swg_view_select: the ROOT's slots that `indices` (original indices, any
// order, duplicates collapse, those of other shards ignored) select among parent's sequences, ascending; SWG_ERR_ARG for
// an index outside the whole database.  swg_view_host: the view of those slots with its whole host image, holding a
// reference on the root.  swg_db_views_alive: views that keep this database's bytes alive.
// marks (or NULL): a scratch vector the caller keeps between many calls on one database, all zero between them -- a short
// list then costs its own length, not the database's.
int swg_view_select(const swg_db *parent, const uint32_t *indices, size_t n, std::vector<uint32_t> *slots,
                    std::vector<uint8_t> *marks = nullptr);
swg_db *swg_view_host(swg_db *parent, const std::vector<uint32_t> &slots);
size_t swg_db_views_alive(const swg_db *db);
// test hook: swg_view_select's answer (out has room for n entries; slots of the root of `db`)
extern "C" int swg_debug_view_ranks(const swg_db *db, const uint32_t *indices, size_t n, uint32_t *out, size_t *n_out);
// Candidate lists (swg_search_lists), host side (swg_pack.cpp; no GPU): the job database J of the queries
// [q0, q0 + nq) -- query i's candidates are cand[c_off[i] .. c_off[i + 1]) --, a view-like selection per query laid end to
// end.  Segment i = the distinct slots of db's root that list i selects (swg_view_select: ascending, so longest first),
// filled up to a whole pair with an empty slot (~0u); row i's pairs are [row_pairs[i], row_pairs[i + 1]).
struct SwgListJobs {
    std::vector<uint32_t> slots;        // J slot -> the root's slot, ~0u = the empty slot that ends an odd segment
    std::vector<uint64_t> row_pairs;    // [nq + 1]
    std::vector<uint32_t> entry_job;    // [entries of the nq lists] J slot of entry c_off[q0] + e, ~0u = ignored (not held here)
    std::vector<uint64_t> row_residues; // [nq] residues of the row's distinct held candidates
    std::vector<uint32_t> row_longest;  // [nq] the longest of them
    std::vector<uint64_t> pair_blocks;  // [pairs + 1] 4-row token blocks before each pair of J (two reset rows + the longer sequence)
    uint64_t entry0 = 0;                // c_off[q0]
};
int swg_list_jobs(const swg_db *db, const uint32_t *cand, const uint64_t *c_off, size_t q0, size_t nq, SwgListJobs *J);
// The workgroups of one launch over J, dealt by work: every row with pairs gets one, the rest of `resident` (the chip's
// resident workgroups of the launch's geometry) goes to the rows in proportion to their token blocks (equal_shares: one
// share per row, the comparison the dealing is measured against), never more than a row's pairs can keep busy at per_wg
// lane groups per workgroup; rows with the most work first, empty rows none.  out: (row, index within the row) per workgroup.
void swg_lists_deal(const SwgListJobs &J, uint64_t per_wg, uint64_t resident, bool equal_shares, std::vector<uint2> *out);
// test hook: that table for the lists' job database, two words per workgroup (copied when it fits cap workgroups)
extern "C" int swg_debug_list_deal(const swg_db *db, const uint32_t *cand, const uint64_t *c_off, size_t n_queries, uint64_t per_wg,
                                   uint64_t resident, uint32_t *out, size_t cap, size_t *n_wgs);
// test hook: J's slots (copied when they fit cap) and the n_queries + 1 pair-range prefix
extern "C" int swg_debug_list_jobs(const swg_db *db, const uint32_t *cand, const uint64_t *c_off, size_t n_queries, uint32_t *slots_out,
                                   size_t cap, size_t *n_slots, uint64_t *row_pairs_out);
// test hook: the pair-token image as the device built it, or as the host restatement builds it
// test hook: the next visit of the named site throws std::bad_alloc (swg_api.cpp); 0 disarms.  Site 4 throws nothing: the
// next growth of swg_search_above_multi's key pool finds no device memory, and that chunk is selected on the host.  Sites
// 5 and 6 throw nothing either: the next reservation of the fourth level's table (5) or of the fifth's (6) is refused as
// if the device had no room, and the context searches on without the level (reserve_refine_table: site 1 + level)
extern "C" void swg_debug_fail_alloc(int site);
extern "C" int swg_debug_plan(const swg_db *db, size_t lq, int n_cu, int32_t *out);
// a gapless search's plan: out[0..5] = route (1 gapless cells, 0 gapped machinery), K, G, W, workgroups, passes
extern "C" int swg_debug_plan_gapless(const swg_db *db, size_t lq, int n_cu, int32_t *out);
// the same for the packed-f16 cells (option f16_pair: 0 auto, 1 perm, 2 fma), out[0..15]: swg_debug_plan's 13 values, then
// the bulk's pairing (1 fma, 0 v_perm_b32), its workgroup's LDS bytes, the long class's pairing
extern "C" int swg_debug_plan_f16(const swg_db *db, size_t lq, int n_cu, long f16_pair, int32_t *out);
// test hook: the planner's answer for a FORCED geometry (options cols_per_wave, group_lanes, max_waves; 0 = free) with
// long_split = -1 (one class), on cells of `form` (0 int16 -- the wide form plans alike --, 2 packed f16, 3 gapless) with
// option f16_pair, without a device.  "No plan" is an answer, not an error: SWG_OK with out[0] = 0 and the rest zero.
// out[0..15] as swg_debug_plan_f16 (the pairing and the LDS bytes for every form); out[12], the last pass's own columns
// per lane, is 0 with last_pass = 0 (option last_pass).
extern "C" int swg_debug_plan_forced(const swg_db *db, size_t lq, int n_cu, long cols, long group, long waves, int form,
                                     long f16_pair, int last_pass, int32_t *out);
// test hooks (swg_api.cpp): plan_search's answers for the two engines the work queue does not serve, without a device, for
// a query idx[0 .. lq) under the 32 x 32 table `rows`.  "No plan" is SWG_OK with out[0] = 0.
// swg_debug_plan_streams: options engine = 2, work_queue = 0, f16 = 0, long_split = -1, cols_per_wave, group_lanes,
// max_waves, workgroups (0 = free): out[0..7] = classes, K, G, W, passes, workgroups, streams, wide form.
// swg_debug_plan_systolic: option engine = 1 with force_bits (0 / 32), cols_per_wave, max_waves, workgroups, f16:
// out[0..11] = planned, K, W, passes, workgroups, f16 cells, the instantiation's most wavefronts, bits, an int32 re-score
// follows (a score can reach 32767), and that re-score's K, W, passes.
// swg_debug_systolic_variants: (K, max_waves) of every systolic instantiation of `bits`; returns their number.
extern "C" int swg_debug_plan_streams(const swg_db *db, const int8_t *rows, const int8_t *idx, size_t lq, int n_cu, long cols, long group,
                                      long waves, long workgroups, int32_t *out);
extern "C" int swg_debug_plan_systolic(const swg_db *db, const int8_t *rows, const int8_t *idx, size_t lq, int gap_open, int gap_extend, int n_cu,
                                       long force_bits, long cols, long max_waves, long workgroups, long f16, int32_t *out);
extern "C" int swg_debug_systolic_variants(int bits, int32_t *out, size_t cap);
// test hooks: what a batch launches on cells of `form` (0 packed int16, 2 packed f16; the hooks have no scoring system, so
// the caller says which cells the score bounds allow), without a device: the geometry rules of plan_batch and plan_lists
// (swg_api.cpp, which share them with these hooks) for options cols_per_wave = cols, group_lanes = group (0 = free),
// batch_geometry and, for a batch, qq.  The engine choice (systolic against lane groups) is not part of the answer: it is
// the answer under option engine = 2.  out[0..7] = launched as a batch (0: one by one, and the rest zero), K, G, W,
// workgroups per CU, two queries per lane, LDS bytes of a workgroup, classes.  swg_debug_plan_batch: n_queries queries, the
// longest of lq_max columns, against db.  swg_debug_plan_lists: a job table of n_pairs pairs, pair p of sequences of
// pair_lens[2p] and pair_lens[2p + 1] residues (0: the empty slot of an odd list), in any order.
extern "C" int swg_debug_plan_batch(const swg_db *db, size_t lq_max, size_t n_queries, int n_cu, int form, int qq_on, long cols, long group,
                                    long batch_geometry, int32_t *out);
extern "C" int swg_debug_plan_lists(const uint32_t *pair_lens, size_t n_pairs, size_t lq_max, int n_cu, int form, long cols, long group,
                                    long batch_geometry, int32_t *out);
// test hook: the launch log (swg_launch_log_add, swg_internal.h).  swg_debug_launch_log(on): clears the log and switches
// it on (1) or off (0); off by default.  While on, the launchers append records until SWG_LAUNCH_LOG_CAP are held (later
// launches are counted, not kept).  swg_debug_launch_log_read: copies up to cap records of SWG_LAUNCH_LOG_FIELDS int32
// each {family, K, G, W, form, edges, flag, workgroups, grid_rows, list}; returns the launches seen since the log was cleared.
#define SWG_LAUNCH_LOG_CAP 4096
#define SWG_LAUNCH_LOG_FIELDS 10
extern "C" void swg_debug_launch_log(int on);
extern "C" size_t swg_debug_launch_log_read(int32_t *out, size_t cap);
// the systolic engine's estimate from the host's bin table (swg_diag_host.cpp); it is picked over the lane groups when it
// wins by this margin (both models are good to about 10 %)
#define SWG_SYSTOLIC_MARGIN 0.85
double swg_systolic_estimate_ms(const swg_db *db, size_t lq, int n_cu, int *best_K, bool f16 = false);
double swg_diag_short_pair_factor(const swg_db *db, const SwgDiagPlan &pl, int form); // lane groups on short pairs: what the fitted estimate misses
extern "C" int swg_debug_engine(const swg_db *db, size_t lq, int n_cu, int form, int32_t *out);
extern "C" int swg_debug_split(swg_db *db, size_t lq, uint64_t qbound, uint64_t *out);
// decisions plan_search (swg_api.cpp) makes on top of the planner's geometry (host only: swg_diag_host.cpp)
bool swg_plan_last_pass(const SwgDiagPlan &pl, size_t lq, int *variant, int *K);
uint32_t swg_split_rows(size_t lq, uint64_t qbound);
void swg_db_split_at(swg_db *db, uint32_t rows);
extern "C" int swg_debug_pair_tokens(swg_ctx *ctx, swg_db *db, int from_host, uint32_t *out, size_t cap_dwords,
                                     size_t *n_dwords);

// test hook: the Newton steps of each query's fit in the context's last swg_calibrate* call (copied when they fit cap)
extern "C" int swg_debug_calib_iters(const swg_ctx *ctx, int32_t *out, size_t cap, size_t *n);

// swg_trace.hip: the pairs of one alignment call.  Query i is src[q_offsets[i] .. q_offsets[i+1]) in positions (index
// bytes, or PSSM rows of 32 bytes), its hits are hits[i*k .. i*k + n_hits[i]), and out / ops take the same layout.
// swg_align_hits is the batch of one query, the context's.
struct SwgTraceBatch {
    const char *fn; // the entry point, for messages
    const int8_t *src;
    bool pssm;
    const uint64_t *q_offsets;
    size_t n_queries;
    const swg_hit *hits;
    size_t k;
    const size_t *n_hits;
};
// The argument checks of the batch entry points (*total = hits of all rows; SWG_OK with 0: nothing to do), and every hit
// of a checked batch through the traceback's kernel, guarded against C++ exceptions (ops == NULL: coordinates only).
// stride0: paths are wanted with an ops_stride of 0 (refused where it always was: after the database, before the rows)
int swg_trace_check_batch(swg_ctx *ctx, const swg_db *db, const SwgTraceBatch &tb, const swg_alignment *out, bool stride0,
                          size_t *total);
// One pair of a traceback launch and what the kernel leaves for it (device structs of swg_trace.hip).  A job carries its
// own query, so one launch can hold the hits of several queries of a batch; the offsets into the launch's predecessor
// bytes, rotating diagonals and paths are the job's own because all three are sized by its lq (and the path by its len).
struct SwgTraceJob {
    uint64_t q_off;    // into the batch's query: first index byte, or first PSSM row
    uint64_t res_off;  // into the gathered residue indices
    uint64_t dir_off;  // into the launch's predecessor bytes: (lq + len - 1) * lq of them
    uint64_t diag_off; // into the launch's rotating anti-diagonals (kernels without LDS): 9 * (lq + 1) words
    uint64_t ops_off;  // into the launch's paths: lq + len + 1 bytes (a path has at most lq + len steps)
    uint32_t lq;       // query length
    uint32_t len;      // database sequence length
};
struct SwgTraceOut {
    int32_t score;
    uint32_t q_begin, q_end, d_begin, d_end, n_ops, pad[2];
};
// An optional sink of a traceback call: run(user, v, stream) is called once per launch, after the launch's kernel was
// queued on `stream` and before the call waits for it, while the device buffers of the launch are valid -- jobs[n_jobs]
// with their results out[n_jobs], their paths in ops (job j's at jobs[j].ops_off) and the gathered residues res (job j's
// at jobs[j].res_off); dest[j] (host) is job j's slot i*k + j' of the batch.  What it queues on the stream is waited for
// with the launch.  A failure ends the call with SWG_ERR_HIP.
struct SwgTraceLaunchView {
    const SwgTraceJob *d_jobs;
    const SwgTraceOut *d_out;
    const char *d_ops;
    const int8_t *d_res;
    const size_t *dest;
    size_t n_jobs;
};
struct SwgTraceSink {
    void *user;
    hipError_t (*run)(void *user, const SwgTraceLaunchView &v, hipStream_t stream);
};
int swg_trace_align_batch(swg_ctx *ctx, const swg_db *db, const SwgTraceBatch &tb, size_t total, swg_alignment *out, char *ops,
                          size_t ops_stride, const SwgTraceSink *sink = nullptr);
// The launch rule of the traceback's kernels, which swg_align_hsps* (swg_hsps.hip) launches its own kernel by: 256 lanes a
// pair; a launch holds the queries of one class -- one power-of-two range of lengths among those whose nine rotating
// diagonals fit LDS (so its dynamic LDS, sized by its longest query, is less than twice what any of its jobs needs), or
// every longer query -- and at most 2 GiB of predecessor bytes (a single larger pair goes alone).
#define SWG_TRACE_THREADS 256
#define SWG_TRACE_LDS_COLS 1700 /* 9 * (cols + 1) * 4 bytes <= 60 KB */
inline int swg_trace_class(uint32_t lq) { return lq > SWG_TRACE_LDS_COLS ? 0 : 32 - __builtin_clz(lq); }
// One launch: jobs [b, e) of the launch order, the bytes its buffers need, its longest query.
struct SwgTraceLaunch {
    size_t b, e;
    uint64_t dir, diag, ops;
    uint32_t lq_max;
};
// The jobs of a checked batch in launch order (by query length, stable), dest[h] = job h's slot i*k + j of the batch, the
// launches, the gathered residue indices, and the most bytes any launch needs of each buffer.
struct SwgTracePlan {
    std::vector<SwgTraceJob> jobs;
    std::vector<size_t> dest;
    std::vector<SwgTraceLaunch> launches;
    std::vector<int8_t> res;
    uint64_t max_dir = 4, max_diag = 4, max_ops = 4;
};
// ... for a call whose jobs own `paths` path slots of lq + len + 1 bytes each, which count against a launch's 2 GiB;
// refuses what swg_trace_check_pairs refuses, with the same messages.  May throw (host vectors).
int swg_trace_plan_batch(swg_ctx *ctx, const swg_db *db, const SwgTraceBatch &tb, size_t total, uint32_t paths, SwgTracePlan *plan);
// The refusals of swg_trace_align_batch that depend on the database (a hit this shard does not hold, a pair outside what
// a traceback holds), on their own: a caller that runs a batch in several calls refuses all of it first.
int swg_trace_check_pairs(swg_ctx *ctx, const swg_db *db, const SwgTraceBatch &tb);

// swg_pssm_host.cpp: the checks every PSSM construction makes before anything else (the background P and the mask of A
// from freq, the pseudocount, lambda of (sub, P)); SWG_ERR_ARG with a message naming fn in swg_global_error().
extern "C" int swg_freq_weights(const double *freq, double w[32], double *tot_out); // host/swg_synth.c
int swg_pssm_check_model(const char *fn, const int8_t sub[32][32], const double *freq, double pseudocount, double P[32],
                         uint32_t *mask, double *lambda);
// swg_bounds.hip, test hook: what the context's last swg_align_bounds* call did -- out[0..3] = pairs on the bounds kernel,
// pairs on the fallback (the traceback's kernel), launches of the bounds kernel, its column limit
#define SWG_BOUNDS_COLS 1024         /* 64 lanes x 16 columns */
#define SWG_BOUNDS_LEN (1u << 20)    /* a sequence below this many residues: the tag holds its origin in 20 bits */
extern "C" int swg_debug_bounds_last(const swg_ctx *ctx, uint32_t out[4]);

// swg_comp.hip / swg_comp_host.cpp: composition-based score adjustment (include/swg.h).
// The option of the call family ("comp_scale"), checked and stored where the family lives: swg_set_option asks this about a
// key it does not hold itself.  *known = whether the key is this family's; the return value is the call's when it is.
int swg_comp_set_option(swg_ctx *ctx, const char *key, long value, bool *known);
// Host side of the rule (no GPU).  swg_comp_counts: C[a][s + 128] of one query (index bytes scored by sub, or PSSM rows).
// swg_comp_lambda_std: lambda(hP) -> status 0, 1 (does not exist), 2 (did not converge); *lambda is 0 unless 0 is returned.
// swg_comp_pair: the whole rule for one pair from the query's count table, its lambda_std (with that status) and the
// sequence's table indices.  swg_comp_pairs_host: the pairs the fill kernel cannot hold, on every core.
#define SWG_COMP_COLS 2048 /* 64 lanes x 32 columns: the fill kernel's widest instantiation */
void swg_comp_counts(const int8_t sub[32][32], const int8_t *query, const int8_t *pssm, size_t lq, uint32_t *C);
int swg_comp_lambda_std(const uint32_t *C, const double P[32], uint32_t mask, double *lambda);
void swg_comp_pair(const int8_t sub[32][32], int go, int ge, const int8_t *query, const int8_t *pssm, size_t lq, const uint32_t *C,
                   uint32_t mask, double lambda_std, int std_status, const int8_t *seq, size_t len, int F, swg_comp_result *out);
struct SwgCompHostPair {
    size_t query, cq, dest; // the batch's query, its place among the queries that have hits (C, lambda_std, std_status), the slot of `out`
    uint32_t index;     // the sequence's original index
    size_t len;         // its length
};
bool swg_comp_pair_fits(size_t lq, size_t len, int go, int ge, int F); // the refusal of a pair whose int32 cells could wrap
int swg_comp_pairs_host(const swg_db *db, const int8_t sub[32][32], int go, int ge, const int8_t *src, bool pssm,
                        const uint64_t *q_offsets, const uint32_t *C, uint32_t mask, const double *lambda_std, const int *std_status,
                        int F, const SwgCompHostPair *pairs, size_t n, swg_comp_result *out);
// test hook: what the context's last swg_comp_adjust* call did -- out[0..11] = pairs on the fill kernel, pairs on the host
// route, launches of the fill kernel, its column limit, the scale F, then the pairs of each of its six instantiations,
// narrowest first, and 0
extern "C" int swg_debug_comp_last(const swg_ctx *ctx, uint32_t out[12]);

// swg_diag_host.cpp (host only)
// geometry of both classes for one query length on one device; returns the number of
// classes (0: the diagonal engine cannot run this with the given options)
int swg_plan_diag_work(const swg_db *db, size_t lq, int n_cu, long opt_cols, long opt_group, long opt_waves,
                       long opt_long_split, bool allow_split, bool work_queue, SwgDiagWork *wk, double copies = 1.0,
                       int form = 0, // form: the cells the plan is for (2: packed f16, 8.5 instead of 10 instructions per column pair)
                       long f16_pair = 0); // form 2: the pairings to consider (option f16_pair: 0 both, 1 perm only, 2 fma where it fits)
// every geometry the model considered, best estimate first (the autotuner times the first few)
int swg_plan_diag_candidates(const swg_db *db, size_t lq, int n_cu, long opt_cols, long opt_group, long opt_waves,
                             long opt_long_split, bool allow_split, bool work_queue,
                             std::vector<SwgDiagWork> *cands, double copies = 1.0, int form = 0, long f16_pair = 0);
// 0 on success; -1 when the database is too large for 32-bit block offsets.  tok == NULL: only
// pair_off (the tokens themselves are built on the device, swg_launch_build_tokens); otherwise also
// the host builder's token image, which the tests compare the device's with.
int swg_build_pair_tokens(const swg_db *db, std::unique_ptr<uint32_t[]> *tok, size_t *tok_dwords,
                          std::vector<uint32_t> *pair_off);
void swg_build_diag_layout(const swg_db *db, uint64_t pair_begin, uint64_t pair_end, uint32_t n_streams,
                           uint32_t streams_per_wg, SwgDiagLayout *out);
// every shard of one database from one global sort (swg_pack.cpp); ready(r, shard) runs on the thread that built shard r
int swg_pack_shards(const int8_t *flat, const uint64_t *offsets, size_t n, int shard_count, swg_db **out,
                    const std::function<int(int, swg_db *)> &ready);
extern "C" unsigned long swg_debug_sort_count(void); // test hook: global sorts run by this process so far
void swg_stage_batches16(const swg_batch16 *batches, const uint32_t *order, const uint64_t *stage_off, size_t lo, size_t hi,
                         uint8_t *stage);
void swg_untranspose_batches16(const swg_batch16 *batches, size_t n_batches, const size_t *first_rec,
                               const uint64_t *rec_off, int8_t *flat);
uint64_t swg_db_pair_count(const swg_db *db);
// rows (2 reset rows + longer length) of the pairs [pair_begin, pair_end): total and longest
uint64_t swg_db_pair_rows(const swg_db *db, uint64_t pair_begin, uint64_t pair_end, uint64_t *longest_rows);
// how many leading (longest) pairs have more than `rows` rows
uint64_t swg_db_pairs_longer_than(const swg_db *db, uint64_t rows);
