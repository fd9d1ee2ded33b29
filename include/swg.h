/*
 * swg.h -- C ABI of libswg: MI355X-native Smith-Waterman protein database search.
 *
 * This is the drop-in boundary for the one hot path of Aseeef/seq-align-gpu:
 * the affine-gap three-state fill `alignment_fill_matrices`
 * (reference src/alignment.c:47-187) as it is driven, one query against a
 * database, by the OpenMP batch-of-batches loop at
 * reference src/alignment_cmdline.c:501-509.  Plain pointers and sizes only;
 * no C++ or torch types; no function here aborts or exits the process (the
 * reference asserts/exit()s: src/alignment.c:63-66, src/alignment_scoring.c:78-79)
 * -- every entry point returns 0 or a negative swg_status and leaves a message
 * retrievable with swg_last_error()/swg_global_error().
 *
 * Residues are exchanged as the reference's substitution-table indices
 * (`letters_to_index`, reference src/alignment_scoring.c:70-81): 1..26 for
 * A..Z case-folded, 31 for '*'.  Index 0 is reserved by this library as the
 * padding residue and is rejected in input.
 *
 * Threading: a swg_ctx is not thread-safe; distinct contexts may be used from
 * distinct threads (the reference's fill is re-entrant per aligner_t,
 * src/alignment_cmdline.c:504-507).  All calls are synchronous at the ABI.
 */
#ifndef SWG_H
#define SWG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SWG_ABI_VERSION 3

typedef enum swg_status {
    SWG_OK = 0,
    SWG_ERR_ARG = -1,     /* bad argument (NULL, zero length, out-of-range value) */
    SWG_ERR_HIP = -2,     /* HIP runtime / launch failure; text in swg_last_error */
    SWG_ERR_NOMEM = -3,   /* host or device allocation failed */
    SWG_ERR_STATE = -4,   /* call order violated (no scoring / no query / db not resident) */
    SWG_ERR_RESIDUE = -5, /* residue index outside 1..31 (reference: exit(1) in letters_to_index) */
    SWG_ERR_IO = -6,      /* file could not be read / parsed (host helpers) */
    SWG_ERR_NODEVICE = -7 /* no usable GPU: the product path never falls back to the CPU */
} swg_status;

typedef struct swg_ctx swg_ctx; /* one GPU, one stream, one query + scoring system */
typedef struct swg_db swg_db;   /* length-sorted, binned, dword-packed database (shard) */

typedef struct swg_config {
    int device;      /* HIP device ordinal */
    int reserved[7]; /* must be zero */
} swg_config;

/* One hit of the top-K report.  Order: higher score first, ties by lower
 * database index (total order => deterministic across shards and GPUs). */
typedef struct swg_hit {
    int32_t score;
    uint32_t index; /* ORIGINAL database index (position in the caller's input) */
} swg_hit;

/* Filled by swg_search.  Times are device times from HIP events on the
 * library's stream; the reference's `Total Time` likewise counts only the fill
 * (src/alignment_cmdline.c:503-509). */
typedef struct swg_stats {
    uint64_t cells;         /* lq * sum(len_i): real cells, what GCUPS counts */
    uint64_t cells_padded;  /* cells actually computed (bin + strip padding) */
    uint64_t bytes_alg;     /* algorithmic HBM bytes of the fill */
    uint64_t n_rescored;    /* SEQUENCES that reached the ceiling of the cells they ran on and were run again on wider
                             * ones.  cell_form 0, 1: those whose int16 / wide score saturated (run again in int32);
                             * 2: those the f16 cells flagged (score >= 4096; their PAIRS are run again on int16 / wide
                             * cells, and only what saturates those too goes on to int32 -- not counted a second time);
                             * 4, 5: the f16 part's flagged sequences plus the int16 / wide part's saturated ones */
    double fill_ms;         /* 16-bit fill kernel (or the int32 fill when forced) */
    double rescore_ms;      /* everything after the fill that runs flagged work again: collection of the lists, the int16 /
                             * wide list re-run of what the f16 cells flagged, the int32 re-score */
    double topk_ms;         /* device top-K selection */
    double total_ms;        /* first kernel start .. last kernel end */
    int32_t path_bits;      /* 16 or 32: arithmetic of the main fill */
    int32_t cols_per_wave;  /* K: query columns held in registers per wavefront (systolic) / per lane (diagonal) */
    int32_t waves;          /* W: wavefronts of one workgroup (systolic: chained over the query) */
    int32_t passes;         /* query passes: systolic ceil(lq / (W*K)), diagonal ceil(lq / (group_lanes*K)) */
    int32_t workgroups;     /* grid size of the fill */
    int32_t engine;         /* 1 systolic (waves chained over the query), 2 diagonal (lane groups) */
    int32_t group_lanes;    /* diagonal engine: lanes sharing one pair of sequences (16/32/64) */
    int32_t streams;        /* diagonal engine: lane groups working in parallel */
    int32_t long_pairs;     /* diagonal engine: longest pairs run as their own class, 64 lanes each */
    int32_t long_cols_per_lane;
    int32_t long_streams;
    int32_t work_queue;     /* diagonal engine: 1 = pairs handed out by the device-side work queue */
    /* Two classes (bulk and long pairs) are launched on two HIP streams and are MEANT to run side by
     * side on every CU (the plan's cost model assumes it).  Whether they did is measured, not assumed:
     * each kernel stamps the wall clock when its first wavefront starts and when its last one ends.
     * 1 = the long class started before a tenth of the bulk's run had passed; 0 = it did not (streams
     * sharing a hardware queue -- a host program with many HIP streams should raise GPU_MAX_HW_QUEUES --
     * or its workgroups found no room); -1 = a single class, nothing to overlap. */
    int32_t classes_overlapped;
    /* launches of the main fill kernel in this search: one per pass of the query, times the segments a
     * pass of a very large database is cut into; 1 for a query of one pass */
    int32_t fill_launches;
    /* the cells the 16-bit fill ran on: 0 packed int16 (scores to 32767), 1 the wide int16 form (to 65535),
     * 2 packed f16 with gfx950's three-operand maxima (exact below 4096; a sequence that reaches it is flagged, and
     * the flagged pairs are run again on the int16 cells -- the wide form if the query can pass 32767 -- by the same
     * kernel in list mode; int32 only for what saturates those too), 3 (swg_search_multi only) the f16 cells with two
     * QUERIES per lane against one sequence instead of two sequences against one query, 4 both of the 16-bit
     * forms in one search: a query long enough to score beyond 32767 runs the sequences that could reach the f16
     * cells' ceiling -- those of split_rows rows or more -- on the wide form and everything shorter on the f16
     * cells (what those flag all the same is run again on the wide form, so the scores are exact either way), 5 the same
     * with option wide16 = 0: the long sequences on the plain int16 cells, everything from 32767 up re-scored in int32,
     * 6 (swg_search_gapless only) the gapless cells: one state per column in the arithmetic of form 2 (exact below
     * 4096, flagged from there and run again like form 2's flags, with the gaps priced out) */
    int32_t cell_form;
    int32_t split_rows;     /* cell_form 4, 5: the length from which sequences took the int16 cells; else 0 */
    int32_t fill_f16_launches; /* cell_form 4, 5: how many of fill_launches ran the f16 cells; else 0 */
    double fill_f16_ms;     /* cell_form 4, 5: the part of fill_ms spent on the f16 cells; else 0 */
    uint64_t cells_f16;     /* cell_form 4, 5: the real cells computed on the f16 cells; else 0 */
    int32_t last_pass_cols; /* diagonal engine, several passes: columns per lane of the last pass when it has a geometry of
                             * its own (fewer than cols_per_wave); else 0 */
} swg_stats;

/* ---- context ---------------------------------------------------------- */

/* Create a context on cfg->device.  Fails with SWG_ERR_NODEVICE when there is
 * no GPU -- there is deliberately no CPU backend behind this ABI. */
int swg_create(const swg_config *cfg, swg_ctx **out);
void swg_destroy(swg_ctx *ctx);
const char *swg_last_error(const swg_ctx *ctx);
const char *swg_global_error(void); /* errors of calls that have no context */
int swg_abi_version(void);

/* Tuning / test switches.  Keys: "force_bits" (0 auto | 16 | 32),
 * "engine" (0 auto | 1 systolic | 2 diagonal; int16 path only),
 * "cols_per_wave" (0 auto | systolic: 16, 24, 32 or 48 columns per wavefront; diagonal: 2..32 columns per lane),
 * "max_waves" (0 auto | systolic: waves chained over the query, 1..16; diagonal:
 * waves per workgroup, 4, 8, 12 or 16), "group_lanes" (0 auto | 16 | 32 | 64; with force_bits = 32 a forced
 * cols_per_wave x group_lanes whose int32 profile does not fit LDS is replaced by the library's pick, which
 * swg_stats reports),
 * "long_split" (-1 off | 0 auto | rows above which a pair joins the long class),
 * "autotune" (1 default: on the first search of a query length the few geometries the cost model
 * ranks best are timed on the device and the fastest is kept for that database | 0 model only),
 * "workgroups" (0 auto), "work_queue" (1 default: single-pass diagonal fills hand pairs to lane
 * groups through device-wide counters | 0 fixed streams laid out on the host), "long_helps"
 * (0 default | 1: lane groups of the long class go on with the bulk's pairs when their own are
 * done -- three wavefronts per SIMD issue as fast as four, so the less efficient helpers cost 1.5 %),
 * "prio_share" (percent of a lane group's mean share above which a bulk pair runs at raised
 * priority; default 150), "wide16" (1 default: when the query is long enough for a score to pass
 * 32767 the diagonal engine runs its wide form, exact to 65535, and only scores beyond that are
 * re-scored in int32 | 0: plain int16 and int32 re-score from 32767), "f16" (1 default: the diagonal engine's
 * 16-bit fill runs on packed-f16 cells -- gfx950's three-operand maxima, 8.5 instead of 10 instructions per
 * column pair, exact below 4096, every pair with a sequence that reaches 4096 flagged and run again on int16 cells
 * (two levels: f16 -> int16 / wide -> int32 for what saturates those) -- unless the
 * query is long enough for scores beyond 32767 (then the sequences too short to get there still do and the rest
 * runs on the wide form: swg_stats.cell_form 4) or the flagged pairs of this database held more than 1/16 of its
 * pair rows for this query | 0: int16 cells only | 2: f16 cells whenever the gap magnitudes are at most 2048), "last_pass" (1 default: the
 * last pass of a query of several passes runs with the fewest columns per lane that cover what is left | 0: like the
 * other passes), "qq" (1 default: a batch of
 * queries on the f16 cells runs two queries per lane | 0: two sequences per lane as a single query does), "side_readout" (1 default:
 * top-K selection and read-out of a search run on their own stream, beside the fill of the search
 * queued next), "batch" (8 default: pairs one work-queue request claims where pairs are short -- at most
 * "batch_blocks" 4-row token blocks long (0 default: about 40 us of work at the launch's geometry: 30 blocks at 2
 * columns per lane, 5 at 32); batch 0 / 1: every request claims one pair), "batch_geometry" (0 default: a batch of
 * queries -- swg_search_multi*, swg_search_lists* -- with cols_per_wave or group_lanes set is searched one query after
 * another, each at that geometry | 1: the batch itself takes the two, as one class and in one pass, where every other
 * rule of its planner allows -- the tests' way to every batch instantiation; max_waves and workgroups still send it one
 * by one), "above_batch" (0 default: swg_search_above_multi* chooses between its two routes | 1: the one launch per
 * class wherever the batch is admitted to it | 2: always one query after another; anything else is SWG_ERR_ARG -- see
 * swg_search_above_multi). */
int swg_set_option(swg_ctx *ctx, const char *key, long value);

/* Replaces scoring_t for the path (reference src/alignment_scoring.h:21-37):
 * sub[a][b] = score of query residue index a against database residue index b
 * (row = query: src/alignment.c:33,41); gap of length n costs
 * gap_open + n*gap_extend (src/alignment_scoring.c:35-36). */
int swg_set_scoring(swg_ctx *ctx, const int8_t sub[32][32], int gap_open, int gap_extend);

/* Replaces the query half of aligner_create (src/alignment.h:64-68):
 * idx[lq] are table indices; the library copies them. */
int swg_set_query(swg_ctx *ctx, const int8_t *idx, size_t lq);

/* A position-specific query (a PSSM: PSI-BLAST, an HMM-derived profile, ...): pssm[i*32 + b] = score of query
 * position i against database residue index b (same coordinates as sub[a][b]; column 0, the padding residue, is
 * ignored).  Replaces the context's query (an index query set by swg_set_query, or an earlier PSSM); swg_set_query
 * replaces a PSSM in turn.  Gap scores still come from swg_set_scoring, which must have been called before a
 * search; the substitution table is not read while a PSSM is the query.  Any int8 value is accepted.  The library
 * copies the lq*32 bytes; like swg_set_query the copy is queued behind the searches in flight (no wait), so PSSMs
 * and index queries can be streamed between swg_search_begin calls.  Every query-dependent call follows the PSSM:
 * swg_search, swg_search_begin/end, swg_fill_batches16, swg_align_hits, swg_align_ops_bound (swg_search_multi
 * takes index queries of its own and leaves the PSSM in place; swg_search_multi_pssm runs a batch of PSSMs in one
 * pass the same way).  A PSSM search has the plan an index query of the
 * same scores would have, so the same fill kernels at the same speed; its score bound (which decides the cells
 * and the re-score) is the sum of each position's best entry over residues 1..31. */
int swg_set_query_pssm(swg_ctx *ctx, const int8_t *pssm, size_t lq);

/* ---- database --------------------------------------------------------- */

/* Host-only (needs no GPU).  Replaces the 16-lane transpose+pad packer of
 * reference src/alignment_cmdline.c:429-452: sequences are sorted by length
 * (descending, stable; the reference requires a pre-sorted input,
 * src/alignment_cmdline.c:431-439) and stored as one byte per residue by sorted
 * rank; 128 consecutive ranks form a bin, the unit of sharding.  That image is
 * what swg_db_upload copies to the GPU; the kernels' own layouts are built from
 * it on the device.
 * flat[offsets[i] .. offsets[i+1]) are the indices of sequence i.
 * shard_count > 1 keeps only bins b with b % shard_count == shard_rank of the
 * GLOBAL bin sequence (round-robin over GPUs: adjacent bins have near-equal
 * work); indices reported later are always original ones. */
int swg_db_pack(const int8_t *flat, const uint64_t *offsets, size_t n,
                int shard_rank, int shard_count, swg_db **out);
/* The same for a shard that was cut elsewhere (a rank that generated or read only
 * its own bins of a large database): the n_local sequences given are exactly the
 * shard, global_index[i] is sequence i's index in the whole database of n_total
 * sequences.  When they are the bins b % count == rank of the whole database's
 * sorted order, in that order, the result equals swg_db_pack(whole, rank, count). */
int swg_db_pack_shard(const int8_t *flat, const uint64_t *offsets, size_t n_local,
                      const uint32_t *global_index, size_t n_total, swg_db **out);
/* All shard_count shards of one database at once: out[r] == swg_db_pack(flat, offsets, n, r, shard_count), from ONE
 * global sort and with the shards built side by side (what swg_group_load uses: one process driving several GPUs
 * should not sort a 10M-sequence database once per device).  On error no shard is returned. */
int swg_db_pack_shards(const int8_t *flat, const uint64_t *offsets, size_t n, int shard_count, swg_db **out);
int swg_db_upload(swg_ctx *ctx, swg_db *db); /* H2D; db becomes resident on ctx's GPU */
/* A view of `parent` (resident on ctx's device): the sequences whose ORIGINAL indices are listed, as a database of
 * its own.  No residue byte is copied or uploaded: the view reads the parent's bytes where they lie, on the host and
 * on the device, and 4 bytes per selected sequence cross PCIe.  Every call that takes a swg_db takes a view, and
 * runs the kernels and plans it would run on a packed and uploaded database of the same sequences.
 *   indices    original indices, in any order; duplicates collapse.  An index >= swg_db_total_count(parent) is
 *              SWG_ERR_ARG.  An index of the whole database that this shard does not hold is ignored, so every rank
 *              of a sharded run passes the same global list.  n == 0, or nothing of the list in this shard: an empty
 *              view, whose searches return no hits and write no score.
 *   parent     must be resident on ctx's device (else SWG_ERR_STATE).  A view of a view is a view of the database
 *              the first one was taken of, holding what both select; it does not depend on the view it was made from.
 * Of a view, swg_db_count is the number of sequences selected in this shard, swg_db_total_count the parent's
 * (scores_out stays indexed by original index and only selected entries are written; hits carry original indices),
 * swg_db_residues the selection's, swg_db_order the view's own order (the parent's sorted order, kept) and
 * swg_db_packed_bytes what the view itself sends to the GPU.  A view is resident from creation: swg_db_upload of a
 * view is SWG_ERR_STATE, swg_db_save of one SWG_ERR_ARG.  Plans, tuned geometries, hints, device layouts and output
 * buffers are the view's own: nothing a view learns changes its parent's searches, or the reverse.
 * Lifetime: the residue bytes live as long as the parent's handle or any view of it.  swg_db_free(parent) while
 * views live only ends the caller's use of the parent (its own search buffers are released); the bytes go with the
 * last view, whichever order the frees come in.  swg_db_upload(ctx, parent) while views live is SWG_ERR_STATE. */
int swg_db_view(swg_ctx *ctx, swg_db *parent, const uint32_t *indices, size_t n, swg_db **out);
/* Packed-database file (host-only): the sorted, re-coded image of swg_db_pack,
 * so a large database is ingested once; swg_db_load validates the structure it reads. */
int swg_db_save(const swg_db *db, const char *path);
int swg_db_load(const char *path, swg_db **out);
void swg_db_free(swg_db *db);
size_t swg_db_count(const swg_db *db);          /* sequences in this shard */
size_t swg_db_total_count(const swg_db *db);    /* sequences given to swg_db_pack */
uint64_t swg_db_residues(const swg_db *db);     /* sum of lengths in this shard */
uint64_t swg_db_packed_bytes(const swg_db *db); /* bytes swg_db_upload copies to the GPU */
/* original index of the i-th sequence of this shard in its sorted order */
const uint32_t *swg_db_order(const swg_db *db);

/* ---- the hot path ----------------------------------------------------- */

/* Replaces the whole timed region of the reference
 * (src/alignment_cmdline.c:503-509) plus the read-out of aligner->max_scores
 * (src/tools/sw_cmdline.c:55-72) for every sequence of `db`:
 *   scores_out  NULL, or an array of swg_db_total_count(db) int32 indexed by
 *               ORIGINAL database index; only this shard's entries are written.
 *   topk_out/k  NULL/0, or room for k hits of this shard (fewer are written
 *               when the shard is smaller; *n_hits tells how many).
 * Scores are exact int32 local-alignment maxima: the 16-bit kernels flag every
 * sequence whose score reaches their ceiling and those are run again on wider cells
 * (f16 -> int16 or its wide form -> int32). */
int swg_search(swg_ctx *ctx, const swg_db *db, int32_t *scores_out,
               swg_hit *topk_out, size_t k, size_t *n_hits, swg_stats *stats);

/* The same search in two halves, so that a caller can keep the GPU busy: swg_search_begin queues
 * everything on the context's stream and returns; swg_search_end waits for that search and
 * delivers its results.  Up to 4 searches may be in flight per context (each has its own output
 * buffers; they execute in order).  want_scores != 0 is required to get scores_out at the end.
 * swg_search(...) == begin + end.  The database must stay alive and resident in between. */
int swg_search_begin(swg_ctx *ctx, const swg_db *db, int want_scores, size_t k, int *ticket);
int swg_search_end(swg_ctx *ctx, int ticket, int32_t *scores_out, swg_hit *topk_out, size_t *n_hits,
                   swg_stats *stats);

/* Hits-only pruning.  A search that returns hits and no score array (k > 0, want_scores == 0) need not fill a pair of
 * sequences that cannot be among the k best: with non-positive gap scores a sequence scores at most the sum, over its
 * residues, of each residue's best score against any query column, and once k sequences are known to score T or more a
 * sequence whose sum is below T is out whatever the ties.  The 16-bit fill of the lane groups' work queue then runs in
 * stages and skips, from the second stage on, the pairs behind the last one whose bound reaches the
 * k-th best score so far.  Hits are exactly those of the unpruned search.  swg_stats is unchanged by it (cells stays the
 * nominal lq x residues); swg_prune_last tells what the search LAST ENDED on the context left out:
 *   pruned             1: the search ran in stages; 0: it did not (the rest is then 0 except pair_rows)
 *   threshold          the last T the stages used (scores of 4095 and more count as 4095)
 *   pairs_skipped      pairs of sequences no launch filled
 *   pair_rows_skipped  their rows, in whole 4-row token blocks (two reset rows + the longer sequence of the pair)
 *   pair_rows          the rows of all pairs of the fill, in the same unit
 * Options (swg_set_option): "prune" 0 off | 1 (default) auto: hits-only searches on the 16-bit lane-group work queue with
 * non-positive gap scores, one class and one cell form, whose range spans several launch segments (a database of some
 * millions of sequences) and has at least 4 x prune_head pairs per resident lane group; never a gapless search, a query of swg_search_multi* or swg_search_lists* (swg_search_above_multi* searched one query after another is pruned per query, as swg_search_above is) or anything on other engines |
 * 2 DIAGNOSTIC, for tests: prune wherever it is structurally possible, ignoring the size rule, and also when scores are
 * requested -- the sequences of skipped pairs then report a score of 0, which is NOT their score.  "prune_head" (default 4):
 * under "prune" 2 a range of one segment runs its longest pairs first, unpruned -- at least k sequences and prune_head pairs per lane
 * group -- so that the rest has a threshold to be cut by.  "prune_kmer" (default 0): the bound a pruned search cuts by.
 * 1: the sum of the residues' best scores, above.  4 | 5: the sum, over consecutive blocks of 4 | 5 rows of the
 * sequence, of each block's own local score against the whole query -- never above the first, never below the
 * sequence's score -- read from a table of every block of residue classes, which is built on the
 * device in front of the first pruned search of a (query, scoring): 22^4 x 4 x lq cell updates at k = 4, 22^4 x 26 x lq
 * at k = 5 (the 22 blocks behind four classes share those four rows), 4 ms at k = 5 for 3000 columns on an MI355X, paid
 * once per query.  0: automatic, the largest k whose table costs at most half of what
 * its tighter cut is expected to save on this range (small databases: 1).  "prune_segments" (default 0): the k-mer
 * bound's table holds, per block, its best cell within each of 1..32 consecutive segments of the query's columns, and
 * a sequence's blocks are taken in order -- a later block cannot score in an earlier segment; 1 is the
 * unordered sum above, a larger value is never above it; the table is 22^k x segments x 2 bytes, refused above 96 MB
 * (k = 5: up to 9 segments).  0: automatic -- with "prune_kmer" 0 the pair (k, segments) is chosen together from a
 * fixed list (a database of millions of sequences: k = 4 in 32 segments), with "prune_kmer" forced the sum is
 * unordered.  "prune_cut" (default 0): 0 a stage takes exactly its pairs whose bound reaches the threshold, in order;
 * 1 the prefix of the length order up to the last such pair.  "prune_refine" (default 0): under "prune_cut" 0 the pairs of
 * a stage whose bound still reaches the threshold are bounded once more over a k = 4 table of 64 | 128 segments, and the
 * lesser bound holds; 1 off; 0 automatic -- on where "prune_kmer" and "prune_segments" are both automatic and took k = 4
 * in segments, off otherwise.  "prune_refine3" (default 0): the pairs that still reach the threshold after that are
 * bounded a third time over a k = 4 table of 256 segments, and the least bound holds; 256 on, behind whatever the second
 * level is; 1 off; 0 automatic -- on where the second level was chosen automatically and took 128, the tables hold
 * bytes (below) and the range is large enough for the finer cut to pay for its table and its walk twice over (the
 * 10M-sequence database: yes; a database of thousands or a few million sequences: no).  "prune_refine4" (default 0):
 * the pairs that still reach the threshold after the third level are bounded a fourth time over a table of 5-residue
 * blocks in 256 segments (22^5 x 256 bytes = 1.32 GB of device memory, built in about 5 ms per query of 3000 columns), and
 * the least bound holds; 5256 on, behind whatever the other levels are; 1 off; 0 automatic -- on where the third level
 * was chosen automatically and the range is large enough (the 10M-sequence database: yes; smaller ones: no).  The table
 * holds bytes only: a query whose blocks of 5 can score above 255 (a PSSM entry of 52 or more) is searched without the
 * level under every value, and so is every search of a context whose device had no room for the table -- neither is an
 * error.  "prune_refine5" (default 0): the pairs that still reach the threshold after the fourth level are bounded a fifth
 * time by the fourth level's walk with the query columns jumped over between two blocks charged as a gap, over a second
 * table of 5-residue blocks in 256 segments (another 1.32 GB, about 3.3 ms per query of 3000 columns), and the least
 * bound holds; 5256 on, behind whatever the other levels are; 1 off; 0 automatic -- on where the fourth level was chosen
 * automatically, the range is large enough and the threshold is the K-th best score (under swg_search_above's threshold
 * the level runs only where it is forced).  It needs gap_extend < 0 and entries that are bytes (5 x (the largest
 * substitution score - gap_extend) <= 255); a search that has neither, or a context whose device had no room for the
 * table, runs without the level under every value -- not an error.  "prune_gate" (default 0): where the first-level bound is a k-mer bound in segments, its kernel can wait for a
 * threshold -- the K-th best score behind the first stage, or swg_search_above's -- and leave out every pair whose
 * colmax bound is already below it (no other bound of the pair can be above that one, so no hit and no count changes);
 * the pairs of the first stage, which is never cut, are then not bounded at all.  2 on wherever the first level is
 * segmented; 1 off; 0 automatic -- on where "prune_kmer" and "prune_segments" are both automatic and the range is large
 * enough for the third level (the 10M-sequence database: yes; smaller ones: no).  "prune_table_bits" (default 0):
 * the width of the k-mer tables' entries.  0: bytes wherever k x the largest score of the query's profile is at most 255
 * (every entry fits: BLOSUM62 44, PAM250 68 at k = 4), uint16_t otherwise (a PSSM with an entry of 64 or more); 16:
 * uint16_t always.  A byte table holds the same values in half the memory and gather traffic.  Hits, bounds and lists are
 * the same under every value of these options. */
typedef struct swg_prune_info {
    uint64_t pairs_skipped;
    uint64_t pair_rows_skipped;
    uint64_t pair_rows;
    uint32_t threshold;
    int32_t pruned;
} swg_prune_info;
int swg_prune_last(const swg_ctx *ctx, swg_prune_info *out);

/* Many queries against one resident database in ONE pass of the hot path.  The reference takes a
 * single query per run (src/alignment_cmdline.c:381-396); its report says the design "extends
 * naturally" to many-to-many (Final Report p.7).  Query i is queries[q_offsets[i] .. q_offsets[i+1])
 * (table indices, as swg_set_query takes them); the scoring system is the context's, the context's own
 * query is left as it was.  All queries of a batch share one launch per class: a database too small to
 * fill the GPU with one query fills it with many.  Batches that cannot take that path (a query of
 * several passes, scores that may pass 32767, gap scores outside the packed int16 form, engine
 * options) are searched one query after another: same results.
 *   scores_out  NULL, or n_queries rows of swg_db_total_count(db) int32 by ORIGINAL database index;
 *   topk_out/k  NULL/0, or n_queries rows of k hits; n_hits NULL or n_queries counts;
 *   stats       NULL, or ONE record for the whole batch (times and cells summed). */
int swg_search_multi(swg_ctx *ctx, const swg_db *db, const int8_t *queries, const uint64_t *q_offsets,
                     size_t n_queries, int32_t *scores_out, swg_hit *topk_out, size_t k, size_t *n_hits,
                     swg_stats *stats);

/* Many position-specific queries against one resident database in ONE pass: swg_search_multi with PSSMs.
 * PSSM i is pssms[(q_offsets[i] + p)*32 + b] for p < q_offsets[i+1] - q_offsets[i] (offsets count POSITIONS,
 * not bytes; column 0 ignored; any int8 accepted).  Gap scores are the context's; the context's own query
 * (index or PSSM) is left as it was.  Outputs, batching, fall-backs and stats as swg_search_multi. */
int swg_search_multi_pssm(swg_ctx *ctx, const swg_db *db, const int8_t *pssms, const uint64_t *q_offsets,
                          size_t n_queries, int32_t *scores_out, swg_hit *topk_out, size_t k, size_t *n_hits,
                          swg_stats *stats);

/* The gapless prefilter score: the best-scoring UNGAPPED diagonal segment of query x sequence,
 *     H[i][j] = max(0, H[i-1][j-1] + S(q_i, d_j)),  score = max over all cells,
 * for the context's query (index or PSSM, whichever was set last) against every sequence of a resident database: what
 * MMseqs2-style pipelines rank the database by before they spend the affine-gap fill on the best candidates
 * (swg_search_lists takes its top-N).  Outputs, hit order (higher score first, ties by lower original index), shards
 * and views exactly as swg_search; scores are exact int32 for every input.
 * The gap scores of swg_set_scoring are NOT read -- the result is the same whatever they are -- but scoring must have
 * been set: the table is needed, and a PSSM query needs the usual call order.
 * Where the query fits one pass of a lane-group geometry (at most 2048 columns; a forced cols_per_wave / group_lanes must
 * still cover it), the database was not built from 16-lane batches and the options do not rule it out (f16 = 0,
 * engine = 1, work_queue = 0), the fill runs the gapless cells: 3.5 packed instructions per column pair instead of
 * 8.5, swg_stats.cell_form 6, path_bits 16, engine 2, work_queue 1, passes 1, n_rescored = the sequences that reached
 * 4096 and were run again.  Everything else runs the gapped machinery with the gaps priced out (never cell_form 6):
 * same scores.  autotune, max_waves, workgroups, batch and batch_blocks act as for swg_search; tuned geometries are
 * kept apart from the gapped searches'.  Searches in flight on the context: SWG_ERR_STATE. */
int swg_search_gapless(swg_ctx *ctx, const swg_db *db, int32_t *scores_out, swg_hit *topk_out, size_t k, size_t *n_hits,
                       swg_stats *stats);
/* A batch of queries, by definition the loop "set query i, swg_search_gapless" (queries, offsets, outputs and the one
 * summed stats record as swg_search_multi / swg_search_multi_pssm take and give them).  The context's own query is left
 * as it was. */
int swg_search_gapless_multi(swg_ctx *ctx, const swg_db *db, const int8_t *queries, const uint64_t *q_offsets, size_t n_queries,
                             int32_t *scores_out, swg_hit *topk_out, size_t k, size_t *n_hits, swg_stats *stats);
int swg_search_gapless_multi_pssm(swg_ctx *ctx, const swg_db *db, const int8_t *pssms, const uint64_t *q_offsets, size_t n_queries,
                                  int32_t *scores_out, swg_hit *topk_out, size_t k, size_t *n_hits, swg_stats *stats);

/* Every hit at or above a score: the question a pipeline asks once an E-value cut-off has been turned into a raw score
 * (swg_calibrate + swg_evalue_min_score do that).  For the context's query (index or PSSM) against a resident database,
 * view or shard, exactly as swg_search takes them:
 *   *n_total   the sequences of this shard or view whose exact int32 score is >= min_score;
 *   hits_out   the best min(cap, *n_total) of them in the library's total order (higher score first, ties by lower
 *              original index); *n_hits says how many were written.  With *n_total > cap the call still succeeds: the
 *              caller sees it and can call again with more room.  cap = 0 with hits_out NULL is a pure count.
 * Scores are exact for every input (the f16 -> int16 / wide -> int32 re-runs happen as in swg_search).  Shards: each
 * rank's call gives its shard's hits, and the union sorted by swg_hit_key is the whole database's answer.
 * min_score < 1 is SWG_ERR_ARG (every sequence scores at least 0); cap > 0 with hits_out NULL is SWG_ERR_ARG; the other
 * errors are swg_search's, and searches in flight on the context give SWG_ERR_STATE (there is no begin / end form).
 * Pruning (option "prune"; the rest of the prune_* options choose the bound as above, "prune_cut" is not read): the
 * threshold of a pruned search is min_score from its first launch on, so every stage -- the first included, and the
 * only one of a range of one segment -- fills exactly the pairs whose score bound reaches it; a pair left out scores
 * below min_score.  0 never | 2 wherever it is structurally possible (non-positive gap scores, the 16-bit lane-group work
 * queue, one class, one cell form) | 1 (default) those of them whose range has at least 16 pairs per resident lane group
 * ("A caller's threshold").  Everything else -- positive gap scores, the int32 path, the systolic
 * engine, two classes, both cell forms -- runs its usual fill; only the read-out differs.  swg_prune_last reports this
 * search too: threshold = min_score, and pairs_skipped is exactly the number of pairs of the fill whose final bound is
 * below it.  stats as swg_search (topk_ms: the read-out's kernel and the host's sort). */
int swg_search_above(swg_ctx *ctx, const swg_db *db, int32_t min_score, swg_hit *hits_out, size_t cap, size_t *n_hits,
                     uint64_t *n_total, swg_stats *stats);
/* The same question of the gapless prefilter score (swg_search_gapless): never pruned, errors and outputs as above. */
int swg_search_gapless_above(swg_ctx *ctx, const swg_db *db, int32_t min_score, swg_hit *hits_out, size_t cap, size_t *n_hits,
                             uint64_t *n_total, swg_stats *stats);

/* Every hit at or above a score, for a BATCH of queries with a score each: what a pipeline with a thousand queries and an
 * E-value cut-off asks (the cut-off turns into a raw score per query: swg_calibrate_multi + swg_evalue_min_score).  Queries
 * and offsets as swg_search_multi takes them.  By definition row i is what swg_set_query(query i) +
 * swg_search_above(ctx, db, min_scores[i], hits_out + i*cap, cap, &n_hits[i], &n_total[i], ..) gives:
 *   n_total[i]       the sequences of this shard or view whose exact int32 score is >= min_scores[i];
 *   hits_out + i*cap the best min(cap, n_total[i]) of them in the library's order (higher score first, ties by lower
 *                    original index); n_hits[i] says how many were written, slots of a row past it are not written.
 *                    cap is the same room for every query; cap = 0 with hits_out NULL is a pure count;
 *   n_hits, n_total  each NULL or an array of n_queries; both are zeroed before anything can fail;
 *   stats            NULL, or ONE summed record, as swg_search_multi gives it.
 * The rows go into swg_align_hits_multi / swg_align_bounds_multi / swg_align_stats_multi unchanged, with k = cap.  The
 * context's own query (index, PSSM or none) is left as it was.  n_queries = 0 is SWG_OK with nothing written.
 * Errors: min_scores NULL or min_scores[i] < 1 is SWG_ERR_ARG (the message names the query); cap > 0 with hits_out NULL
 * is SWG_ERR_ARG; everything else as swg_search_multi (an empty query, a residue outside 1..31, a database that is not
 * resident, searches in flight: SWG_ERR_STATE).
 * Two routes, option "above_batch" (swg_set_option): 1 the one launch per class of swg_search_multi for chunks of up to
 * 256 queries, wherever that call would take it; its fill is NOT pruned, and each score row is compacted on the device
 * against its own threshold, so that only counts and keys cross PCIe (swg_stats: fill_launches = the chunks, cell_form
 * 3, 2 or 0) | 2 one query after another, each a plain swg_search_above whose fill is cut at its own min_scores[i]
 * wherever a single swg_search_above would be (option "prune"; swg_stats sums the searches, fill_launches 0) | 0
 * (default) automatic: the launch where the batch is admitted to it and swg_search_above of the batch's longest query
 * on this database would not be pruned, one by one otherwise.  Answers are the same on both routes.
 * swg_prune_last after the call: pruned = 1 if any query's search was pruned; pairs_skipped, pair_rows_skipped and
 * pair_rows summed over the batch's queries (the one launch: 0, 0, 0 and pruned 0); threshold = the last query's
 * min_score.  topk_ms is the read-out's kernels plus the host's sort. */
int swg_search_above_multi(swg_ctx *ctx, const swg_db *db, const int8_t *queries, const uint64_t *q_offsets, size_t n_queries,
                           const int32_t *min_scores, swg_hit *hits_out, size_t cap, size_t *n_hits, uint64_t *n_total, swg_stats *stats);
/* The same with position-specific queries: pssms and offsets (which count POSITIONS) as swg_search_multi_pssm takes them. */
int swg_search_above_multi_pssm(swg_ctx *ctx, const swg_db *db, const int8_t *pssms, const uint64_t *q_offsets, size_t n_queries,
                                const int32_t *min_scores, swg_hit *hits_out, size_t cap, size_t *n_hits, uint64_t *n_total, swg_stats *stats);
/* The same question of the gapless prefilter score, row i as swg_search_gapless_above gives it: always one query after
 * another (the batch launch has no gapless cells) and never pruned. */
int swg_search_gapless_above_multi(swg_ctx *ctx, const swg_db *db, const int8_t *queries, const uint64_t *q_offsets, size_t n_queries,
                                   const int32_t *min_scores, swg_hit *hits_out, size_t cap, size_t *n_hits, uint64_t *n_total,
                                   swg_stats *stats);
int swg_search_gapless_above_multi_pssm(swg_ctx *ctx, const swg_db *db, const int8_t *pssms, const uint64_t *q_offsets, size_t n_queries,
                                        const int32_t *min_scores, swg_hit *hits_out, size_t cap, size_t *n_hits, uint64_t *n_total,
                                        swg_stats *stats);

/* ---- E-values and bit scores: a query calibrated on the device ---------- */

/* The residue counts of a resident database, shard or view: counts[r] = how many residues of index r it holds
 * (counts[0], the padding residue, is 0; the sum is swg_db_residues(db); the shards of a database add up).  One kernel
 * over the resident bytes -- a view walks its own slots over its parent's bytes --, so that a caller can calibrate
 * against the composition of what it searches (freq[r] = counts[r]).  A database that is not resident on ctx's device,
 * or one built from 16-lane batches (swg_fill_batches16: it has no residue bytes), is SWG_ERR_STATE. */
int swg_db_composition(swg_ctx *ctx, const swg_db *db, uint64_t counts[32]);

/* What a calibration leaves per query: the Gumbel fit of the query's scores against random sequences, and the
 * Karlin-Altschul pair (lambda, K) read off it.  The score S of the query against n_seqs random sequences of seq_len
 * residues each follows P(S >= x) = 1 - exp(-exp(-lambda (x - mu))); with K = exp(lambda mu) / (lq seq_len) the expected
 * number of sequences of a database of N residues in all that score S or more by chance is
 *     E = K lq N exp(-lambda S)
 * (no edge correction: the fit is made at a finite length and carries the effect that the correction estimates --
 * DESIGN 8.4).  status: 0 a fit; 1 no fit, fewer than two distinct scores (lambda, K and mu are 0); 2 Newton's iteration
 * did not converge in 100 steps (lambda and mu are where it stopped). */
typedef struct swg_evalue_params {
    double lambda, K, mu;
    uint32_t lq, n_seqs, seq_len;
    int32_t status;
} swg_evalue_params;

/* Pure helpers (host only, no context).  With status != 0 (or p NULL) they return NaN, NaN and -1.
 *   swg_evalue            K lq db_residues exp(-lambda score)
 *   swg_bitscore          (lambda score - ln K) / ln 2, so that E = lq db_residues 2^-bits
 *   swg_evalue_min_score  the smallest S >= 1 with swg_evalue(p, db_residues, S) <= E, checked against its neighbour
 *                         S - 1; -1 where there is none in int32 (E <= 0 or not a number) */
double swg_evalue(const swg_evalue_params *p, uint64_t db_residues, int32_t score);
double swg_bitscore(const swg_evalue_params *p, int32_t score);
int32_t swg_evalue_min_score(const swg_evalue_params *p, uint64_t db_residues, double E);

/* Calibration by simulation (what HMMER and SSEARCH do): the query is scored against "calib_seqs" random sequences of
 * "calib_len" residues each, i.i.d. from a background composition (swg_synth_db_iid with seed "calib_seed"), the scores
 * stay on the device, one workgroup per query histograms its row and fits a Gumbel distribution to it by maximum
 * likelihood (swg_gumbel_fit_hist is the same fit on the host), and 32 bytes per query come back.  Works for whatever
 * the library scores: any table and gap scores, a PSSM, the gapless score (gapless != 0: swg_search_gapless's score).
 *   freq     NULL: the built-in Swiss-Prot-like table; else 32 weights by residue index as swg_synth_db_iid takes them
 *            (swg_db_composition's counts, as doubles, calibrate against a database's own composition)
 *   out      swg_calibrate: one record, for the context's query (index or PSSM; none set: SWG_ERR_STATE);
 *            the batch calls: n_queries records, queries / pssms and offsets as swg_search_multi / swg_search_multi_pssm
 *            take them; the context's own query is left as it was; n_queries = 0 is SWG_OK.
 * The scores come from the planner's usual routes: one launch per chunk of up to 256 queries where swg_search_multi
 * would take it, one query after another otherwise (several passes, gapless, a batch of one); every re-run of flagged
 * sequences happens as in a search, so the histogram is of exact scores (those of 4095 and more count as 4095).  A query
 * whose fit has status != 0 does not fail the call.  The random database is generated, packed and uploaded on first use
 * and kept on the context, for the last (freq, calib_seqs, calib_len, calib_seed) asked for, until swg_destroy.
 * Options (swg_set_option): "calib_seqs" (default 8192; 2 .. 1048576), "calib_len" (default 384; 8 .. 16384),
 * "calib_seed" (default 1; >= 0); anything outside is SWG_ERR_ARG.  8192 samples give lambda a standard error of
 * 0.78 lambda / sqrt(n), about 0.9 %.  Errors: NULL arguments, a malformed freq: SWG_ERR_ARG; no scoring set, searches in
 * flight on the context: SWG_ERR_STATE.  A sharded caller calibrates on one context and sums swg_db_residues. */
int swg_calibrate(swg_ctx *ctx, const double *freq, int gapless, swg_evalue_params *out);
int swg_calibrate_multi(swg_ctx *ctx, const int8_t *queries, const uint64_t *q_offsets, size_t n_queries, const double *freq,
                        int gapless, swg_evalue_params *out);
int swg_calibrate_multi_pssm(swg_ctx *ctx, const int8_t *pssms, const uint64_t *q_offsets, size_t n_queries, const double *freq,
                             int gapless, swg_evalue_params *out);

/* Every query of a batch against ITS OWN candidate list in one pass: what a prefilter, a PSI-BLAST iteration or a list
 * of family members per query hands to the alignment step.  Query i is queries[q_offsets[i] .. q_offsets[i+1]) as
 * swg_search_multi takes it; its candidates are cand[c_offsets[i] .. c_offsets[i+1]): ORIGINAL database indices, in any
 * order, duplicates allowed, the list possibly empty.  The result for query i is by definition what
 * swg_db_view(ctx, db, list i) + swg_set_query(query i) + swg_search(view) reports: exact int32 scores, hits ordered
 * by higher score first, ties by lower index.  All lists of a chunk of 256 queries run in ONE launch over a table of
 * (query, sequence) jobs; device memory and PCIe traffic grow with the total length of the lists, never with
 * n_queries x database.  Batches that cannot take that launch (a query of several passes, scores that may pass 32767,
 * gap scores outside the packed int16 form, engine or geometry options) go one list after another through a view: same
 * results, swg_stats.fill_launches 0.
 *   cand        an index >= swg_db_total_count(db) is SWG_ERR_ARG (the message names the query and the entry).  An
 *               index this shard does not hold is ignored, and so is one that db, itself a view, does not select:
 *               every rank of a sharded run passes the same lists.
 *   db          resident (else SWG_ERR_STATE); one built from 16-lane batches is SWG_ERR_STATE as for swg_db_view.
 *               Searches in flight on the context: SWG_ERR_STATE, as for swg_search_multi.
 *   scores_out  NULL, or c_offsets[n_queries] int32 PARALLEL TO cand: scores_out[c_offsets[i] + j] is query i against
 *               cand[c_offsets[i] + j]; duplicates each get the score, an ignored entry is not written.
 *   topk_out/k  NULL/0, or n_queries rows of k hits with ORIGINAL indices (swg_align_hits_multi takes them against db
 *               unchanged); n_hits NULL or n_queries counts, each at most the distinct candidates of its list held
 *               here, 0 for an empty list.
 *   stats       NULL, or ONE record for the batch: cells = sum over i of lq_i x the residues of list i's distinct
 *               held candidates; the one launch reports engine 2, work_queue 1, path_bits 16, cell_form 0 or 2,
 *               passes 1 and fill_launches = the chunks launched.
 * The context's own query (index or PSSM) is left as it was. */
int swg_search_lists(swg_ctx *ctx, const swg_db *db, const int8_t *queries, const uint64_t *q_offsets, size_t n_queries,
                     const uint32_t *cand, const uint64_t *c_offsets, int32_t *scores_out, swg_hit *topk_out, size_t k,
                     size_t *n_hits, swg_stats *stats);
/* The same with position-specific queries: PSSM i is pssms[(q_offsets[i] + p)*32 + b], as swg_search_multi_pssm takes it. */
int swg_search_lists_pssm(swg_ctx *ctx, const swg_db *db, const int8_t *pssms, const uint64_t *q_offsets, size_t n_queries,
                          const uint32_t *cand, const uint64_t *c_offsets, int32_t *scores_out, swg_hit *topk_out, size_t k,
                          size_t *n_hits, swg_stats *stats);

/* Reference-shaped replay of the call site itself: n_batches 16-lane batches
 * exactly as `alignment_fill_matrices` receives them -- db_idx_t is
 * aligner_t.seq_b_batch_indexes, [max_len][16] int8 (src/alignment.h:28,
 * src/alignment_cmdline.c:434,445), padded rows included and computed as real
 * rows like the reference does; max_scores receives
 * aligner_t.max_scores for lanes 0..vector_size-1, saturated to int16.
 * Uses the scoring and query already set on ctx (a PSSM query included; its scores saturate the same way).
 * Lanes at or beyond vector_size are never read and their max_scores never written.  A residue index outside
 * 1..31 in a live lane is SWG_ERR_RESIDUE; searches in flight on the context (swg_search_begin) are SWG_ERR_STATE. */
typedef struct swg_batch16 {
    const int8_t *db_idx_t;
    size_t max_len;
    size_t vector_size;
    int16_t *max_scores;
} swg_batch16;
int swg_fill_batches16(swg_ctx *ctx, const swg_batch16 *batches, size_t n_batches,
                       double *fill_seconds);

/* ---- alignments of reported hits -------------------------------------- */

/* The reference reports scores only (its fork removed upstream's traceback: Final Report p.7; the
 * comment at src/alignment.c:46 is what is left of it).  swg_align_hits re-runs the given pairs on
 * the GPU with the recurrence of src/alignment.c:124-161 kept whole and walks back from the best
 * match cell.  Coordinates are 0-based and half-open.  ops spells the path first to last:
 * 'M' query residue against database residue, 'I' database residue against a gap (state A of the
 * recurrence), 'D' query residue against a gap (state B); the path's substitution and gap scores
 * (a gap position costs gap_extend when it continues a gap of the same kind, else
 * gap_open + gap_extend) add up to `score`.  Ties, which the reference never had to define: the
 * best cell is the one with the highest score, then the smallest database position, then the
 * smallest query position; a state whose maximum is 0 starts the alignment; otherwise the first
 * maximal predecessor in the order H, A, B. */
typedef struct swg_alignment {
    int32_t score;  /* recomputed here; equals the search's score for the pair */
    uint32_t index; /* ORIGINAL database index, copied from the hit */
    uint32_t q_begin, q_end; /* aligned part of the query */
    uint32_t d_begin, d_end; /* aligned part of the database sequence */
    uint32_t n_ops;          /* steps of the path (0 when the score is 0) */
    uint32_t reserved;
} swg_alignment;

/* hits[n_hits]: only .index is read (every sequence must belong to this shard).  out[n_hits].
 * ops: NULL, or n_hits strings of ops_stride bytes each, NUL-terminated;
 * swg_align_ops_bound(ctx, db) = query length + longest sequence + 1 is always enough. */
int swg_align_hits(swg_ctx *ctx, const swg_db *db, const swg_hit *hits, size_t n_hits,
                   swg_alignment *out, char *ops, size_t ops_stride);
size_t swg_align_ops_bound(const swg_ctx *ctx, const swg_db *db);

/* The alignments of a batch's hits in one call: query i is queries[q_offsets[i] .. q_offsets[i+1]) (table
 * indices, as swg_search_multi takes them), its hits are hits[i*k .. i*k + n_hits[i]) (n_hits[i] <= k; only .index
 * is read; any order, and a sequence may appear in several rows), i.e. swg_search_multi's topk_out / n_hits.
 * out[i*k + j] and, when ops is not NULL, the path at ops + (i*k + j)*ops_stride belong to hit j of query i; slots
 * past n_hits[i] are not written.  Every field and path equals swg_set_query(query i) + swg_align_hits.  Scoring
 * is the context's; the context's own query (index, PSSM or none) is neither read nor changed.  The database must
 * be resident.  swg_align_ops_bound_multi(db, q_offsets, n_queries) = longest query + longest sequence + 1 is
 * always enough for ops_stride (0 for NULL arguments; host only). */
int swg_align_hits_multi(swg_ctx *ctx, const swg_db *db, const int8_t *queries, const uint64_t *q_offsets,
                         size_t n_queries, const swg_hit *hits, size_t k, const size_t *n_hits,
                         swg_alignment *out, char *ops, size_t ops_stride);
/* The same with position-specific queries: PSSM i is pssms[(q_offsets[i] + p)*32 + b] as swg_search_multi_pssm
 * takes it; equals swg_set_query_pssm(PSSM i) + swg_align_hits. */
int swg_align_hits_multi_pssm(swg_ctx *ctx, const swg_db *db, const int8_t *pssms, const uint64_t *q_offsets,
                              size_t n_queries, const swg_hit *hits, size_t k, const size_t *n_hits,
                              swg_alignment *out, char *ops, size_t ops_stride);
size_t swg_align_ops_bound_multi(const swg_db *db, const uint64_t *q_offsets, size_t n_queries);

/* The coordinates without the path: swg_align_bounds / _multi / _multi_pssm write, for the same arguments, every field
 * (score, index, q_begin, q_end, d_begin, d_end, n_ops, reserved = 0) that swg_align_hits / _multi / _multi_pssm write
 * with ops == NULL -- same tie rules, same errors, hits in any order and repeated, slots past n_hits[i] not written --
 * but from a forward pass alone: every state of the recurrence carries the origin and the length of its path, so there
 * is no predecessor byte per cell and no walk.  One lane group takes a pair; the residues are read from the
 * resident database (a view is accepted), so the database must be resident for all three calls.  A pair the kernel
 * cannot hold (a query of more than 1024 columns, a sequence of 2^20 residues or more) goes through the traceback's
 * kernel in the same call, with the same results.  swg_align_bounds uses the context's query (index or PSSM); the
 * batch calls neither read nor change it.  For what is printed, swg_align_hits gives the path. */
int swg_align_bounds(swg_ctx *ctx, const swg_db *db, const swg_hit *hits, size_t n_hits, swg_alignment *out);
int swg_align_bounds_multi(swg_ctx *ctx, const swg_db *db, const int8_t *queries, const uint64_t *q_offsets,
                           size_t n_queries, const swg_hit *hits, size_t k, const size_t *n_hits, swg_alignment *out);
int swg_align_bounds_multi_pssm(swg_ctx *ctx, const swg_db *db, const int8_t *pssms, const uint64_t *q_offsets,
                                size_t n_queries, const swg_hit *hits, size_t k, const size_t *n_hits,
                                swg_alignment *out);

/* The line of a tabular report (BLAST -outfmt 6, MMseqs2 convertalis) without the path: swg_align_stats / _multi /
 * _multi_pssm take the arguments of swg_align_bounds / _multi / _multi_pssm, write to `out` exactly what those write
 * (same errors, hit order, repeats, views and fallback; reserved = 0) and to `counts`, parallel to `out` (slot i*k + j in
 * the batch calls; slots past n_hits[i] are not written), the column counts of the path swg_align_hits* would spell
 * for the same pair under the tie rules above.  counts, like out, must not be NULL when there is a hit (SWG_ERR_ARG).
 * A pair of score 0 has all four counts 0.  The forward pass carries n_ident and n_gap_open with every state's tag; the
 * other two follow from the coordinates (every M takes a query column and a residue, every I or D one of the two).
 * Percent identity as BLAST prints it is 100 * n_ident / n_ops, mismatches are n_match - n_ident.
 * A PSSM has no residues: identity is counted against its consensus, as MMseqs2 reports identity for profile queries --
 * position p's consensus is the lowest residue index b in 1..31 whose score pssm[p*32 + b] is the row's maximum over
 * 1..31.  DESIGN 8.3. */
typedef struct swg_align_counts {
    uint32_t n_ident;    /* 'M' steps whose query residue equals the database residue */
    uint32_t n_match;    /* 'M' steps (aligned columns); mismatches = n_match - n_ident */
    uint32_t n_gap_open; /* maximal runs of 'I' or of 'D' in the path ("ID" is two runs) */
    uint32_t n_gap;      /* 'I' + 'D' steps = n_ops - n_match */
} swg_align_counts;
int swg_align_stats(swg_ctx *ctx, const swg_db *db, const swg_hit *hits, size_t n_hits, swg_alignment *out,
                    swg_align_counts *counts);
int swg_align_stats_multi(swg_ctx *ctx, const swg_db *db, const int8_t *queries, const uint64_t *q_offsets,
                          size_t n_queries, const swg_hit *hits, size_t k, const size_t *n_hits, swg_alignment *out,
                          swg_align_counts *counts);
int swg_align_stats_multi_pssm(swg_ctx *ctx, const swg_db *db, const int8_t *pssms, const uint64_t *q_offsets,
                               size_t n_queries, const swg_hit *hits, size_t k, const size_t *n_hits,
                               swg_alignment *out, swg_align_counts *counts);

/* Several alignments per hit: every non-overlapping local alignment of a pair at or above a score, best first (the
 * HSPs of BLAST, the alignments upstream seq-align's smith_waterman prints one after another; Waterman and Eggert 1987).
 * Alignment 0 of a pair is what swg_align_hits gives: recurrence, tie rules, coordinates and path letters as above.
 * Alignment r >= 1 is the best alignment of the same recurrence with one change.  A cell (j, i) is USED when database
 * residue j was aligned to query column i by an 'M' step of alignments 0 .. r-1 of this pair, and the H state of a used
 * cell is minus infinity: a used cell is never the best cell, and no state of a neighbouring cell takes the used cell's
 * H as a predecessor.  The used cell's own A and B states (the gap states) are computed as before from its neighbours,
 * so a later alignment may cross an earlier one through a gap; it never shares an aligned residue pair with it.
 * Everything else is unchanged: the best cell is the highest H, then the smallest database position, then the smallest
 * query position; a state whose maximum is 0 starts the alignment; otherwise the first maximal predecessor in the
 * order H, A, B.  The rounds of a pair stop at the first alignment whose score is below min_score (>= 1), or after
 * max_hsps (1 .. SWG_MAX_HSPS) alignments; the scores of a pair's alignments never increase from one to the next.
 * Each round fills the pair's whole matrix again: max_hsps fills at worst.
 *
 * The arguments are those of swg_align_hits / _multi / _multi_pssm (only .index of a hit is read; hits in any order
 * and repeated; a view is accepted; the database must be resident; swg_align_hsps uses the context's query, index or
 * PSSM, and the batch calls neither read nor change it).  Outputs by hit slot s (s = h for swg_align_hsps, s = i*k + j
 * for the batch calls): n_hsps[s] alignments were written, to out[s*max_hsps + r], and, where the pointers are not
 * NULL, their counts (the four fields of swg_align_stats, for that alignment's path; a PSSM's identity against its
 * consensus) to counts[s*max_hsps + r] and their paths to ops + (s*max_hsps + r)*ops_stride.  n_hsps[s] is 0 when the
 * pair's best is below min_score.  Slots past n_hsps[s] are not written, nor those of hits past n_hits[i]; reserved = 0.
 * swg_align_ops_bound* still give a sufficient ops_stride.  With max_hsps = 1 and min_score = 1 every written field
 * and path equals swg_align_hits*.  Errors, all before anything is launched: max_hsps outside 1 .. SWG_MAX_HSPS,
 * min_score < 1, out or n_hsps NULL with a hit present (SWG_ERR_ARG); everything else as the swg_align_hits* call of the
 * same shape. */
#define SWG_MAX_HSPS 64
int swg_align_hsps(swg_ctx *ctx, const swg_db *db, const swg_hit *hits, size_t n_hits, uint32_t max_hsps, int32_t min_score,
                   swg_alignment *out, uint32_t *n_hsps, swg_align_counts *counts, char *ops, size_t ops_stride);
int swg_align_hsps_multi(swg_ctx *ctx, const swg_db *db, const int8_t *queries, const uint64_t *q_offsets, size_t n_queries,
                         const swg_hit *hits, size_t k, const size_t *n_hits, uint32_t max_hsps, int32_t min_score,
                         swg_alignment *out, uint32_t *n_hsps, swg_align_counts *counts, char *ops, size_t ops_stride);
int swg_align_hsps_multi_pssm(swg_ctx *ctx, const swg_db *db, const int8_t *pssms, const uint64_t *q_offsets, size_t n_queries,
                              const swg_hit *hits, size_t k, const size_t *n_hits, uint32_t max_hsps, int32_t min_score,
                              swg_alignment *out, uint32_t *n_hsps, swg_align_counts *counts, char *ops, size_t ops_stride);
/* The host twin: the same rule for one pair in plain C++ (no GPU needed).  Exactly one of query (lq table indices 1..31,
 * scored by sub) and pssm (lq rows of 32) is not NULL; seq holds len table indices.  out[max_hsps] (index = 0), and where
 * not NULL counts[max_hsps] and the paths at ops + r*ops_stride (lq + len + 1 is always enough); *n_out alignments were
 * written.  Errors are SWG_ERR_ARG / SWG_ERR_RESIDUE with swg_global_error() set. */
int swg_align_hsps_host(const int8_t sub[32][32], int gap_open, int gap_extend, const int8_t *query, const int8_t *pssm, size_t lq,
                        const int8_t *seq, size_t len, uint32_t max_hsps, int32_t min_score, swg_alignment *out,
                        swg_align_counts *counts, char *ops, size_t ops_stride, uint32_t *n_out);

/* ---- a PSSM from a query's hits (the step between two iterations of a profile search) ------------------- */

/* PSI-BLAST's construction (Altschul et al. 1997) with one simplification: the alignment block of every column is the
 * whole query, so a query has ONE set of sequence weights and ONE diversity figure.
 *   background  P = freq normalised (32 weights by residue index, validated as swg_synth_db_iid validates them; NULL: the
 *               built-in table of swg_synth_db), A = {a in 1..31 : P_a > 0}; lambda = swg_matrix_lambda(sub, freq).
 *   rows        row 0 is the query's own residues; row r >= 1 is hit r under the path swg_align_hits* spells for it (the
 *               same kernel, the same tie rules): an 'M' step puts the database residue into its query column, a 'D'
 *               step a gap, 'I' steps are dropped, columns outside [q_begin, q_end) are empty.  A residue outside A and
 *               a gap count as empty in everything below; a hit of score 0 contributes nothing; a hit listed twice
 *               counts twice.
 *   counts      n[p][a] rows showing a in column p; k_p distinct residues of column p; m_p = sum_a n[p][a]; Nbar = the
 *               mean of k_p over the columns with m_p >= 1.
 *   weights     w_r = sum over the columns p where row r shows a residue x of 1 / (k_p n[p][x])   (Henikoff).
 *   frequencies f[p][a] = (sum of w_r over the rows showing a in p) / (sum of w_r over the rows showing anything in p).
 *   pseudocounts alpha_p = min(Nbar, m_p) - 1, beta = pseudocount (finite, > 0),
 *               g[p][a] = P_a sum_{b in A} f[p][b] exp(lambda sub[b][a]),   Q = (alpha_p f + beta g) / (alpha_p + beta).
 *   scores      v[p][a] = ln(Q[p][a] / P_a) / lambda for a in A; pssm[p*32 + a] = v rounded half away from zero and
 *               clamped to -128..127; for a >= 1 outside A sub[query residue p][a], as swg_pssm_load fills the columns
 *               a file does not name; column 0 is 0; a column with m_p = 0 takes its whole row from sub[query residue p].
 * With no hits the PSSM is sub[query residue p][a] in every entry.  Every floating sum has a fixed order and nothing is
 * added atomically in floating point: two calls give the same bytes.  The host twin is swg_pssm_from_paths
 * (include/swg_host.h).
 *
 * Two options (swg_set_option, both default 0: the model above, byte for byte) take the simplification back and purge
 * near-identical hits, as PSI-BLAST does; swg_pssm_build, _multi and _multi_pssm read both.
 *   extents     row 0 has extent [0, lq); row r >= 1 of a hit of score > 0 has extent [b_r, e_r) = [q_begin, q_end) of
 *               the path swg_align_hits* spells; a hit of score 0 and a purged row have no extent and contribute nothing
 *               anywhere.
 *   "pssm_purge" = T, 0 (off) or 50..100 (percent identity; 94 is PSI-BLAST's), anything else SWG_ERR_ARG.  The purge
 *               runs before everything else, on the rows as written above.  For rows r and s, c(r, s) = the columns where
 *               both show a residue 1..31 (gaps and empty cells do not count; membership in A plays no part), i(r, s) =
 *               those of them where the two residues are equal.  Rows are taken in hit order, r = 1, 2, ...: row r is
 *               purged if c(r, 0) >= 1 and i(r, 0) = c(r, 0) (a copy of the query, at any T), or if some KEPT s with
 *               1 <= s < r has c(r, s) >= 1 and 100 i(r, s) >= T c(r, s) -- integers only; a row purged earlier purges
 *               no later one.  A purged row is then exactly a hit of score 0: not counted in n_rows, counted in n_purged.
 *   "pssm_blocks" = 1: per-column blocks.  For column p,
 *     rows      R_p = the rows whose extent contains p (a row that shows a gap or a residue outside A at p included;
 *               row 0 always);
 *     block     [L_p, U_p), L_p = max b_r and U_p = min e_r over R_p;
 *     counts    within the block and over the rows of R_p only: n^(p)[c][a] rows showing a in column c, k^(p)_c distinct
 *               residues of column c, m^(p)_c = sum_a n^(p)[c][a];
 *     weights   w^(p)_r = sum over the block's columns c where row r shows a residue x in A of 1 / (k^(p)_c n^(p)[c][x]);
 *     diversity Nbar_p = the mean of k^(p)_c over the block's columns with m^(p)_c >= 1;
 *     frequencies f[p][a] = (sum of w^(p)_r over the rows of R_p showing a at p) / (the same sum over the rows of R_p
 *               showing any residue of A at p);
 *     pseudocounts alpha_p = min(Nbar_p, m_p) - 1 with m_p as above; g, Q, v, the rounding, the clamping and the
 *               fallback columns are unchanged; info.n_distinct = the mean of Nbar_p over the columns with m_p >= 1.
 *               Gaps stay "empty", not a 21st letter.  Columns between two consecutive extent boundaries (a segment)
 *               share R_p, hence the block, the weights and Nbar_p; where every row spans the query the two models
 *               coincide.
 *   With pssm_blocks = 0 and the purge on, the whole-query model runs on the kept rows.
 * The host twin with the options is swg_pssm_from_paths_ex. */
#define SWG_PSSM_PSEUDOCOUNT_DEFAULT 10.0 /* PSI-BLAST's constant */
typedef struct swg_pssm_info {
    double lambda;       /* of (sub, freq) */
    double n_distinct;   /* Nbar; 0 when no column holds a residue of A */
    uint32_t n_rows;     /* rows used: the query and every hit of score > 0 that was not purged */
    uint32_t n_observed; /* columns in which some hit shows a residue of A */
    uint32_t n_clamped;  /* entries whose rounded score lay outside -128..127 */
    uint32_t n_purged;   /* hits dropped as near-identical ("pssm_purge"); 0 when purging is off */
} swg_pssm_info;

/* swg_pssm_build: the PSSM of the context's query from hits[n_hits] (only .index is read, as swg_align_hits reads them).
 * query_residues is NULL for an index query; for a PSSM query it is required -- the query's residues, as many as the
 * PSSM has rows: the hits are then aligned under the PSSM and row 0 is query_residues.  pssm_out [lq*32] in
 * swg_set_query_pssm's layout; values_out NULL or double[lq*32], the unrounded v (0 where there is none); info NULL or
 * one record.  The batch calls take the hit layout of swg_align_hits_multi, so swg_search_above_multi's hits_out with its
 * n_total clipped to cap goes in unchanged; PSSM i is written at pssms_out + q_offsets[i]*32 (values_out alike), ready
 * for swg_search_multi_pssm; info NULL or n_queries records.  swg_pssm_build_multi_pssm: pssms scores the alignments,
 * queries (same offsets) are the residues.  The context's own query is neither read nor changed by the batch calls.
 * The alignments' paths stay on the device: swg_pssm_rows_kernel turns them into the rows, three more kernels count,
 * weight and score (csrc/swg_pssm.hip); only the outputs come back.  The rows of a launch group take sum rows x lq bytes
 * of device memory; option "pssm_msa_mb" (default 1024; 0 .. 65536, 0: every query alone) bounds them -- a batch over the bound runs
 * in chunks of queries, a single query over it alone --, with the same bytes out.  With "pssm_purge" on, one kernel
 * compares every pair of a query's rows and a second resolves the greedy order; with "pssm_blocks" = 1 the segments are
 * listed on the device and one workgroup per (query, segment) counts, weights and scores in place of the three kernels.
 * What they keep in device memory counts against the same bound: the purge's bits, (rows + 1) x ceil(rows / 64) x 8 bytes
 * per query, and, for a query of more than 1024 rows, the weights of the rows beyond the 1024 a workgroup holds in LDS,
 * min(lq, 2 rows) x (rows - 1024) x 8 bytes.  The database must be resident; a view is
 * accepted.  Errors, all before anything is launched: those of swg_align_hits_multi (a hit not in the shard, a pair
 * outside what a traceback holds, NULL arguments, ...), pssm_out NULL with a query to build, a malformed freq, a
 * pseudocount that is not finite and positive, a matrix without a lambda: SWG_ERR_ARG. */
int swg_pssm_build(swg_ctx *ctx, const swg_db *db, const swg_hit *hits, size_t n_hits, const int8_t *query_residues,
                   const double *freq, double pseudocount, int8_t *pssm_out, double *values_out, swg_pssm_info *info);
int swg_pssm_build_multi(swg_ctx *ctx, const swg_db *db, const int8_t *queries, const uint64_t *q_offsets, size_t n_queries,
                         const swg_hit *hits, size_t k, const size_t *n_hits, const double *freq, double pseudocount,
                         int8_t *pssms_out, double *values_out, swg_pssm_info *info);
int swg_pssm_build_multi_pssm(swg_ctx *ctx, const swg_db *db, const int8_t *pssms, const int8_t *queries,
                              const uint64_t *q_offsets, size_t n_queries, const swg_hit *hits, size_t k, const size_t *n_hits,
                              const double *freq, double pseudocount, int8_t *pssms_out, double *values_out,
                              swg_pssm_info *info);

/* ---- composition-based score adjustment of reported hits -------------------------------------------------- */

/* The calibration behind swg_evalue scores the query against random sequences of ONE background composition; a database
 * sequence whose own composition is skewed the way the query's is scores far above what that predicts.  This is the
 * correction PSI-BLAST applies ("composition-based statistics", Schaffer et al. 2001, its mode 1): the pair is scored
 * again under scores scaled by the ratio of two ungapped lambdas.  It applies per query and per hit; the query is an
 * index query or a PSSM.  DESIGN 8.7.
 *   profile      R_p[a], p in 0..lq-1, a in 0..31: sub[q_p][a] for an index query, pssm[p*32 + a] for a PSSM.
 *   background   freq as swg_pssm_build takes it (NULL: the built-in table; validated the same way);
 *                A = {a in 1..31 : freq_a > 0}, P_a = freq_a / sum_A freq.
 *   composition  c_a = the number of residues a in A in the WHOLE hit sequence, n = sum_A c_a; residues outside A (X, B,
 *                Z, padding) are not counted.
 *   distribution C[a][s] = the number of positions p with R_p[a] == s, s in -128..127.  Against the subject
 *                h[s] = sum_{a in A} c_a C[a][s] (exact integers of total weight n lq); against the background
 *                hP[s] = sum_{a in A} P_a C[a][s].
 *   lambda       for weights w[s] of total W, lambda(w) is the positive root of sum_s w[s] exp(lambda s) = W; it exists
 *                exactly when sum_s s w[s] < 0 and some w[s] > 0 with s > 0.  lambda_std = lambda(hP), lambda_hit = lambda(h).
 *   ratio        r = min(1, max(0.5, lambda_hit / lambda_std)): scores are only ever scaled down, and by at most a half
 *                (constants of this contract).  ratio16 = floor(r 65536 + 0.5), in 32768..65536.
 *                n == 0, or either lambda does not exist: status 1, ratio16 = 65536.  The iteration does not converge in
 *                100 steps: status 2, ratio16 = 65536.  Otherwise status 0.  (lambda_hit is 0 unless it was solved.)
 *   rescaling    everything from here on is integer.  F = option "comp_scale", 1..64, default 32 (NCBI's scaling factor
 *                of this step).  T[s] = floor((s F ratio16 + 32768) / 65536), floor toward minus infinity, s in
 *                -128..127; |T| <= 8192, an int16.  The pair is scored by the library's recurrence unchanged (H, A and B
 *                floored at 0, go = open + extend, any signs) with the substitution score T[R_p[d_j]] and the gap scores
 *                F gap_open and F gap_extend -- the ratio does not scale the gaps --, in int32 cells.  scaled_score is
 *                that maximum, adj_score = floor((2 scaled_score + F) / (2 F)).
 * Consequences: ratio16 == 65536 gives T[s] = F s, scaled_score = F x (the pair's exact score) and adj_score = the exact
 * score.  F = 1 makes T an int8 table, so any scorer of the recurrence can score the pair.  The adjusted E-value is
 * swg_evalue(params, residues, adj_score) with the params of swg_calibrate on the same background.
 * The solver, one iteration for host and device (csrc/swg_comp_rule.h): hi = 1 / (the highest populated score) doubled
 * until the sum exceeds W, then Newton steps from hi, a step that leaves the bracket replaced by its middle; double
 * arithmetic, a fixed order of additions, no fused multiply-add; it stops at |step| <= 1e-12 lambda.  lambda_std is
 * solved once per query on the host, lambda_hit on the device from the exact integers h[s].
 *
 * swg_comp_adjust: the context's query (index or PSSM) against hits[n_hits]; only .index is read; hits in any order and
 * repeated.  out[n_hits] is parallel to the hits.  A hit whose sequence this handle (shard, view) does not hold is NOT
 * written and is no error, so the shards of one database fill one array between them; an index outside the whole
 * database is SWG_ERR_ARG.  lambda_std: NULL or one double (0 where it does not exist).  The batch calls take the layout of
 * swg_align_bounds_multi / _multi_pssm (row i's hits at hits[i*k .. i*k + n_hits[i]), out alike; slots past n_hits[i] are
 * not written; lambda_std NULL or n_queries doubles) and neither read nor change the context's own query; row i equals
 * swg_set_query(query i) + swg_comp_adjust.  The database must be resident (a view or a masked root is accepted: the
 * composition is that of the bytes the handle holds).  Three kernels (csrc/swg_comp.hip): the count tables C per query,
 * one workgroup per hit for composition, lambda_hit, ratio16 and the pair's table T, and a score-only lane-group fill
 * that reads every score through T; results come back in one copy.  A query of more than 2048 columns goes through the
 * host twin below inside the same call, with the same results.  Alignments, coordinates and counts (swg_align_*) stay
 * those of the unadjusted scores.
 * Errors, all before anything is launched: NULL arguments, a malformed freq, a pair whose cells could leave int32
 * ((lq + len) F max(127, |gap_open + gap_extend|, |gap_extend|) >= 2^31): SWG_ERR_ARG; a database that is not resident
 * or was built from 16-lane batches, no query or no scoring set, searches in flight on the context: SWG_ERR_STATE.
 * n_hits = 0 returns SWG_OK.  Group forms (swg_group_*) are out of scope. */
typedef struct swg_comp_result {
    int32_t adj_score, scaled_score;
    uint32_t ratio16;
    int32_t status;
    double lambda_hit;
} swg_comp_result;
int swg_comp_adjust(swg_ctx *ctx, const swg_db *db, const swg_hit *hits, size_t n_hits, const double *freq,
                    swg_comp_result *out, double *lambda_std);
int swg_comp_adjust_multi(swg_ctx *ctx, const swg_db *db, const int8_t *queries, const uint64_t *q_offsets, size_t n_queries,
                          const swg_hit *hits, size_t k, const size_t *n_hits, const double *freq, swg_comp_result *out,
                          double *lambda_std);
int swg_comp_adjust_multi_pssm(swg_ctx *ctx, const swg_db *db, const int8_t *pssms, const uint64_t *q_offsets, size_t n_queries,
                               const swg_hit *hits, size_t k, const size_t *n_hits, const double *freq, swg_comp_result *out,
                               double *lambda_std);
/* The host twin for one pair, in plain C++ (no GPU needed): exactly one of query (lq table indices 1..31, scored by sub)
 * and pssm (lq rows of 32) is not NULL; seq holds len table indices 0..31; scale is F.  out: one record; lambda_std NULL
 * or one double.  Errors are SWG_ERR_ARG / SWG_ERR_RESIDUE with swg_global_error() set. */
int swg_comp_adjust_host(const int8_t sub[32][32], int gap_open, int gap_extend, const int8_t *query, const int8_t *pssm,
                         size_t lq, const int8_t *seq, size_t len, const double *freq, int scale, swg_comp_result *out,
                         double *lambda_std);

/* ---- masking of low-complexity regions -------------------------------------------------------------------- */

/* The rule: the trigger and extension stages of SEG (Wootton & Federhen 1993), decided in integers.  There is NO third
 * stage: a kept segment is not trimmed to its least probable sub-segment, so this masks a little more than SEG does.
 *   window W (4..64), trigger K1 and extend K2 in bits (0 <= K1 <= K2), replace = the residue index written (1..31).
 *   T[0] = 0, T[c] = rint(c log2(c) 65536) for c = 1..W, computed once on the host in double.
 *   A window start s (0 <= s <= len - W) has counts c_a of each residue index a (all 32 indices, each a letter of its
 *   own) in [s, s + W); its weight is S(s) = sum_a T[c_a].  The window is LOW AT K iff
 *       S(s) >= ceil(W (log2 W - K) 65536),
 *   which is "entropy <= K".  For W = 12 the thresholds of K1 = 2.2 and K2 = 2.5 are 1089179 and 853250.
 *   A maximal run of consecutive window starts that are all low at K2 is KEPT iff at least one of its starts is low at
 *   K1.  Position i is masked iff some kept start s has s <= i < s + W.  A sequence shorter than W has no window and is
 *   left alone.
 * The device kernels (csrc/swg_mask.hip) and the host twin swg_seg_mask receive the same T and the same two thresholds
 * (swg_mask_tables), so their results are equal byte for byte. */
typedef struct swg_mask_params {
    int32_t window;  /* W */
    int32_t replace; /* residue index written at a masked position */
    double trigger;  /* K1 */
    double extend;   /* K2 */
} swg_mask_params;
#define SWG_MASK_WINDOW_DEFAULT 12
#define SWG_MASK_TRIGGER_DEFAULT 2.2
#define SWG_MASK_EXTEND_DEFAULT 2.5
#define SWG_MASK_REPLACE_DEFAULT 24 /* swg_letter_index('X') */
void swg_mask_params_default(swg_mask_params *p);
/* The integers of the rule: T[0..64] (entries past W are 0) and the thresholds of K1 and K2.  p NULL: the defaults.
 * SWG_ERR_ARG for parameters out of range (or not finite). */
int swg_mask_tables(const swg_mask_params *p, int32_t T[65], int64_t *thr_trigger, int64_t *thr_extend);
/* The host twin, and what a caller masks a QUERY with: mask_out[i] = 1 where position i of idx[len] (table indices 0..31)
 * is masked, 0 elsewhere (mask_out NULL: counts only); n_masked, n_segments (either NULL): the positions covered and the
 * kept runs.  idx is not changed: a caller writes p->replace where mask_out says so.  p NULL: the defaults. */
int swg_seg_mask(const int8_t *idx, size_t len, const swg_mask_params *p, uint8_t *mask_out, size_t *n_masked);
int swg_seg_mask_segments(const int8_t *idx, size_t len, const swg_mask_params *p, uint8_t *mask_out, size_t *n_masked,
                          size_t *n_segments);
/* One sequence back out of a database's host image (root, view, loaded file, masked copy): the table indices of the
 * sequence whose ORIGINAL index is given.  *len is always its length; the residues are written when cap >= *len (else
 * SWG_ERR_ARG with *len set, so that a caller can ask again).  A sequence this shard or view does not hold: SWG_ERR_ARG;
 * a database built from 16-lane batches: SWG_ERR_STATE.  Host only; a call walks the shard's slot table (it is for tests
 * and read-backs of a few sequences, not a bulk export). */
int swg_db_sequence(const swg_db *db, uint32_t original_index, int8_t *idx_out, size_t cap, size_t *len);

/* A masked copy of a resident database, made on the device: *out is an ordinary packed, resident ROOT database with
 * the parent's sequences, order, lengths, offsets and original indices and residue bytes of its own (one more byte
 * per residue on the host and on the device), in which every masked position holds `replace`; the fill bytes of a
 * sequence's last dword stay the padding residue.  Every call that takes a swg_db takes it unchanged; hits carry the
 * parent's original indices, so a caller may search the masked copy and align the hits against the parent (soft
 * masking).  It shares nothing with the parent: either may be freed first, and nothing the parent planned or tuned
 * changes.  Three kernels run over the resident bytes (window flags into bitmaps by sliding counts; kept runs, the
 * widening by W and the counts on 64-bit words; the bytes), then ONE device-to-host copy makes the host image.
 * Refusals, all before anything is launched: parent a view: SWG_ERR_ARG (mask the root and take the view of the
 * result); parent not resident on ctx's device, or built from 16-lane batches: SWG_ERR_STATE; parameters out of range:
 * SWG_ERR_ARG.  A failed allocation leaves nothing behind.  p NULL: the defaults. */
typedef struct swg_mask_info {
    swg_mask_params params;
    uint64_t residues_masked;  /* positions covered */
    uint64_t sequences_masked; /* sequences with at least one */
    uint64_t segments;         /* kept runs */
    double kernel_ms;          /* the kernels, from HIP events */
    double host_image_ms;      /* the device-to-host copy of the bytes that makes the host image (wall clock) */
} swg_mask_info;
int swg_db_mask(swg_ctx *ctx, const swg_db *parent, const swg_mask_params *p, swg_db **out);
/* What swg_db_mask made `db` with and what it covered (summed on the device); any other database -- one loaded from a
 * file included, which is an ordinary root whatever it was saved from --: SWG_ERR_STATE. */
int swg_db_mask_info(const swg_db *db, swg_mask_info *out);

/* ---- translated search: the six frames of a nucleotide database ------------------------------------------------ */

/* The rule.  A nucleotide database is an ordinary database packed from nucleotide letters (residue index = position of
 * the letter: swg_letter_index).  A residue index names a BASE with a 2-bit code, in NCBI's TCAG order:
 *     20 (T) or 21 (U) -> 0,   3 (C) -> 1,   1 (A) -> 2,   7 (G) -> 3,   anything else (N, IUPAC codes, '*', 0) -> no base.
 * The three bit planes below give, at bit `index`, the low and the high bit of the code and whether there is a base;
 * the kernel and the host twin read the same three words.  The complement of code c is c ^ 2 (T <-> A, C <-> G).
 *   A codon of bases b1 b2 b3 translates to codon[16 b1 + 4 b2 + b3] (a residue index 1..31; 31 = '*' is a stop); a
 *   codon with any position that is no base translates to `unknown` (default 24 = X).  An ambiguous codon that still
 *   names one amino acid (GCN) is NOT resolved.
 *   For a sequence of L nucleotides, frame f = 0, 1, 2 reads the codons that start at f, f + 3, ... of the forward
 *   strand and frame 3 + f the same offsets of the reverse complement; both have (L - f) / 3 residues (0 when
 *   L - f < 3): a trailing partial codon is dropped, and a stop is a residue in place -- it does not split the frame.
 *   Frame g (0..5) of the sequence with original index i is the sequence with original index 6 i + g. */
#define SWG_NT_PLANE_LO 0x00000088u   /* bit 0 of the code: C (3), G (7) */
#define SWG_NT_PLANE_HI 0x00000082u   /* bit 1 of the code: A (1), G (7) */
#define SWG_NT_PLANE_BASE 0x0030008Au /* a base at all: A, C, G, T (20), U (21) */
#define SWG_TRANSLATE_UNKNOWN_DEFAULT 24 /* swg_letter_index('X') */
typedef struct swg_translate_params {
    int8_t codon[64]; /* residue index (1..31) of codon 16 b1 + 4 b2 + b3, TCAG order */
    int8_t unknown;   /* residue index (1..31) of a codon with a position that is no base */
} swg_translate_params;
/* NCBI genetic codes 1, 2, 3, 4, 5, 6 and 11 with unknown = X; any other id: SWG_ERR_ARG (a caller with another code
 * fills the struct).  Host only. */
int swg_codon_table(int ncbi_id, swg_translate_params *out);
/* The host twin: the six frames of nt[nt_len] (residue indices 0..31).  out[g] must have room for nt_len / 3 residues;
 * len_out[g] is frame g's length.  p NULL: code 1.  SWG_ERR_ARG: NULL arguments, a table entry or unknown outside
 * 1..31. */
int swg_translate_seq(const int8_t *nt, size_t nt_len, const swg_translate_params *p, int8_t *out[6], size_t len_out[6]);
/* The same over a whole database laid end to end, on every core: sequence i is flat[offsets[i] .. offsets[i+1]); frame
 * g of sequence i becomes sequence 6 i + g of out_flat / out_offsets[6 n + 1].  out_flat needs room for
 * 2 (offsets[n] - offsets[0]) residues.  What a caller without swg_db_translate does in front of swg_db_pack. */
int swg_translate_flat(const int8_t *flat, const uint64_t *offsets, size_t n, const swg_translate_params *p, int8_t *out_flat,
                       uint64_t *out_offsets);
/* A hit of a translated database back to the nucleotide record: index = 6 nt_index + frame, frame 0..5 (0..2 forward,
 * 3..5 = offsets 0..2 of the reverse complement; BLAST writes them +1 +2 +3 -1 -2 -3).  Pure arithmetic. */
void swg_translate_hit(uint32_t index, uint32_t *nt_index, int *frame);
/* The nucleotides a residue range of a frame covers.  [d_begin, d_end) is 0-based and half-open in the frame's residues,
 * as swg_alignment gives it; the answer is 0-based and half-open on the FORWARD strand, nt_begin < nt_end:
 *     frame f:      [f + 3 d_begin, f + 3 d_end)          frame 3 + f:  [L - f - 3 d_end, L - f - 3 d_begin)
 * with L = nt_len, the length of the nucleotide record.  An alignment of score 0 has n_ops = 0 and the empty range
 * d_begin = d_end: it covers no nucleotide and is SWG_ERR_ARG here, as are a frame outside 0..5 and a range that ends
 * past the frame's (L - f) / 3 residues. */
int swg_translate_coords(int frame, uint32_t nt_len, uint32_t d_begin, uint32_t d_end, uint32_t *nt_begin, uint32_t *nt_end);

/* The six-frame translation of a resident NUCLEOTIDE database, made on the device: *out is an ordinary packed, resident
 * ROOT database of 6 x the parent's sequences -- frame g of the parent's original index i has original index 6 i + g,
 * swg_db_total_count is 6 x the parent's -- indistinguishable from swg_db_pack + swg_db_upload of the host twin's
 * frames given in index order: the same order (length descending, stable), bins, offsets and residue bytes, fill bytes
 * included.  Every call that takes a swg_db takes it unchanged (searches, batches, PSSMs, lists, alignments,
 * statistics, calibration, swg_db_mask, swg_db_view).  The host builds the slot tables from the parent's lengths alone
 * and uploads them with one word per (parent slot, frame) that says where the frame goes: tens of bytes per translated
 * sequence and never a residue.  One kernel writes the residue bytes from the parent's resident ones; ONE
 * device-to-host copy then makes the host image.  Nothing is shared with the parent: either may be freed first.
 * Refusals, all before anything is launched: parent a view: SWG_ERR_ARG (translate the root and take the view of the
 * result: its indices are 6 i + g); parent not resident on ctx's device, or built from 16-lane batches: SWG_ERR_STATE;
 * a table entry or unknown outside 1..31, or a parent with 6 x total count >= 0xFFFFFFF0: SWG_ERR_ARG.  A shard is a
 * root: its frames keep 6 x the global index + g.  A masked root is accepted.  p NULL: code 1. */
typedef struct swg_translate_info {
    swg_translate_params params;
    uint64_t codons;         /* residues written: the sum of the six frames' lengths */
    uint64_t stops;          /* codons of three bases that the table sends to 31 ('*') */
    uint64_t unknown_codons; /* codons with a position that is no base */
    double kernel_ms;        /* the kernel, from HIP events */
    double host_image_ms;    /* the device-to-host copy of the bytes that makes the host image (wall clock) */
} swg_translate_info;
int swg_db_translate(swg_ctx *ctx, const swg_db *parent, const swg_translate_params *p, swg_db **out);
/* What swg_db_translate made `db` with and what it wrote; any other database -- a saved translation that was loaded
 * again included, which is the ordinary root it was saved as --: SWG_ERR_STATE. */
int swg_db_translate_info(const swg_db *db, swg_translate_info *out);

/* ---- multi-GPU merge -------------------------------------------------- */

/* 64-bit sort key of a hit: (score << 32) | (0xFFFFFFFF - index).  Larger key =
 * better hit, so one max-all-reduce (RCCL, ncclMax on n_gpus*k keys) or one
 * all-gather merges the shards' top-K lists. */
uint64_t swg_hit_key(int32_t score, uint32_t index);
void swg_key_hit(uint64_t key, swg_hit *out);
/* keys[n] (zeros ignored) -> best k hits, sorted.  Returns hits written. */
size_t swg_topk_merge_keys(const uint64_t *keys, size_t n, size_t k, swg_hit *out);

/* ---- several GPUs in one process ----------------------------------------- */

/* A group owns one context per device.  swg_group_load deals the database's bins round-robin
 * over the devices; swg_group_search runs all shards concurrently and merges their top-K lists
 * with a single RCCL max-all-reduce of n_gpus*k hit keys (RCCL is loaded on first use; with one
 * device no collective is issued unless force_collective is set, which is how a 1-GPU box
 * rehearses the path).  scores_out is indexed by original database index; stats, if given, is
 * an array of swg_group_size() entries.  (bench.py uses the other arrangement: one process per
 * GPU, torch.distributed over RCCL.) */
typedef struct swg_group swg_group;
int swg_group_create(const int *devices /* NULL: 0..n-1 */, int n, int force_collective, swg_group **out);
void swg_group_destroy(swg_group *g);
int swg_group_size(const swg_group *g);
const char *swg_group_last_error(const swg_group *g);
int swg_group_set_option(swg_group *g, const char *key, long value);
int swg_group_set_scoring(swg_group *g, const int8_t sub[32][32], int gap_open, int gap_extend);
int swg_group_set_query(swg_group *g, const int8_t *idx, size_t lq);
int swg_group_set_query_pssm(swg_group *g, const int8_t *pssm, size_t lq); /* swg_set_query_pssm on every device */
int swg_group_load(swg_group *g, const int8_t *flat, const uint64_t *offsets, size_t n);
int swg_group_search(swg_group *g, int32_t *scores_out, swg_hit *topk_out, size_t k, size_t *n_hits,
                     swg_stats *stats);
/* swg_align_hits for a group: every hit is re-run on the GPU whose shard holds the sequence. */
int swg_group_align_hits(swg_group *g, const swg_hit *hits, size_t n_hits, swg_alignment *out, char *ops,
                         size_t ops_stride);
size_t swg_group_align_ops_bound(const swg_group *g);
/* Restrict the group to the listed sequences (original indices of the loaded database; the rules of swg_db_view):
 * every device makes a view of its shard from the same list, and swg_group_search, swg_group_align_hits and
 * swg_group_align_ops_bound use the views until the next swg_group_select.  indices == NULL returns to the whole
 * database.  swg_group_load drops a selection. */
int swg_group_select(swg_group *g, const uint32_t *indices, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* SWG_H */
