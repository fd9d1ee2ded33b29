// swg_diag_host.cpp -- host side of the diagonal engine: geometry planning, the
// pair-major token array of the work queue, and the stream layout of the fixed-stream
// form (which pair of sequences runs in which lane group, in what order).  Host-only C++ (OpenMP); no GPU needed.
#include "swg_host_internal.h"
#include "../../include/swg_host.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <mutex>
#include <queue>

static std::mutex g_plan_cache_mutex; // (swg_db::plan_key, plan_last: databases may be searched from several threads)

// Cycles one SIMD needs per packed-int16 / DPP / v_perm wave-instruction when `wps` waves share
// it.  One wave: the microbenchmark (profiles/r01_valu_issue_rates.txt).  Two to four: from the
// fill kernel itself on a uniform database (tools/sweeps/occ.sh): three waves per SIMD are as good
// as four, two cost 5 %; the microbenchmark's 5.3 / 5.05 / 4.56 were pessimistic.
static const double kCyclesPerInstr[5] = {0.0, 6.8, 4.55, 4.27, 4.35};
// ... and per instruction of a raised-priority wavefront beside three others (traced: the long
// class advances a 4-row block of 64 x 6 columns, 296 instructions, every 1.6 us)
static const double kHotCycles = 13.0;

uint64_t swg_db_pair_count(const swg_db *db) { return (db->n_local + 1) / 2; }

// Rows of the pairs [pair_begin, pair_end) (two reset rows + the longer sequence's residues each) and the longest of
// them.  The planner asks on every search, for prefixes of the sorted order: a prefix sum, built on first use (8 bytes per
// pair), makes that O(1) -- the loop it replaces walked 5 million pairs per search of the 10M-sequence database and, for
// 2 million peptides, cost more than the fill (round 4: step 1.39 ms for a 0.97 ms fill).
uint64_t swg_db_pair_rows(const swg_db *db, uint64_t pair_begin, uint64_t pair_end, uint64_t *longest_rows)
{
    const uint64_t n = swg_db_pair_count(db);
    std::vector<uint64_t> &pre = const_cast<swg_db *>(db)->pair_rows_prefix;
    if (pre.size() != n + 1) {
        pre.assign(n + 1, 0);
        for (uint64_t p = 0; p < n; ++p) pre[p + 1] = pre[p] + 2ull + db->lens[2 * p];
    }
    pair_end = std::min(pair_end, n);
    if (pair_begin >= pair_end) {
        if (longest_rows) *longest_rows = 0;
        return 0;
    }
    if (longest_rows) *longest_rows = 2ull + db->lens[2 * pair_begin]; // (sorted longest first)
    return pre[pair_end] - pre[pair_begin];
}

uint64_t swg_db_pairs_longer_than(const swg_db *db, uint64_t rows)
{
    // pairs are sorted by length, longest first: binary search the prefix
    uint64_t lo = 0, hi = swg_db_pair_count(db);
    while (lo < hi) {
        const uint64_t mid = (lo + hi) / 2;
        if (2ull + db->lens[2 * mid] > rows) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Cost model (cycles of one SIMD per packed/DPP wave-instruction, measured):
//   a lane group spends (10*K + overhead) instructions per database row; a SIMD shared by
//   `wps` waves issues one such instruction every kCyclesPerInstr[wps] cycles, so one wave
//   advances a row every instr * kCyclesPerInstr[wps] * wps cycles.  A search lasts as long
//   as the larger of (a) all work divided by all SIMDs and (b) the longest chain of rows any
//   one lane group has to walk.  The few longest pairs can be split off into their own class
//   (64 lanes per pair, fewest columns per lane, raised wave priority) so that (b) does not
//   dominate small databases.
// 10 per column pair plus the row's bookkeeping: 14 instructions, but worth about 30 issue slots
// (DPP wait states, the wait for the row's first profile read) by the K = 16 / 24 / 32 comparison
// (the packed-f16 cells, form 2, take 8.5 per column pair, 7.5 with the fma pairing: DESIGN 4.1)
static double instr_per_row(int K, int G, int form = 0, bool fma = false)
{
    // (the gapless cells, form 3: 3.5 per column pair)
    return (form == 3 ? 3.5 : form == 2 ? (fma ? 7.5 : 8.5) : 10.0) * K + (G == 32 ? 34.0 : 30.0);
}

// The f16 cells' pairings a geometry may take (f16_pair: 0 both, ranked by the model; 1 v_perm_b32 only; 2 the fma
// pairing wherever its doubled profile fits, v_perm_b32 elsewhere): bit 0 perm, bit 1 fma.  W: the wavefronts whose
// lane-group records share the LDS with the profile (0: the profile alone).  edges: one pass of several.  (The fma
// form's instantiations with edges at 23 and 24 columns do not fit their 128 registers -- 19 and 22 spilled -- and are
// left out.)  With f16_pair = 2 both bits are set where the fma pairing fits: the caller takes the fma pairing and
// keeps v_perm_b32 for the geometries whose fma candidate its later rules drop (plan_candidates).
static int pairings(int form, int K, int G, int W, bool edges, long f16_pair)
{
    if (form != 2) return 1;
    const bool fits = (W > 0 ? swg_diag_dyn_lds_bytes(K, G, W, true) : swg_diag_slice_bytes(K, G, true)) <= SWG_LDS_PER_CU;
    if (!fits || f16_pair == 1 || (edges && (K == 23 || K == 24))) return 1;
    return 3;
}
// one pass of several through the work queue: row index, edge hand-over to the leader, the tail's
// edge store
static const double kEdgeInstr = 7.0;

// Wavefronts per SIMD the work-queue kernel reaches at (K, G) with the perm pairing's profile, at its best workgroup size
static int perm_occupancy(const SwgKernelInfo &info, int G)
{
    int best = 0;
    for (int W = 4; W <= info.max_waves; W += 4)
        best = std::max(best, std::min(4, W / 4 * swg_workgroups_per_cu(info.max_waves, W, swg_diag_dyn_lds_bytes(info.K, G, W))));
    return best;
}

// Long class: the cheapest geometry (instructions per pair-row, column padding included)
// whose longest chain still finishes within `budget_cycles`; if none does, the shortest chain.
long g_swg_long_cols = 0;  // experiment switch: restrict the long class to this K (0 = free)
long g_swg_long_group = 0; // experiment switch: restrict the long class to this G (0 = free)

static bool long_class_geometry(size_t lq, uint64_t longest_rows, double budget_cycles, bool dynamic, SwgDiagPlan *lp, int form,
                                long f16_pair)
{
    bool ok = false, ok_fit = false;
    double best_cost = 1e300, best_depth = 1e300;
    SwgDiagPlan fit, fast;
    const int groups[2] = {32, 64};
    for (int v = 0; v < swg_num_diag_variants(); ++v) {
        const SwgKernelInfo info = swg_diag_variant_info(v);
        if (g_swg_long_cols > 0 && info.K != (int)g_swg_long_cols) continue;
        // with static streams the 2-column-chunk instantiations (K % 4 == 2) measured slower as the
        // long class than the next multiple of 4 despite fewer instructions: only on request there.
        // With the work queue they win (64 x 6 = 384 columns for a 367-column query: no padding
        // beyond the bulk's).
        if (!dynamic && g_swg_long_cols == 0 && info.K % 4 != 0) continue;
        for (int gi = 0; gi < 2; ++gi) {
            const int G = groups[gi];
            if (g_swg_long_group > 0 && G != (int)g_swg_long_group) continue;
            const size_t cols = (size_t)G * info.K;
            if ((size_t)G * swg_diag_padded_cols(info.K) * 64 > SWG_LDS_PER_CU) continue;
            const int npass = (int)((lq + cols - 1) / cols);
            if (dynamic && npass > 1) continue; // the queue serves single-pass classes only
            // (the f16 cells: the fma pairing where it fits beside the records of the class's four wavefronts)
            const bool fma = pairings(form, info.K, G, 4, npass > 1, f16_pair) & 2;
            const double instr = npass * instr_per_row(info.K, G, form, fma);
            const double cost = instr / (64 / G);                     // per pair-row
            const double depth = ((double)longest_rows + G) * instr * kHotCycles;
            SwgDiagPlan c;
            c.variant = v;
            c.K = info.K;
            c.G = G;
            c.npass = npass;
            c.W = 4;
            c.fma = fma ? 1 : 0;
            c.lds_bytes = swg_diag_slice_bytes(info.K, G, fma);
            if (depth <= budget_cycles && cost < best_cost) {
                best_cost = cost;
                fit = c;
                ok_fit = true;
            }
            if (depth < best_depth) {
                best_depth = depth;
                fast = c;
                ok = true;
            }
        }
    }
    if (ok_fit) *lp = fit; else if (ok) *lp = fast;
    return ok;
}

// sorted = false: only cands[0] is the first-ranked plan (what swg_plan_diag_work needs, on every search: no sort)
static int plan_candidates(const swg_db *db, size_t lq, int n_cu, long opt_cols, long opt_group, long opt_waves,
                           long opt_long_split, bool allow_split, bool work_queue, std::vector<SwgDiagWork> *cands,
                           double copies, int form, long f16_pair, bool sorted)
{
    // copies > 1: the same database is searched by that many queries in ONE launch (swg_search_multi):
    // all throughput terms grow with it, the longest chain of rows does not
    cands->clear();
    const uint64_t n_pairs = swg_db_pair_count(db);
    if (n_pairs == 0) return 0;
    if (copies < 1.0) copies = 1.0;
    uint64_t longest = 0;
    const uint64_t rows_once = swg_db_pair_rows(db, 0, n_pairs, &longest);
    const double rows_all = (double)rows_once * copies;
    const bool have_long = allow_split && opt_long_split >= 0;
    const double simds = 4.0 * n_cu;
    const int groups[3] = {16, 32, 64};
    for (int v = 0; v < swg_num_diag_variants(); ++v) {
        const SwgKernelInfo info = swg_diag_variant_info(v);
        if (opt_cols > 0 && info.K != (int)opt_cols) continue;
        for (int gi = 0; gi < 3; ++gi) {
            const int G = groups[gi];
            if (opt_group > 0 && G != (int)opt_group) continue;
            const size_t cols = (size_t)G * info.K;
            if (swg_diag_slice_bytes(info.K, G) > SWG_LDS_PER_CU) continue;
            const int npass = (int)((lq + cols - 1) / cols);
            if (form == 3 && npass > 1) continue; // the gapless cells have no edges: one pass or not at all
            const int NG = 64 / G;
            // with the work queue (several passes: one launch per pass) there are no fixed shares, the
            // chain that matters is the longest pair at the rate of a wavefront that gets its fair
            // share of the SIMD
            const bool dynamic = work_queue && (npass == 1 || db->n_local < (1u << 30));
            // the f16 cells' two pairings are two candidates: the fma one's profile is twice the size (occupancy).
            // f16_pair = 2 ("fma wherever it fits, v_perm_b32 elsewhere"): the fma candidates first, and the perm ones
            // of this (K, G) only when the rules below left none of them standing -- the records do not fit beside the
            // doubled profile at the workgroup size asked for, or it would cost resident wavefronts -- so that the
            // option plans wherever f16_pair = 1 does
            const size_t n_before = cands->size();
            for (int step = 0; step <= 1; ++step) {
            const int fma = f16_pair == 2 ? 1 - step : step;
            if (f16_pair == 2 && !fma && cands->size() > n_before) continue;
            // (the f16 cells run on the work queue only)
            if (!(pairings(form, info.K, G, 0, npass > 1, f16_pair) & (1 << fma)) || (fma && !dynamic)) continue;
            const size_t lds = swg_diag_slice_bytes(info.K, G, fma);
            const double instr = instr_per_row(info.K, G, form, fma) + (dynamic && npass > 1 ? kEdgeInstr : 0.0);
            for (int wps = 1; wps <= 4; ++wps) {
                const int W = 4 * wps;
                if (W > info.max_waves) continue;
                if (opt_waves > 0 && W != (int)opt_waves) continue;
                // with the work queue the workgroup size does not matter for balance; four wavefronts
                // (one per SIMD) interleave the two classes on every CU, larger workgroups partition the
                // CUs between them (timed faster in isolation, slower back to back).  Larger ones only
                // where LDS allows a single workgroup per CU and more wavefronts mean more occupancy.
                if (dynamic && opt_waves == 0 && wps != 1) {
                    // (occupancy by the workgroup's real LDS size, lane-group records included: at exactly two
                    // profiles per CU they decide whether a second workgroup fits)
                    auto occupancy = [&](int w) {
                        const size_t l = swg_diag_dyn_lds_bytes(info.K, G, 4 * w, fma);
                        return std::min(4, w * swg_workgroups_per_cu(info.max_waves, 4 * w, l));
                    };
                    bool improves = true;
                    for (int w2 = 1; w2 < wps; ++w2)
                        if (occupancy(w2) >= occupancy(wps)) improves = false;
                    if (!improves) continue;
                }
                // (the work-queue kernels keep a 512-byte record per lane group behind the profile)
                if (fma && swg_diag_dyn_lds_bytes(info.K, G, W, true) > SWG_LDS_PER_CU) continue;
                const size_t lds_wg = dynamic ? swg_diag_dyn_lds_bytes(info.K, G, W, fma) : lds;
                const int per_cu = swg_workgroups_per_cu(info.max_waves, W, lds_wg);
                const int eff_wps = std::min(4, wps * per_cu);
                // the fma pairing only where its doubled profile costs no resident wavefronts: at fewer per SIMD than the
                // perm pairing reaches with the same columns and lanes it measured slower (config 2, 16 x 23: two
                // wavefronts per SIMD instead of four, -1.6 %), whatever the instruction count says
                if (fma && eff_wps < perm_occupancy(info, G)) continue;
                const uint64_t spw = (uint64_t)W * NG;
                const uint64_t hw_streams = (uint64_t)n_cu * per_cu * spw;
                // (a long class beside a multi-pass queue launch would need its own edge buffers: not built)
                for (int split = 0; split <= (have_long && !(dynamic && npass > 1) ? 3 : 0); ++split) {
                    uint64_t n_long = 0, longest_bulk = longest, longest_long = 0;
                    double rows_long = 0;
                    uint64_t streams0 = std::max<uint64_t>(1, std::min<uint64_t>(hw_streams, (uint64_t)((double)n_pairs * copies)));
                    streams0 = (streams0 + spw - 1) / spw * spw;
                    if (split) {
                        if (split == 3 && opt_long_split > 0) continue;
                        // experiment switch long_group=16: only the bulk's own geometry as the long class
                        if (g_swg_long_group == 16 && split != 2) continue;
                        if (g_swg_long_group != 16 && g_swg_long_group > 0 && split == 2) continue;
                        const double frac = split == 3 ? 0.6 : 0.33;
                        uint64_t thr = opt_long_split > 0 ? (uint64_t)opt_long_split
                                                          : (uint64_t)(frac * rows_all / (double)streams0);
                        if (dynamic && opt_long_split <= 0) {
                            // longest pair a fair-share wavefront finishes within the whole search
                            const double cps0 = kCyclesPerInstr[eff_wps]; // (a database that needs a long class fills its slots)
                            const double all_cycles = rows_all / NG * instr * cps0 / simds;
                            thr = (uint64_t)((split == 3 ? 0.65 : 0.9) * all_cycles / (instr * cps0 * eff_wps));
                        }
                        thr = std::max<uint64_t>(thr, 64);
                        if (longest <= thr) continue;
                        n_long = swg_db_pairs_longer_than(db, thr);
                        if (n_long == 0 || n_long * 4 > n_pairs) continue;
                        rows_long = (double)swg_db_pair_rows(db, 0, n_long, &longest_long) * copies;
                        longest_bulk = 2ull + db->lens[2 * n_long];
                    }
                    const uint64_t n_bulk = n_pairs - n_long;
                    const double rows_bulk = rows_all - rows_long;
                    uint64_t streams = std::max<uint64_t>(1, std::min<uint64_t>(hw_streams, (uint64_t)((double)n_bulk * copies)));
                    streams = (streams + spw - 1) / spw * spw;
                    // A database of few pairs does not fill the wave slots the geometry allows: the chain's wavefront
                    // shares its SIMD with as many others as the launch really has (a 300 000-row sequence among 400
                    // short ones, lq 400: 64 lanes x 17 columns ranked first -- "one wavefront per SIMD" by its LDS
                    // size, where 64 x 7 has the SIMD to itself just the same at half the instructions per row).
                    const int eff = std::max(1, std::min(eff_wps, (int)std::ceil((double)(streams / spw) * W / simds)));
                    const double cps = kCyclesPerInstr[eff];
                    // (a) throughput: SIMD-cycles of both classes over all SIMDs
                    double work = rows_bulk / NG * npass * instr * cps;
                    double crit = (std::max<double>(rows_bulk / streams, (double)longest_bulk) + G) * npass *
                                  instr * cps * eff;
                    uint64_t lstreams = 0;
                    SwgDiagPlan lp;
                    if (split) {
                        // the long pairs have to be done by the time the bulk is
                        const double bulk_cycles = std::max(work / simds, crit);
                        if (split == 2) {
                            // the bulk's own geometry (no extra column padding), own streams, raised priority
                            lp.variant = v;
                            lp.K = info.K;
                            lp.G = G;
                            lp.npass = npass;
                            lp.W = 4;
                            lp.fma = fma;
                            lp.lds_bytes = lds;
                        } else if (!long_class_geometry(lq, longest_long, 0.8 * bulk_cycles, dynamic, &lp, form, f16_pair)) {
                            continue;
                        }
                        const uint64_t lspw = 4ull * (64 / lp.G);
                        // static: two pairs per stream to balance; queue: a wavefront on every SIMD
                        lstreams = std::max<uint64_t>(1, std::min<uint64_t>(dynamic ? (uint64_t)((double)n_long * copies) : (n_long + 1) / 2,
                                                                            (uint64_t)n_cu * lspw));
                        lstreams = (lstreams + lspw - 1) / lspw * lspw;
                        const double linstr = instr_per_row(lp.K, lp.G, form, lp.fma != 0);
                        work += rows_long / (64 / lp.G) * lp.npass * linstr * cps;
                        const double lcrit = (std::max<double>(rows_long / lstreams, (double)longest_long) + lp.G) *
                                             lp.npass * linstr * kHotCycles;
                        crit = std::max(crit, lcrit);
                    }
                    double cycles = std::max(work / simds, crit);
                    if (dynamic)
                        cycles += (npass - 1) * 0.15e-3 * 2.35e9; // a launch per pass: drain and ramp
                    else
                        cycles *= 1.0 + 0.04 * (npass - 1); // profile reloads, pass barriers, edge spills
                    // fixed streams lose what the work queue was built to recover (uneven wavefront
                    // rates, a thinning tail): measured 4 900 against 5 600 GCUPS on config 2
                    if (!dynamic) cycles *= 1.15;
                    // Workgroups of more than four wavefronts are candidates only where they raise the
                    // occupancy (above), and then they deliver it -- round 2, 200 000 sequences: lq 800 7 030
                    // against 6 750 GCUPS, lq 1000 7 060 against 6 820, lq 2500 (3 passes) 6 800 against 6 450
                    // with 12 wavefronts instead of 4 -- so they carry no penalty of their own (round 1 had one).
                    // Where a third wavefront per SIMD hurts, it is through the longest pair's chain, which
                    // `crit` prices (config 5's 8 200-row near-copies: 6 070 with 12 against 6 590 with 8).
                    // a second class is a second launch that takes LDS and issue slots from the bulk: worth
                    // it where the chain decides, not for a tie (lq 600: 6 420 with 19 long pairs, 6 880 without)
                    if (split) cycles *= 1.02;
                    // (where a chain decides, the plans it ties are told apart by their throughput time)
                    const double ms = (cycles + 1e-3 * work / simds) / 2.35e9 * 1e3;
                    {
                        SwgDiagWork one;
                        SwgDiagWork *wk = &one;
                        SwgDiagPlan &b = wk->plan[0];
                        b.variant = v;
                        b.K = info.K;
                        b.G = G;
                        b.npass = npass;
                        b.W = W;
                        b.fma = fma;
                        b.n_streams = (uint32_t)streams;
                        b.workgroups = (int)(streams / spw);
                        b.lds_bytes = lds;
                        b.est_ms = ms;
                        wk->pair_begin[0] = n_long;
                        wk->pair_end[0] = n_pairs;
                        wk->n_classes = 1;
                        if (split) {
                            wk->n_classes = 2;
                            wk->plan[1] = lp;
                            wk->plan[1].n_streams = (uint32_t)lstreams;
                            wk->plan[1].workgroups = (int)(lstreams / (4ull * (64 / lp.G)));
                            wk->plan[1].est_ms = ms;
                            wk->pair_begin[1] = 0;
                            wk->pair_end[1] = n_long;
                        }
                        cands->push_back(one);
                    }
                }
            }
            }
        }
    }
    // (a positive long_split is a request: plans with the class it asks for rank before those without, whatever
    // the model thinks of them -- when no pair is that long there are none, and the rest is ranked as usual)
    const bool want_long = have_long && opt_long_split > 0;
    auto before = [want_long](const SwgDiagWork &a, const SwgDiagWork &b) {
        const bool la = want_long && a.n_classes == 2, lb = want_long && b.n_classes == 2;
        return la != lb ? la : a.plan[0].est_ms < b.plan[0].est_ms;
    };
    if (sorted) std::stable_sort(cands->begin(), cands->end(), before);
    else if (!cands->empty()) std::iter_swap(cands->begin(), std::min_element(cands->begin(), cands->end(), before)); // (the first of equals, as the stable sort)
    return (int)cands->size();
}

int swg_plan_diag_candidates(const swg_db *db, size_t lq, int n_cu, long opt_cols, long opt_group, long opt_waves,
                             long opt_long_split, bool allow_split, bool work_queue, std::vector<SwgDiagWork> *cands,
                             double copies, int form, long f16_pair)
{
    return plan_candidates(db, lq, n_cu, opt_cols, opt_group, opt_waves, opt_long_split, allow_split, work_queue, cands, copies,
                           form, f16_pair, true);
}

int swg_plan_diag_work(const swg_db *db, size_t lq, int n_cu, long opt_cols, long opt_group, long opt_waves,
                       long opt_long_split, bool allow_split, bool work_queue, SwgDiagWork *wk, double copies, int form, long f16_pair)
{
    // (the experiment switches of the long class are part of the question too)
    const std::vector<double> key = {(double)lq, (double)n_cu, (double)opt_cols, (double)opt_group, (double)opt_waves,
                                     (double)opt_long_split, (double)allow_split, (double)work_queue, copies, (double)form,
                                     (double)f16_pair, (double)g_swg_long_cols, (double)g_swg_long_group,
                                     (double)swg_db_pair_count(db)};
    swg_db *mdb = const_cast<swg_db *>(db);
    {
        std::lock_guard<std::mutex> lock(g_plan_cache_mutex);
        if (mdb->plan_key == key) {
            *wk = mdb->plan_last;
            return mdb->plan_last_n;
        }
    }
    std::vector<SwgDiagWork> c;
    wk->n_classes = 0;
    if (plan_candidates(db, lq, n_cu, opt_cols, opt_group, opt_waves, opt_long_split, allow_split, work_queue, &c, copies, form,
                        f16_pair, false) > 0)
        *wk = c[0];
    std::lock_guard<std::mutex> lock(g_plan_cache_mutex);
    mdb->plan_key = key;
    mdb->plan_last = *wk;
    mdb->plan_last_n = wk->n_classes;
    return wk->n_classes;
}

// Tokens of one pair of sequences (two reset rows, then one row per residue of the longer
// one, the last block filled up with padding rows), one 32-bit token per row: byte 0 = X residue
// byte, byte 1 = Y residue byte, bit 16 = reset row, bit 17 = last row; returns the number of 4-row
// blocks.  The device builds the same image from the resident residue bytes
// (swg_build_tokens_kernel); this is its host restatement, used by the fixed-stream layout and by
// the tests that compare the two.
static const uint32_t kTokReset = SWG_TOK_RESET, kTokLast = SWG_TOK_LAST;
static uint64_t write_pair_tokens(const swg_db *db, size_t p, uint32_t *t)
{
    const size_t n_slots = (size_t)db->n_bins * SWG_BIN;
    const uint32_t lx = db->lens[2 * p];
    const bool has_y = 2 * p + 1 < n_slots && db->order[2 * p + 1] != 0xFFFFFFFFu;
    const uint32_t ly = has_y ? db->lens[2 * p + 1] : 0;
    const uint8_t *cx = swg_db_codes(db) + db->code_off[2 * p];
    const uint8_t *cy = has_y ? swg_db_codes(db) + db->code_off[2 * p + 1] : nullptr;
    t[0] = kTokReset; // reset rows: padding residue for both sequences
    t[1] = kTokReset | SWG_TOK_RESET2;
    uint32_t *r = t + 2;
    const uint32_t both = std::min(lx, ly); // (= ly: sorted order)
    for (uint32_t j = 0; j < both; ++j) r[j] = (uint32_t)cx[j] | (uint32_t)cy[j] << 8;
    for (uint32_t j = both; j < lx; ++j) r[j] = cx[j];
    const uint64_t blocks = (2ull + lx + 3) / 4;
    for (uint64_t j = 2ull + lx; j < blocks * 4; ++j) t[j] = 0; // rest of the last block: padding rows
    // last row of the pair: X's last residue; for an empty pair the second reset row, so that every
    // pair is finished by the tail lane exactly once
    t[lx + 1] |= kTokLast;
    return blocks;
}

void swg_build_diag_layout(const swg_db *db, uint64_t pair_begin, uint64_t pair_end, uint32_t n_streams,
                           uint32_t streams_per_wg, SwgDiagLayout *L)
{
    const size_t n_pairs = (size_t)(pair_end - pair_begin);
    L->pair_begin = pair_begin;
    L->pair_end = pair_end;
    L->n_streams = n_streams;
    // longest-processing-time-first: pairs are already sorted by length (descending)
    std::vector<uint32_t> owner(n_pairs);
    std::vector<uint64_t> load(n_streams, 0);
    std::vector<uint32_t> count(n_streams, 0);
    {
        typedef std::pair<uint64_t, uint32_t> item; // (blocks so far, stream)
        std::priority_queue<item, std::vector<item>, std::greater<item>> heap;
        for (uint32_t s = 0; s < n_streams; ++s) heap.push(item(0, s));
        // Heap slot h fills up in longest-first order, so slots 0,1,2,.. hold the longest
        // pairs.  Physical stream = lane group of a workgroup: deal the slots round-robin
        // over the workgroups so every CU gets its share of long streams instead of one CU
        // getting all of them.
        const uint32_t spw = std::max<uint32_t>(1, streams_per_wg);
        const uint32_t n_wgs = (n_streams + spw - 1) / spw;
        auto phys = [&](uint32_t h) -> uint32_t {
            const uint32_t s = (h % n_wgs) * spw + (h / n_wgs);
            return s < n_streams ? s : h; // (n_streams is a multiple of spw in practice)
        };
        for (size_t q = 0; q < n_pairs; ++q) {
            const size_t p = pair_begin + q;
            const uint64_t blocks = (2ull + db->lens[2 * p] + 3) / 4;
            item it = heap.top();
            heap.pop();
            const uint32_t s = phys(it.second);
            owner[q] = s;
            load[s] = it.first + blocks;
            count[s]++;
            heap.push(item(it.first + blocks, it.second));
        }
    }
    L->stream_off.assign((size_t)n_streams + 1, 0);
    L->stream_pair_off.assign((size_t)n_streams + 1, 0);
    for (uint32_t s = 0; s < n_streams; ++s) {
        L->stream_off[s + 1] = L->stream_off[s] + load[s];
        L->stream_pair_off[s + 1] = L->stream_pair_off[s] + count[s];
    }
    L->total_blocks = L->stream_off[n_streams];
    L->max_stream_blocks = n_streams ? *std::max_element(load.begin(), load.end()) : 0;
    L->stream_pairs.assign(n_pairs, 0);
    {
        std::vector<uint32_t> fill(n_streams, 0);
        for (size_t q = 0; q < n_pairs; ++q) {
            const uint32_t s = owner[q];
            L->stream_pairs[L->stream_pair_off[s] + fill[s]++] = (uint32_t)(pair_begin + q);
        }
    }
    uint64_t rows_total = 0;
    for (size_t p = pair_begin; p < pair_end; ++p) rows_total += 2ull + db->lens[2 * p];
    L->pair_rows_total = rows_total;
    L->tok.assign(L->total_blocks * 4, 0u);
    uint32_t *base = L->tok.data(); // one 32-bit token per row
#pragma omp parallel for schedule(dynamic, 16) num_threads(swg_host_threads())
    for (long long s = 0; s < (long long)n_streams; ++s) {
        uint32_t *t = base + L->stream_off[s] * 4;
        for (uint32_t i = L->stream_pair_off[s]; i < L->stream_pair_off[s + 1]; ++i)
            t += write_pair_tokens(db, L->stream_pairs[i], t) * 4; // rest of the last block stays padding
    }
}

int swg_build_pair_tokens(const swg_db *db, std::unique_ptr<uint32_t[]> *tok, size_t *tok_dwords,
                          std::vector<uint32_t> *pair_off)
{
    if (tok_dwords) *tok_dwords = 0;
    const uint64_t n_pairs = swg_db_pair_count(db);
    if (n_pairs >= (1ull << 31)) return -1;
    pair_off->assign((size_t)n_pairs + 1, 0u);
    uint64_t total = 0;
    for (uint64_t p = 0; p < n_pairs; ++p) {
        total += (2ull + db->lens[2 * p] + 3) / 4;
        if (total + 1 >= (1ull << 32)) return -1; // block offsets are 32-bit on the device (and one block of zeros follows the last pair)
        (*pair_off)[p + 1] = (uint32_t)total;
    }
    if (!tok) return 0; // offsets only: the tokens themselves are built on the device
    // every pair writes all rows of its blocks, so the buffer needs no zero fill: its pages are
    // first touched by the threads that fill them
    tok->reset(new uint32_t[std::max<size_t>(4, (size_t)total * 4)]);
    *tok_dwords = (size_t)total * 4;
    uint32_t *base = tok->get();
#pragma omp parallel for schedule(dynamic, 64) num_threads(swg_host_threads())
    for (long long p = 0; p < (long long)n_pairs; ++p)
        write_pair_tokens(db, (size_t)p, base + (size_t)(*pair_off)[p] * 4);
    return 0;
}

// Several passes of G*K columns each leave the last one partly empty (3000 columns in 6 passes of 512: 72 of them, 2.3 %
// of the work): it runs the instantiation with the fewest columns per lane that cover what is left.  Returns false when
// there is nothing to gain (one pass; the rest needs all K columns; no instantiation takes the plan's workgroup size).
bool swg_plan_last_pass(const SwgDiagPlan &pl, size_t lq, int *variant, int *K)
{
    if (pl.npass < 2 || pl.G <= 0 || pl.K <= 0 || lq <= (size_t)(pl.npass - 1) * pl.G * pl.K) return false;
    const size_t rest = lq - (size_t)(pl.npass - 1) * pl.G * pl.K;
    const int need = (int)((rest + pl.G - 1) / pl.G);
    int best = -1, bestK = pl.K;
    for (int v = 0; v < swg_num_diag_variants(); ++v) {
        const SwgKernelInfo info = swg_diag_variant_info(v);
        if (info.K >= need && info.K < bestK && pl.W <= info.max_waves) best = v, bestK = info.K;
    }
    if (best < 0) return false;
    *variant = best;
    *K = bestK;
    return true;
}

// How high can a score get (declared in swg_host_internal.h)?  Below SWG_I16_CEILING nothing can saturate the int16
// cells; below SWG_WIDE_CEILING the wide form is exact and nothing needs the int32 re-score; below SWG_F16_CEILING the f16
// cells flag nothing.
SwgScoreBound swg_score_bound(const int8_t *rows, const int8_t *idx, size_t lq, uint64_t longest)
{
    SwgScoreBound r;
    if (idx) // (the table's largest entry: any of its 32 x 32)
        for (int i = 0; i < 32 * 32; ++i) r.smax = std::max<int>(r.smax, rows[i]);
    for (size_t i = 0; i < lq; ++i) {
        const int8_t *row = idx ? rows + 32 * ((uint8_t)idx[i] & 31) : rows + 32 * i;
        int best = 0;
        for (int b = 1; b < 32; ++b) best = std::max<int>(best, row[b]);
        if (!idx) r.smax = std::max(r.smax, best);
        r.qbound += (uint64_t)best;
    }
    r.bound = std::min<uint64_t>(r.qbound, std::min<uint64_t>(lq, longest) * (uint64_t)r.smax);
    return r;
}

extern "C" int swg_debug_score_bound(const int8_t *rows, const int8_t *idx, size_t lq, uint64_t longest, uint64_t *out)
{
    if (!rows || !out) return SWG_ERR_ARG;
    const SwgScoreBound r = swg_score_bound(rows, idx, lq, longest);
    out[0] = r.qbound;
    out[1] = (uint64_t)r.smax;
    out[2] = r.bound;
    return SWG_OK;
}

// Hits-only pruning (declared in swg_host_internal.h).  The table of the bound: for every database residue
// the best it can score against any column of the query, never below 0.  With non-positive gap scores a local alignment
// matches each database residue at most once, at best with its best column, and gaps add nothing positive: a sequence
// scores at most the sum of its residues' entries.  The padding residue 0 scores nothing.
SwgColMax swg_prune_colmax(const int8_t *rows, const int8_t *idx, size_t lq)
{
    SwgColMax cm;
    memset(&cm, 0, sizeof cm);
    bool seen[32] = {false};
    if (idx)
        for (size_t i = 0; i < lq; ++i) seen[(uint8_t)idx[i] & 31] = true;
    const size_t n_rows = idx ? 32 : lq;
    for (size_t i = 0; i < n_rows; ++i) {
        if (idx && !seen[i]) continue;
        const int8_t *row = rows + 32 * i;
        for (int r = 1; r < 32; ++r)
            if (row[r] > (int)cm.v[r]) cm.v[r] = (uint8_t)row[r];
    }
    return cm;
}

uint64_t swg_prune_bound(const SwgColMax &cm, const int8_t *seq, size_t len)
{
    uint64_t u = 0;
    for (size_t j = 0; j < len; ++j) u += cm.v[(uint8_t)seq[j] & 31];
    return u;
}

// test hook: the table (32 bytes) and U of each of the n sequences flat[offsets[i] .. offsets[i+1]) (table indices)
extern "C" int swg_debug_prune_bound(const int8_t *rows, const int8_t *idx, size_t lq, const int8_t *flat, const uint64_t *offsets, size_t n,
                                     uint8_t *colmax_out, uint64_t *u_out)
{
    if (!rows || lq == 0 || (n > 0 && (!flat || !offsets || !u_out))) return SWG_ERR_ARG;
    const SwgColMax cm = swg_prune_colmax(rows, idx, lq);
    if (colmax_out) memcpy(colmax_out, cm.v, 32);
    for (size_t i = 0; i < n; ++i) u_out[i] = swg_prune_bound(cm, flat + offsets[i], (size_t)(offsets[i + 1] - offsets[i]));
    return SWG_OK;
}

// Whether a search is pruned, and how its range is staged.  Pruned: hits only (k > 0 within the device top-K's capacity,
// no score array -- mode 2 prunes with one, skipped sequences then report 0), non-positive gap scores on the 16-bit lane
// groups' work queue, one class, one cell form, not a gapless search and not one query of a batch call.  A range of several
// segments is staged by segment (head_pairs 0).  Mode 1 (auto) prunes such ranges only, and of those the ones with at
// least 4 x prune_head pairs per lane group (under the default segment size every range of several segments is far above
// that; the rule keeps test-sized segments unpruned): their stage order costs nothing but the small kernels between the
// segments.  A range of ONE segment would have to be split into a head and a rest whose launches are list launches
// (one more load per claim, no batch claims); whether that pays has not been measured, so only mode 2 (diagnostic) does
// it: the head is the longest pairs -- at least k sequences and prune_head pairs per resident lane group, but no longer
// than a quarter of the range, so that a database of a few thousand sequences still has a rest to cut.
// A caller's threshold (a.fixed: swg_search_above) takes the structural conditions alone: T stands before the first
// kernel, so every stage is a list launch, no stage is a head, and k, want_scores, n_segments and prune_head decide
// nothing.  Mode 1 (auto) then asks for the range a list launch's cost is small against (swg_prune_above_auto).
SwgPrunePlan swg_prune_plan(const SwgPruneAsk &a)
{
    SwgPrunePlan r;
    if (a.fixed) {
        if (a.mode == 0 || a.gap_open > 0 || a.gap_extend > 0 || a.bits != 16 || !a.use_diag || a.n_classes != 1 || !a.work_queue || a.both_forms ||
            a.gapless || a.batch || a.range_pairs == 0)
            return r;
        if (a.mode == 1 && !swg_prune_above_auto(a.range_pairs, a.groups)) return r;
        r.on = true;
        r.fixed = true;
        return r;
    }
    if (a.mode == 0 || a.k == 0 || a.k > SWG_TOPK_CAND_CAP / 2 || (a.want_scores && a.mode != 2) || a.gap_open > 0 || a.gap_extend > 0 ||
        a.bits != 16 || !a.use_diag || a.n_classes != 1 || !a.work_queue || a.both_forms || a.gapless || a.batch || a.range_pairs == 0 ||
        a.prune_head < 0)
        return r;
    const uint64_t need = ((uint64_t)a.k + 1) / 2, per_group = (uint64_t)a.prune_head * std::max<uint64_t>(1, a.groups);
    if (a.mode == 1 && (a.n_segments <= 1 || a.range_pairs < 4 * per_group)) return r;
    uint64_t head = 0;
    if (a.n_segments <= 1) {
        head = std::max(need, std::min(per_group, a.range_pairs / 4));
        if (head >= a.range_pairs) return r;
    }
    r.on = true;
    r.head_pairs = (uint32_t)head;
    return r;
}

// test hook: in[0..15] = mode, k, want_scores, gap_open, gap_extend, bits, use_diag, n_classes, work_queue, both_forms, gapless,
// batch, range_pairs, groups, prune_head, n_segments; out[0..1] = pruned, head pairs
extern "C" int swg_debug_prune_plan(const int64_t *in, int64_t *out)
{
    if (!in || !out || in[1] < 0 || in[12] < 0 || in[13] < 0 || in[15] < 0) return SWG_ERR_ARG;
    SwgPruneAsk a;
    a.mode = (int)in[0], a.k = (size_t)in[1], a.want_scores = in[2] != 0, a.gap_open = (int)in[3], a.gap_extend = (int)in[4];
    a.bits = (int)in[5], a.use_diag = in[6] != 0, a.n_classes = (int)in[7], a.work_queue = in[8] != 0, a.both_forms = in[9] != 0;
    a.gapless = in[10] != 0, a.batch = in[11] != 0, a.range_pairs = (uint64_t)in[12], a.groups = (uint64_t)in[13], a.prune_head = (long)in[14];
    a.n_segments = (size_t)in[15];
    const SwgPrunePlan r = swg_prune_plan(a);
    out[0] = r.on ? 1 : 0;
    out[1] = (int64_t)r.head_pairs;
    return SWG_OK;
}

// test hook: in[0..11] = mode, gap_open, gap_extend, bits, use_diag, n_classes, work_queue, both_forms, gapless, batch,
// range_pairs, groups; in[12..13] = n_segments, prune_head (read, and without a say); out[0..1] = pruned, head pairs (0)
extern "C" int swg_debug_prune_plan_above(const int64_t *in, int64_t *out)
{
    if (!in || !out || in[10] < 0 || in[11] < 0 || in[12] < 0) return SWG_ERR_ARG;
    SwgPruneAsk a;
    a.fixed = true;
    a.mode = (int)in[0], a.gap_open = (int)in[1], a.gap_extend = (int)in[2], a.bits = (int)in[3], a.use_diag = in[4] != 0, a.n_classes = (int)in[5];
    a.work_queue = in[6] != 0, a.both_forms = in[7] != 0, a.gapless = in[8] != 0, a.batch = in[9] != 0, a.range_pairs = (uint64_t)in[10];
    a.groups = (uint64_t)in[11], a.n_segments = (size_t)in[12], a.prune_head = (long)in[13];
    const SwgPrunePlan r = swg_prune_plan(a);
    out[0] = r.on ? 1 : 0;
    out[1] = (int64_t)r.head_pairs;
    return SWG_OK;
}

// The stages of a pruned fill and what is queued in front of each (swg_host_internal.h has the rules in words).
std::vector<SwgPruneStage> swg_prune_stages(const SwgPrunePlan &plan, const std::vector<std::pair<uint32_t, uint32_t>> &segments)
{
    std::vector<SwgPruneStage> stages;
    for (size_t i = 0; i < segments.size(); ++i) {
        const uint32_t b = segments[i].first, en = segments[i].second;
        const uint32_t mid = segments.size() == 1 && plan.head_pairs > 0 ? std::min(en, b + plan.head_pairs) : en;
        stages.push_back(SwgPruneStage{b, mid, (uint32_t)i, 0u});
        if (mid < en) stages.push_back(SwgPruneStage{mid, en, (uint32_t)i, 0u});
    }
    for (size_t si = 0; si < stages.size(); ++si) {
        if (si == 0 && !plan.fixed) continue; // (nothing to cut by yet)
        uint32_t q = plan.fixed ? 0u : SWG_STAGE_THRESHOLD;
        if (plan.gate && si == (plan.fixed ? 0u : 1u)) q |= SWG_STAGE_BOUND; // (the first stage with a threshold)
        if (plan.prefix_cut) q |= SWG_STAGE_PREFIX_CUT;
        else {
            if (plan.refine[0] && plan.fixed && si == 0 && stages.size() > 1) q |= SWG_STAGE_GATE;
            for (int i = 0; i < SWG_REFINE_LEVELS; ++i)
                if (plan.refine[i]) q |= SWG_REFINE_LEVEL[i].stage_bit;
            q |= SWG_STAGE_LIST;
        }
        stages[si].queued = q;
    }
    return stages;
}

SwgPruneBoundRange swg_prune_bound_range(const std::vector<SwgPruneStage> &stages, uint32_t n_pairs)
{
    for (size_t i = 0; i < stages.size(); ++i)
        if (stages[i].queued & SWG_STAGE_BOUND) return SwgPruneBoundRange{i, stages[i].begin, stages.back().end, stages.front().begin, stages[i].begin};
    return SwgPruneBoundRange{stages.size(), 0u, n_pairs, 0u, 0u};
}

// (head: the words in front of the segments -- 5, 6 with the third level's in[4], 7 with the fourth's in[5] as well, 8
// with the gate's in[6], 9 with the fifth level's in[7])
static int debug_prune_stages(const int64_t *in, int head, int64_t *out, size_t cap, size_t *n_out)
{
    if (!in || !n_out || (cap > 0 && !out) || in[0] < 0 || in[head - 1] < 0) return SWG_ERR_ARG;
    SwgPrunePlan plan;
    plan.on = true;
    plan.head_pairs = (uint32_t)in[0], plan.fixed = in[1] != 0, plan.prefix_cut = in[3] != 0;
    plan.gate = head > 7 && in[6] != 0;
    static const int level_word[SWG_REFINE_LEVELS] = {2, 4, 5, 7}; // (a level's word, where the head reaches past it: the last word is n)
    for (int i = 0; i < SWG_REFINE_LEVELS; ++i) plan.refine[i] = head > level_word[i] + 1 ? (int)in[level_word[i]] : 0;
    std::vector<std::pair<uint32_t, uint32_t>> segments;
    for (int64_t i = 0; i < in[head - 1]; ++i) segments.emplace_back((uint32_t)in[head + 2 * i], (uint32_t)in[head + 1 + 2 * i]);
    const std::vector<SwgPruneStage> stages = swg_prune_stages(plan, segments);
    for (size_t i = 0; i < stages.size() && i < cap; ++i)
        out[4 * i] = stages[i].begin, out[4 * i + 1] = stages[i].end, out[4 * i + 2] = stages[i].segment, out[4 * i + 3] = stages[i].queued;
    *n_out = stages.size();
    return SWG_OK;
}
extern "C" int swg_debug_prune_stages(const int64_t *in, int64_t *out, size_t cap, size_t *n_out) { return debug_prune_stages(in, 5, out, cap, n_out); }
extern "C" int swg_debug_prune_stages3(const int64_t *in, int64_t *out, size_t cap, size_t *n_out) { return debug_prune_stages(in, 6, out, cap, n_out); }
extern "C" int swg_debug_prune_stages4(const int64_t *in, int64_t *out, size_t cap, size_t *n_out) { return debug_prune_stages(in, 7, out, cap, n_out); }
extern "C" int swg_debug_prune_stages5(const int64_t *in, int64_t *out, size_t cap, size_t *n_out) { return debug_prune_stages(in, 8, out, cap, n_out); }
extern "C" int swg_debug_prune_stages6(const int64_t *in, int64_t *out, size_t cap, size_t *n_out) { return debug_prune_stages(in, 9, out, cap, n_out); }

// The k-mer form of the bound, on the host: what the device builds (swg_kmer_cprof_kernel,
// swg_kmer_table_kernel) and sums (swg_pair_bound_kmer_kernel), restated for the tests.  cprof[lq][22]: query column i
// against residue class c -- the residue's own score for classes 1..20, the best of the merged residues for class 21 (the
// local score is monotone in the substitution scores), SWG_KMER_PAD_SCORE for the padding class, which can then be
// neither matched nor crossed for free.
void swg_kmer_cprof(const int8_t *rows, const int8_t *idx, size_t lq, int8_t *cprof)
{
    for (size_t i = 0; i < lq; ++i) {
        const int8_t *row = idx ? rows + 32 * ((uint8_t)idx[i] & 31) : rows + 32 * i;
        int8_t *out = cprof + SWG_KMER_CLASSES * i;
        for (uint32_t c = 0; c < SWG_KMER_CLASSES; ++c) out[c] = SWG_KMER_PAD_SCORE;
        for (uint32_t r = 1; r < 32; ++r) {
            const uint32_t c = swg_kmer_class(r);
            out[c] = std::max(out[c], row[r]);
        }
    }
}

// table[c_1 .. c_k][s] = the best cell of the class block against the query within segment s of its columns (gap
// magnitudes g, e; the recurrence of DESIGN 4.1 in int32; S segments of W = ceil(lq / S) columns, one without columns
// holds 0; S = 1: the block's local score against the whole query).  Blocks that share a prefix share its cells: the block
// runs along the columns, a column is lq cells, and the columns of a prefix are computed once for all the blocks behind it
// (depth first, the first class in parallel), its segment maxima handed down.  Value for value what the device's
// one-thread-per-block walk along the query gives.
// one row of a class block: class c behind the row (Mp, Bp) of its prefix (none: the block's first row), the segment maxima
// best_p of the prefix handed down
static void kmer_row(const int8_t *cprof, size_t lq, int g, int e, size_t S, uint32_t c, const int *Mp, const int *Bp, const int *best_p, int *Mn,
                     int *Bn, int *best)
{
    const size_t W = (lq + S - 1) / S;
    int a = 0, up = 0;
    for (size_t s = 0; s < S; ++s) best[s] = best_p ? best_p[s] : 0;
    for (size_t s = 0, i = 0; i < lq; ++s) {
        int bs = best[s];
        for (const size_t end = std::min(lq, i + W); i < end; ++i) {
            const int sc = cprof[SWG_KMER_CLASSES * i + c];
            a = std::max(std::max(up - g, a - e), 0);
            const int b = Mp ? std::max(std::max(Mp[i] - g, Bp[i] - e), 0) : 0;
            const int diag = Mp && i ? Mp[i - 1] : 0;
            const int m = std::max(std::max(diag + sc, a), b);
            Mn[i] = m, Bn[i] = b, up = m;
            bs = std::max(bs, m);
        }
        best[s] = bs;
    }
}

static void kmer_extend(const int8_t *cprof, size_t lq, int g, int e, int k, size_t S, int depth, size_t prefix, const int *Mp, const int *Bp,
                        const int *best_p, std::vector<int> &work, uint16_t *table, uint32_t c_begin, uint32_t c_end)
{
    int *Mn = work.data() + (size_t)depth * (2 * lq + S), *Bn = Mn + lq, *best = Bn + lq;
    for (uint32_t c = c_begin; c < c_end; ++c) {
        kmer_row(cprof, lq, g, e, S, c, depth ? Mp : nullptr, Bp, best_p, Mn, Bn, best);
        const size_t at = prefix * SWG_KMER_CLASSES + c;
        if (depth + 1 == k)
            for (size_t s = 0; s < S; ++s) table[at * S + s] = (uint16_t)std::min(best[s], 65535);
        else kmer_extend(cprof, lq, g, e, k, S, depth + 1, at, Mn, Bn, best, work, table, 0, SWG_KMER_CLASSES);
    }
}

void swg_kmer_table_seg(const int8_t *cprof, size_t lq, int g, int e, int k, size_t S, uint16_t *table)
{
    g = std::min(g, 65536), e = std::min(e, 65536);
#pragma omp parallel for schedule(dynamic, 1)
    for (int c = 0; c < (int)SWG_KMER_CLASSES; ++c) {
        std::vector<int> work((size_t)k * (2 * lq + S));
        kmer_extend(cprof, lq, g, e, k, S, 0, 0, nullptr, nullptr, nullptr, work, table, (uint32_t)c, (uint32_t)c + 1u);
    }
}

// U_{k,S} of one sequence as the device sums it: the sequence's token rows -- two reset rows (padding), its
// residues (a 0 among them is a padding row: the shorter sequence of a pair, filled up to the longer one's length),
// padding to a whole 4-row token block -- in blocks of 4 rows (k = 4), or in blocks of 5 over every whole 20 rows and of 4
// over the rest (k = 5).  A block counts its table entry, or the sum of its rows' colmax entries where that is less: the
// entry of a block with residues of class 21 is taken under the best scores of all of them, and may exceed what these
// residues can reach.  The blocks are taken in order over the table's S segments: the segment that holds a block's last
// matched column never decreases along the sequence, so with H[s] the best total of the blocks so far whose last one ended
// in segment s, a block gives H[s] = max_{s' <= s} H[s'] + min(table[block][s], the block's colmax sum), and the bound is
// max_s H[s].  S = 1 is the unordered sum of the blocks.
// (entries(ix): the S entries of block ix)
// (each(ix, sum): a block's index in the table of k and the colmax sum of its rows, in the sequence's order)
template <class Each>
static void kmer_blocks(Each each, int k, const SwgColMax &cm, const int8_t *seq, size_t len)
{
    const size_t n_blocks = (2 + len + 3) / 4, n_rows = 4 * n_blocks;
    auto res = [&](size_t row) -> uint32_t { return row < 2 || row >= 2 + len ? 0u : (uint8_t)seq[row - 2] & 31u; };
    const size_t rows5 = k == 5 ? 20 * (n_blocks / 5) : 0;
    for (size_t r = 0; r < n_rows;) {
        const size_t rows = r < rows5 ? 5 : 4;
        size_t ix = 0;
        uint64_t sum = 0;
        for (size_t j = 0; j < rows; ++j) ix = ix * SWG_KMER_CLASSES + swg_kmer_class(res(r + j)), sum += cm.v[res(r + j)];
        if (k == 5 && rows == 4) ix *= SWG_KMER_CLASSES;
        each(ix, sum);
        r += rows;
    }
}

template <class Entries>
static uint64_t kmer_bound_walk(Entries entries, int k, size_t S, const SwgColMax &cm, const int8_t *seq, size_t len)
{
    std::vector<uint64_t> H(S, 0);
    kmer_blocks(
        [&](size_t ix, uint64_t sum) {
            const uint16_t *t = entries(ix);
            uint64_t run = 0;
            for (size_t s = 0; s < S; ++s) {
                run = std::max(run, H[s]);
                H[s] = run + std::min<uint64_t>(t[s], sum);
            }
        },
        k, cm, seq, len);
    return *std::max_element(H.begin(), H.end());
}

uint64_t swg_kmer_bound_seg(const uint16_t *table, int k, size_t S, const SwgColMax &cm, const int8_t *seq, size_t len)
{
    return kmer_bound_walk([&](size_t ix) { return table + ix * S; }, k, S, cm, seq, len);
}

// The body of the three mirror hooks below, each of which admits its own (k, S): the table (22^k x S uint16, or NULL) and
// U_{k,S} of each of the n sequences flat[offsets[i] .. offsets[i+1]), under the gap scores of swg_set_scoring
static int debug_prune_kmer(bool admitted, const int8_t *rows, const int8_t *idx, size_t lq, int gap_open, int gap_extend, int k, int S,
                            const int8_t *flat, const uint64_t *offsets, size_t n, uint16_t *table_out, uint64_t *u_out)
{
    if (!admitted || !rows || lq == 0 || gap_open > 0 || gap_extend > 0 || (n > 0 && (!flat || !offsets || !u_out))) return SWG_ERR_ARG;
    std::vector<int8_t> cprof(lq * SWG_KMER_CLASSES);
    swg_kmer_cprof(rows, idx, lq, cprof.data());
    std::vector<uint16_t> own;
    if (!table_out) {
        own.resize(swg_kmer_entries(k) * (size_t)S);
        table_out = own.data();
    }
    swg_kmer_table_seg(cprof.data(), lq, -(gap_open + gap_extend), -gap_extend, k, (size_t)S, table_out);
    const SwgColMax cm = swg_prune_colmax(rows, idx, lq);
    for (size_t i = 0; i < n; ++i) u_out[i] = swg_kmer_bound_seg(table_out, k, (size_t)S, cm, flat + offsets[i], (size_t)(offsets[i + 1] - offsets[i]));
    return SWG_OK;
}
// test hooks: the unsegmented bound of k = 4 or 5; over S = 1..32 segments; and the second level's -- k = 4 with the
// segments the refine kernel walks: 32 (the first level's widest), 64 or 128
extern "C" int swg_debug_prune_kmer(const int8_t *rows, const int8_t *idx, size_t lq, int gap_open, int gap_extend, int k, const int8_t *flat,
                                    const uint64_t *offsets, size_t n, uint16_t *table_out, uint64_t *u_out)
{
    return debug_prune_kmer(k == 4 || k == 5, rows, idx, lq, gap_open, gap_extend, k, 1, flat, offsets, n, table_out, u_out);
}
extern "C" int swg_debug_prune_kmer_seg(const int8_t *rows, const int8_t *idx, size_t lq, int gap_open, int gap_extend, int k, int S,
                                        const int8_t *flat, const uint64_t *offsets, size_t n, uint16_t *table_out, uint64_t *u_out)
{
    return debug_prune_kmer((k == 4 || k == 5) && S >= 1 && S <= (int)SWG_KMER_MAX_SEGMENTS, rows, idx, lq, gap_open, gap_extend, k, S, flat, offsets, n,
                            table_out, u_out);
}
extern "C" int swg_debug_prune_kmer_refine(const int8_t *rows, const int8_t *idx, size_t lq, int gap_open, int gap_extend, int S2, const int8_t *flat,
                                           const uint64_t *offsets, size_t n, uint16_t *table_out, uint64_t *u_out)
{
    return debug_prune_kmer(S2 == 32 || S2 == 64 || S2 == 128, rows, idx, lq, gap_open, gap_extend, 4, S2, flat, offsets, n, table_out, u_out);
}
// ... and the third level's: k = 4 over the 256 segments swg_pair_bound_refine_kernel<4, 8> walks.  The tables of all
// these hooks are uint16_t whatever width the device keeps: the values are the same (swg_kmer_table_bits).
extern "C" int swg_debug_prune_kmer_refine3(const int8_t *rows, const int8_t *idx, size_t lq, int gap_open, int gap_extend, int S3, const int8_t *flat,
                                            const uint64_t *offsets, size_t n, uint16_t *table_out, uint64_t *u_out)
{
    return debug_prune_kmer(S3 == 256, rows, idx, lq, gap_open, gap_extend, 4, S3, flat, offsets, n, table_out, u_out);
}
// ... and the fourth level's: k = 5 over the 128 or 256 segments swg_pair_bound_refine_kernel<5, PL> walks, blocked as
// swg_kmer_bound_seg blocks k = 5.  The table of (5, 256) is 22^5 x 256 entries, so there is none here: the sequences are
// taken in batches of up to SWG_REFINE4_BATCH blocks, and a batch computes the entries of the blocks it holds -- sorted, so
// that blocks behind one prefix share its rows the way the table's build shares them.
#define SWG_REFINE4_BATCH 32768u
// (the first sequence of each batch, and n)
static std::vector<size_t> blocks5_batches(const uint64_t *offsets, size_t n)
{
    std::vector<size_t> batch{0};
    for (size_t i = 0, blocks = 0; i < n; ++i) {
        const size_t nb = (2 + (size_t)(offsets[i + 1] - offsets[i]) + 3) / 4;
        if (blocks > 0 && blocks + nb > SWG_REFINE4_BATCH) batch.push_back(i), blocks = 0;
        blocks += nb;
    }
    batch.push_back(n);
    return batch;
}
// (the blocks of 5 the sequences [first, last) hold, sorted, each once)
static std::vector<uint32_t> blocks5_held(const SwgColMax &cm, const int8_t *flat, const uint64_t *offsets, size_t first, size_t last)
{
    std::vector<uint32_t> held;
    for (size_t i = first; i < last; ++i)
        kmer_blocks([&](size_t ix, uint64_t) { held.push_back((uint32_t)ix); }, 5, cm, flat + offsets[i], (size_t)(offsets[i + 1] - offsets[i]));
    std::sort(held.begin(), held.end());
    held.erase(std::unique(held.begin(), held.end()), held.end());
    return held;
}
// (their S entries each, by the row recurrence `row`: kmer_row, or kmer_row2 of the fifth level)
template <class Row>
static std::vector<uint16_t> blocks5_entries(Row row, const std::vector<uint32_t> &held, const int8_t *cprof, size_t lq, int g, int e, size_t S)
{
    const uint32_t C = SWG_KMER_CLASSES;
    std::vector<uint16_t> entries(held.size() * S);
    std::vector<int> work(5 * (2 * lq + S));
    uint32_t prev[5] = {0, 0, 0, 0, 0};
    for (size_t h = 0; h < held.size(); ++h) {
        uint32_t c[5];
        for (uint32_t j = 5, v = held[h]; j-- > 0; v /= C) c[j] = v % C;
        int d = 0;
        while (h > 0 && d < 4 && c[d] == prev[d]) ++d; // (the rows above d are the previous block's)
        for (; d < 5; ++d) {
            int *Mn = work.data() + (size_t)d * (2 * lq + S), *Mp = d ? Mn - (2 * lq + S) : nullptr;
            row(cprof, lq, g, e, S, c[d], Mp, Mp ? Mp + lq : nullptr, Mp ? Mp + 2 * lq : nullptr, Mn, Mn + lq, Mn + 2 * lq);
            prev[d] = c[d];
        }
        const int *best = work.data() + 4 * (2 * lq + S) + 2 * lq;
        for (size_t s = 0; s < S; ++s) entries[h * S + s] = (uint16_t)std::min(best[s], 65535);
    }
    return entries;
}
extern "C" int swg_debug_prune_kmer_refine4(const int8_t *rows, const int8_t *idx, size_t lq, int gap_open, int gap_extend, int S4, const int8_t *flat,
                                            const uint64_t *offsets, size_t n, uint64_t *u_out)
{
    if ((S4 != 128 && S4 != 256) || !rows || lq == 0 || gap_open > 0 || gap_extend > 0 || (n > 0 && (!flat || !offsets || !u_out))) return SWG_ERR_ARG;
    const size_t S = (size_t)S4, C = SWG_KMER_CLASSES;
    std::vector<int8_t> cprof(lq * C);
    swg_kmer_cprof(rows, idx, lq, cprof.data());
    const SwgColMax cm = swg_prune_colmax(rows, idx, lq);
    const int g = std::min(-(gap_open + gap_extend), 65536), e = std::min(-gap_extend, 65536);
    const std::vector<size_t> batch = blocks5_batches(offsets, n);
#pragma omp parallel for schedule(dynamic, 1)
    for (long bi = 0; bi < (long)batch.size() - 1; ++bi) {
        const std::vector<uint32_t> held = blocks5_held(cm, flat, offsets, batch[bi], batch[bi + 1]);
        const std::vector<uint16_t> entries = blocks5_entries(kmer_row, held, cprof.data(), lq, g, e, S);
        for (size_t i = batch[bi]; i < batch[bi + 1]; ++i)
            u_out[i] = kmer_bound_walk(
                [&](size_t ix) { return entries.data() + (size_t)(std::lower_bound(held.begin(), held.end(), (uint32_t)ix) - held.begin()) * S; }, 5, S, cm,
                flat + offsets[i], (size_t)(offsets[i + 1] - offsets[i]));
    }
    return SWG_OK;
}

// The fifth level: the fourth level's blocks, segments and walk, with the query columns a chain jumps over
// between two blocks charged as the gap they are.  A second entry per block and segment, T2 = the best of score + e x span
// over the block's chains whose LAST MATCH lies in the segment (span: last matched column - first matched column), by the
// table's recurrence with the credit e paid per column a chain advances: a diagonal step that continues a chain earns e,
// opening a gap along the query costs g - e and extending it nothing, gaps along the block are unchanged, a chain starts at a
// match without credit, and "no chain" is SWG_KMER_NO_CHAIN, not 0.  Only cells that end in a match enter a segment's
// maximum (the state of a gap along the query no longer decays).
static void kmer_row2(const int8_t *cprof, size_t lq, int g, int e, size_t S, uint32_t c, const int *Mp, const int *Bp, const int *best_p, int *Mn,
                      int *Bn, int *best)
{
    const size_t W = (lq + S - 1) / S;
    int a = SWG_KMER_NO_CHAIN, up = SWG_KMER_NO_CHAIN;
    for (size_t s = 0; s < S; ++s) best[s] = best_p ? best_p[s] : 0;
    for (size_t s = 0, i = 0; i < lq; ++s) {
        int bs = best[s];
        for (const size_t end = std::min(lq, i + W); i < end; ++i) {
            const int sc = cprof[SWG_KMER_CLASSES * i + c];
            a = std::max(std::max(up - (g - e), a), SWG_KMER_NO_CHAIN);
            const int b = Mp ? std::max(std::max(Mp[i] - g, Bp[i] - e), SWG_KMER_NO_CHAIN) : SWG_KMER_NO_CHAIN;
            const int diag = Mp && i ? Mp[i - 1] : SWG_KMER_NO_CHAIN;
            const int h = sc + std::max(0, diag + e);
            const int m = std::max(std::max(h, a), b);
            Mn[i] = m, Bn[i] = b, up = m;
            bs = std::max(bs, h);
        }
        best[s] = bs;
    }
}

// The walk.  H[s]: the best total of the blocks so far over the chains whose last block ended in segment s (a running
// maximum: a block may be left out).  A block with entries t, t2 and colmax sum `sum`, tm[s] = min(t[s], sum), gives
//   H'[s] = max( H[s],  max_{s'' in {s, s - 1}} H[s''] + tm[s],  max_{n = 1..N} H[s - 1 - n] + min(tm[s], t2[s] - e W n),
//                min( tm[s] + max_{s'' < s - 1 - N} H[s''],  t2[s] - e W (s - 1) + max_{s'' < s - 1 - N} (H[s''] + e W s'') ) )
// -- n = s - s'' - 1 whole segments lie between the two chains' ends, e W n is the least their columns cost, the first N are
// taken one by one and the rest by two prefix maxima (the least of two maxima is at least the maximum of the leasts).  Every
// term is at most the fourth level's H[s''] + tm[s].  N >= S: the exact form.
static uint64_t kmer_bound_walk5(const uint16_t *t, const uint16_t *t2, const std::vector<uint32_t> &held, size_t S, size_t W, int e, size_t N,
                                 const SwgColMax &cm, const int8_t *seq, size_t len)
{
    const int64_t c = (int64_t)e * (int64_t)W;
    std::vector<int64_t> H(S, 0), Hn(S), PH(S), PC(S);
    kmer_blocks(
        [&](size_t ix, uint64_t sum) {
            const size_t at = (size_t)(std::lower_bound(held.begin(), held.end(), (uint32_t)ix) - held.begin()) * S;
            for (size_t s = 0; s < S; ++s) {
                PH[s] = std::max(s ? PH[s - 1] : 0, H[s]);
                PC[s] = std::max(s ? PC[s - 1] : INT64_MIN, H[s] + c * (int64_t)s);
            }
            for (size_t s = 0; s < S; ++s) {
                const int64_t tm = (int64_t)std::min<uint64_t>(t[at + s], sum), v2 = t2[at + s];
                int64_t best = std::max(H[s], std::max(H[s], s ? H[s - 1] : 0) + tm);
                for (size_t n = 1; n <= N && n + 1 <= s; ++n) best = std::max(best, H[s - 1 - n] + std::min(tm, v2 - c * (int64_t)n));
                if (s >= N + 2) best = std::max(best, std::min(tm + PH[s - 2 - N], v2 - c * (int64_t)(s - 1) + PC[s - 2 - N]));
                Hn[s] = best;
            }
            H.swap(Hn);
        },
        5, cm, seq, len);
    return (uint64_t)*std::max_element(H.begin(), H.end());
}

// ... and the fifth level's mirror: like the fourth's it holds no table and computes batch by batch.  It is on (*on_out = 1)
// where e > 0 and both kinds of entry are bytes -- 5 x (the largest colmax entry + e) <= 255 (swg_kmer_refine5_admitted) --;
// elsewhere the level is off, *on_out = 0 and u_out is not written.  n_explicit: N of the walk, 0 for the device's
// (SWG_REFINE5_EXPLICIT).
extern "C" int swg_debug_prune_kmer_refine5(const int8_t *rows, const int8_t *idx, size_t lq, int gap_open, int gap_extend, int S5, int n_explicit,
                                            const int8_t *flat, const uint64_t *offsets, size_t n, uint64_t *u_out, int *on_out)
{
    if (S5 != 256 || n_explicit < 0 || !rows || lq == 0 || gap_open > 0 || gap_extend > 0 || !on_out || (n > 0 && (!flat || !offsets || !u_out)))
        return SWG_ERR_ARG;
    const size_t S = (size_t)S5, C = SWG_KMER_CLASSES, W = (lq + S - 1) / S;
    const SwgColMax cm = swg_prune_colmax(rows, idx, lq);
    const int g = std::min(-(gap_open + gap_extend), 65536), e = std::min(-gap_extend, 65536);
    *on_out = swg_kmer_refine5_admitted(cm, e, lq) ? 1 : 0;
    if (!*on_out) return SWG_OK;
    std::vector<int8_t> cprof(lq * C);
    swg_kmer_cprof(rows, idx, lq, cprof.data());
    const std::vector<size_t> batch = blocks5_batches(offsets, n);
#pragma omp parallel for schedule(dynamic, 1)
    for (long bi = 0; bi < (long)batch.size() - 1; ++bi) {
        const std::vector<uint32_t> held = blocks5_held(cm, flat, offsets, batch[bi], batch[bi + 1]);
        const std::vector<uint16_t> t = blocks5_entries(kmer_row, held, cprof.data(), lq, g, e, S);
        const std::vector<uint16_t> t2 = blocks5_entries(kmer_row2, held, cprof.data(), lq, g, e, S);
        for (size_t i = batch[bi]; i < batch[bi + 1]; ++i)
            u_out[i] = kmer_bound_walk5(t.data(), t2.data(), held, S, W, e, n_explicit ? (size_t)n_explicit : (size_t)SWG_REFINE5_EXPLICIT, cm,
                                        flat + offsets[i], (size_t)(offsets[i + 1] - offsets[i]));
    }
    return SWG_OK;
}
extern "C" int swg_debug_prune_table_bits(const int8_t *rows, const int8_t *idx, size_t lq, int k)
{
    if (!rows || lq == 0 || (k != 4 && k != 5)) return SWG_ERR_ARG;
    return swg_kmer_table_bits(swg_prune_colmax(rows, idx, lq), k);
}

// Which bound a pruned search cuts by: k = 1 (colmax), 4 or 5 (k-mer tables) and the S segments of its table (1: the
// unordered sum).  An unpruned search builds nothing (0).  A forced k is taken as it is wherever the search is pruned, with
// the forced S, or unsegmented when that is left automatic; a forced S alone goes with the k the unsegmented candidates
// give, stepped down to 4 where the table of (5, S) is beyond SWG_KMER_TABLE_BUDGET.  Automatic weighs, over the fixed
// list SWG_KMER_CANDIDATES, what a candidate costs -- its table, swg_kmer_table_cells(k) * lq cells at table_rate cells per second paid by
// every search with a new query, and its bound kernel's time per pair row beyond the colmax kernel's -- against what its
// tighter cut saves: the share of the range's pair rows it takes off the fill (the hard case, a database of unrelated
// sequences) at fill_rate pair rows per second for this query.  In the order of what they save, a step up
// must cost at most half of what it saves.
struct SwgKmerCandidate {
    int k, S;
    double gain;      // the headline's rows kept at (1, 1), 0.5584, less the candidate's (profiles/prune_segments_ab.txt)
    double bound_row; // seconds per pair row that a step spends outside the fill's rows, beyond what it spends there at (1, 1)
};
static const SwgKmerCandidate SWG_KMER_CANDIDATES[] = {
    {1, 1, 0.0, 0.0},         {4, 1, 0.1426, 3.1e-12},  {5, 1, 0.2006, 3.1e-12},
    {4, 16, 0.2493, 4.0e-12}, {4, 32, 0.2741, 6.1e-12}, {5, 8, 0.2760, 9.0e-12},
};
int swg_prune_kmer_choice(const SwgKmerAsk &a, int *segments)
{
    int S_out = 1;
    int k = 0;
    if (a.pruned) {
        const bool forced_k = a.forced == 1 || a.forced == 4 || a.forced == 5;
        const long forced_S = a.forced_segments >= 1 && a.forced_segments <= (long)SWG_KMER_MAX_SEGMENTS ? a.forced_segments : 0;
        if (forced_k) {
            k = (int)a.forced;
            S_out = k > 1 && forced_S ? (int)forced_S : 1;
        } else if (a.table_rate <= 0 || a.fill_rate <= 0 || a.lq == 0) {
            k = 1;
        } else {
            auto cost = [&](const SwgKmerCandidate &c) {
                return c.k == 1 ? 0.0 : swg_kmer_table_cells(c.k) * (double)a.lq / a.table_rate + c.bound_row * (double)a.pair_rows;
            };
            auto gain = [&](const SwgKmerCandidate &c) { return c.gain * (double)a.pair_rows / a.fill_rate; };
            const SwgKmerCandidate *cur = &SWG_KMER_CANDIDATES[0];
            for (const SwgKmerCandidate &c : SWG_KMER_CANDIDATES) {
                if (forced_S && c.S != 1) continue; // (a forced S: k from the unsegmented candidates)
                if (c.gain > cur->gain && cost(c) - cost(*cur) <= 0.5 * (gain(c) - gain(*cur))) cur = &c;
            }
            k = cur->k, S_out = cur->S;
            if (forced_S && k > 1) {
                if (k == 5 && !swg_kmer_table_admitted(5, forced_S)) k = 4;
                S_out = (int)forced_S;
            }
        }
    }
    if (segments) *segments = k > 1 ? S_out : (k ? 1 : 0);
    return k;
}

// The questions of the three choice hooks below: in[0..5] = forced (option "prune_kmer"), pruned, lq, pair rows, table cells
// per second, fill pair rows per second (0, 0: the library's own rates for this lq), then in[6] = the forced segments
// (option "prune_segments") and in[7] = the forced refinement (option "prune_refine") where the hook has them (n_in words)
static bool debug_kmer_ask(const int64_t *in, int64_t *out, int n_in, SwgKmerAsk *a)
{
    if (!in || !out) return false;
    for (int i = 2; i < std::min(n_in, 7); ++i)
        if (in[i] < 0) return false;
    if (n_in > 7 && !swg_refine_value_ok(0, (long)in[7])) return false;
    a->forced = (long)in[0], a->pruned = in[1] != 0, a->lq = (size_t)in[2], a->pair_rows = (uint64_t)in[3];
    a->table_rate = in[4] ? (double)in[4] : SWG_KMER_TABLE_RATE;
    a->fill_rate = in[5] ? (double)in[5] : swg_kmer_fill_rate(a->lq);
    a->forced_segments = n_in > 6 ? (long)in[6] : 1;
    a->forced_refine[0] = n_in > 7 ? (long)in[7] : 0;
    return true;
}
// test hook: out[0] = k.  Like swg_debug_prune_kmer and swg_debug_prune_kmer_read it keeps its unsegmented meaning: the k
// of "prune_segments" = 1.
extern "C" int swg_debug_prune_kmer_choice(const int64_t *in, int64_t *out)
{
    SwgKmerAsk a;
    if (!debug_kmer_ask(in, out, 6, &a)) return SWG_ERR_ARG;
    out[0] = swg_prune_kmer_choice(a);
    return SWG_OK;
}
// ... with the forced segments: out[0..3] = k, S, the table's bytes, whether a context builds it (1) or refuses it as
// beyond its budget (0)
extern "C" int swg_debug_prune_kmer_choice_seg(const int64_t *in, int64_t *out)
{
    SwgKmerAsk a;
    if (!debug_kmer_ask(in, out, 7, &a)) return SWG_ERR_ARG;
    int S = 0;
    out[0] = swg_prune_kmer_choice(a, &S);
    out[1] = S;
    out[2] = (int64_t)(swg_kmer_entries((int)out[0]) * (uint64_t)S * sizeof(uint16_t));
    out[3] = out[0] <= 1 || swg_kmer_table_admitted((int)out[0], S) ? 1 : 0;
    return SWG_OK;
}

// The automatic rule of a level behind the first, in the style of SWG_KMER_CANDIDATES: over the level's candidates (the
// segments its option can force, in the order of what they save: SWG_REFINE_LEVEL has the shares, the seconds and where
// they were measured), what a candidate costs -- its table, swg_kmer_table_cells(k) * lq cells at table_rate cells per
// second like a first-level table of that k, and its walk's seconds per pair row of the range (it walks the pairs of the
// cut stages whose earlier bounds reach T) -- against what its tighter cut saves: the share of the range's pair rows it
// takes off the fill at fill_rate pair rows per second.  A step up must cost at most half of what it saves.  -> the
// segments of the candidate the range pays for, or 0: none.
static int refine_level_pays(const SwgKmerAsk &a, const SwgRefineLevel &L)
{
    if (a.table_rate <= 0 || a.fill_rate <= 0 || a.lq == 0) return 0;
    const double cost = swg_kmer_table_cells(L.k) * (double)a.lq / a.table_rate + L.bound_row * (double)a.pair_rows;
    int S = 0;
    double cur_share = 0.0, cur_cost = 0.0, cur_gain = 0.0;
    for (const SwgRefineLevel::Forced &c : L.forced) {
        const double gain = c.gain * (double)a.pair_rows / a.fill_rate;
        if (c.gain > cur_share && cost - cur_cost <= 0.5 * (gain - cur_gain)) S = c.segments, cur_share = c.gain, cur_cost = cost, cur_gain = gain;
    }
    return S;
}

// The chain, in level order.  Whoever asks, a level whose table holds blocks of 5 needs that table as bytes (16-bit
// entries are refused at this size: swg_kmer_refine4_admitted), and the fifth e > 0 and second entries that are bytes
// (a.refine5_ok).  Forced by its option a level is taken behind whatever the other levels are; "off" is off.  Automatic
// only where no level or first-level option in front of it was forced (a forced "prune_kmer" or "prune_segments" leaves
// d_pair_bound the mirror of exactly that bound; every forced earlier level stays without the later ones), behind a
// predecessor that took what the level was measured behind, and where refine_level_pays.
void swg_prune_refine_choices(const SwgKmerAsk &a, int k, int S, int out[SWG_REFINE_LEVELS])
{
    std::fill(out, out + SWG_REFINE_LEVELS, 0);
    if (!a.pruned || k < 1) return;
    for (int i = 0; i < SWG_REFINE_LEVELS; ++i) {
        const SwgRefineLevel &L = SWG_REFINE_LEVEL[i];
        if (L.k == 5 && !swg_kmer_refine4_admitted(a.table_bits5)) continue;
        if (i == 3 && !a.refine5_ok) continue;
        if (a.forced_refine[i] != 0) {
            out[i] = swg_refine_forced_segments(i, a.forced_refine[i]); // (0 for "off")
            continue;
        }
        bool forced_in_front = a.forced != 0 || a.forced_segments != 0;
        for (int j = 0; j < i; ++j) forced_in_front = forced_in_front || a.forced_refine[j] != 0;
        if (forced_in_front) continue;
        bool behind = false;
        switch (i) {
        case 0: // the second level: an automatic first level that took a segmented k = 4 candidate
            behind = k == 4 && S > 1;
            break;
        case 1: // the third: the second took 128, and the k = 4 tables are byte-wide (the 256-segment table is then the 60 MB
                // the 128-segment one is as uint16_t, and a lane's 8 entries one 8-byte load)
            behind = out[0] == 128 && a.table_bits == 8;
            break;
        case 2: // the fourth: the third took 256 (so the tables of k = 4 are bytes, as those of k = 5 are)
            behind = out[1] == 256;
            break;
        case 3: // the fifth: the fourth was taken, and the threshold is the K-th best so far -- under a caller's what the level
                // saves depends on where T lies among the bounds (profiles/prune_adjacent_ab.txt, section 4: 23.6 ms saved at
                // the score of the 100th hit, 3.3 ms lost at twice that), so there it runs only where it is forced
            behind = out[2] != 0 && !a.fixed;
            break;
        }
        if (behind) out[i] = refine_level_pays(a, L);
    }
}

// The gate in front of the first level (swg_host_internal.h has the rule in words).  Nothing smaller than the headline
// was measured (profiles/prune_gate_ab.txt): the automatic rule keeps the third level's floor, about 2e8 pair rows at
// 3000 columns, below which a stage's fill no longer hides the one launch moved behind the first stage.
bool swg_prune_gate_choice(const SwgKmerAsk &a, int k, int S)
{
    if (!a.pruned || k <= 1 || S <= 1 || a.forced_gate == 1) return false;
    if (a.forced_gate == 2) return true;
    if (a.forced != 0 || a.forced_segments != 0) return false;
    return refine_level_pays(a, SWG_REFINE_LEVEL[1]) != 0;
}

extern "C" int swg_debug_prune_gate_choice(const int64_t *in, int64_t *out)
{
    SwgKmerAsk a;
    if (!debug_kmer_ask(in, out, 8, &a)) return SWG_ERR_ARG;
    if (!swg_prune_gate_value_ok((long)in[8])) return SWG_ERR_ARG;
    a.forced_gate = (long)in[8];
    int S = 0;
    out[0] = swg_prune_kmer_choice(a, &S);
    out[1] = S;
    out[2] = swg_prune_gate_choice(a, (int)out[0], S) ? 1 : 0;
    return SWG_OK;
}

// test hooks: the chain up to its n_levels-th level (swg_host_internal.h has the words of in): in[0..7] the first level's
// question and option "prune_refine"; then, where the hook has them, in[8] "prune_refine3" and in[9] the width of the k = 4
// tables' entries (0: bytes); in[10] "prune_refine4" and in[11] the width of the k = 5 tables'; in[12] "prune_refine5",
// in[13] whether the query and scoring admit the fifth level, in[14] whether the threshold is a caller's
// -> out[0..1 + n_levels] = k, S, then the segments of the levels
static int debug_prune_refine_choices(const int64_t *in, int n_levels, int64_t *out)
{
    SwgKmerAsk a;
    if (!debug_kmer_ask(in, out, 8, &a)) return SWG_ERR_ARG;
    static const int option_word[SWG_REFINE_LEVELS] = {7, 8, 10, 12};
    auto width_ok = [](int64_t w) { return w == 0 || w == 8 || w == 16; };
    for (int i = 1; i < n_levels; ++i) {
        if (!swg_refine_value_ok(i, (long)in[option_word[i]])) return SWG_ERR_ARG;
        a.forced_refine[i] = (long)in[option_word[i]];
    }
    if (n_levels >= 2) {
        if (!width_ok(in[9])) return SWG_ERR_ARG;
        a.table_bits = in[9] == 16 ? 16 : 8;
    }
    if (n_levels >= 3) {
        if (!width_ok(in[11])) return SWG_ERR_ARG;
        a.table_bits5 = in[11] == 16 ? 16 : 8;
    }
    if (n_levels >= 4) {
        if ((in[13] != 0 && in[13] != 1) || (in[14] != 0 && in[14] != 1)) return SWG_ERR_ARG;
        a.refine5_ok = in[13] != 0, a.fixed = in[14] != 0;
    }
    int S = 0, levels[SWG_REFINE_LEVELS];
    out[0] = swg_prune_kmer_choice(a, &S);
    out[1] = S;
    swg_prune_refine_choices(a, (int)out[0], S, levels);
    std::copy(levels, levels + n_levels, out + 2);
    return SWG_OK;
}
extern "C" int swg_debug_prune_refine_choice(const int64_t *in, int64_t *out) { return debug_prune_refine_choices(in, 1, out); }
extern "C" int swg_debug_prune_refine3_choice(const int64_t *in, int64_t *out) { return debug_prune_refine_choices(in, 2, out); }
extern "C" int swg_debug_prune_refine4_choice(const int64_t *in, int64_t *out) { return debug_prune_refine_choices(in, 3, out); }
extern "C" int swg_debug_prune_refine5_choice(const int64_t *in, int64_t *out) { return debug_prune_refine_choices(in, 4, out); }

// Both 16-bit forms in one search (plan_search in swg_api.cpp): the length from which a sequence can reach the f16 cells' ceiling
// as an exact copy of a stretch of the query -- such a copy scores qbound / lq per row on average, qbound being the
// query's best possible total --, and where that length cuts the sorted pair order (kept per database and length).
uint32_t swg_split_rows(size_t lq, uint64_t qbound)
{
    if (qbound == 0) return 0u;
    return (uint32_t)std::min<uint64_t>(((uint64_t)SWG_F16_CEILING * lq + qbound - 1) / qbound, 1u << 30);
}

void swg_db_split_at(swg_db *db, uint32_t rows)
{
    if (db->split_rows == rows) return;
    const size_t n = db->lens.size();
    const size_t first_short = (size_t)(std::partition_point(db->lens.begin(), db->lens.end(), [rows](uint32_t l) { return l >= rows; }) -
                                        db->lens.begin());
    db->split_rows = rows;
    db->split_pair = (uint32_t)((first_short + 1) / 2); // (a pair with one long member is a long pair)
    uint64_t sum = 0;
    for (size_t i = std::min(n, (size_t)db->split_pair * 2); i < n; ++i) sum += db->lens[i];
    db->split_residues = sum;
}

// Test hook (not part of the public ABI): the both-forms cut of a packed database for a query of lq columns whose best
// possible total is qbound.  out[0..2] = rows, first pair of the f16 part, residues of the f16 part.
extern "C" int swg_debug_split(swg_db *db, size_t lq, uint64_t qbound, uint64_t *out)
{
    if (!db || !out || lq == 0 || qbound == 0) return SWG_ERR_ARG;
    const uint32_t rows = swg_split_rows(lq, qbound);
    swg_db_split_at(db, rows);
    out[0] = rows;
    out[1] = db->split_pair;
    out[2] = db->split_residues;
    return SWG_OK;
}

// What the systolic engine (swg_fill_kernel: lane l owns sequences 2l, 2l+1 of a 128-sequence bin, W wavefronts of a
// workgroup chained over the query, int16 cells) would need for this database, by the host's bin table: a bin costs its
// LONGEST member's rows (rounded to 4-row blocks) on every one of the W wavefronts, 10 K + 12 instructions per row, plus
// ~5 000 cycles per bin and wavefront for taking it off the work counter; and the search cannot end before the longest
// bin's chain has, at the rate of a wavefront that shares its SIMD.  Calibrated on 2 M peptides (round 4,
// profiles/r04_peptides_systolic.txt: lq 128 K 32 x 4 wavefronts 1.15 ms measured / 1.21 estimated, lq 30 K 16 x 2 0.37 /
// 0.33) and on config 2, where the 5 000-row bin's chain is the whole search (11.8 ms measured, 11 estimated).
// Returns the estimate in ms and the columns per wavefront of the best single-pass instantiation (0: none).
double swg_systolic_estimate_ms(const swg_db *db, size_t lq, int n_cu, int *best_K, bool f16)
{
    *best_K = 0;
    if (db->n_bins == 0 || db->bin_nblk.size() != db->n_bins) return 1e300;
    uint64_t blocks = 0;
    for (uint32_t b : db->bin_nblk) blocks += b;
    const double rows = 4.0 * (double)blocks, longest = 4.0 * (double)db->max_nblk;
    double best = 1e300;
    for (int v = 0; v < swg_num_variants(16); ++v) {
        const SwgKernelInfo info = swg_variant_info(16, v);
        const int W = (int)((lq + (size_t)info.K - 1) / (size_t)info.K);
        if (W > info.max_waves) continue; // (several passes: never the better engine)
        if (info.K > 32) continue;         // (the 48-column instantiation runs at two wavefronts per SIMD: measured 45 % over its count)
        const size_t lds = info.lds_per_wave * (size_t)W + info.lds_fixed;
        const int per_cu = swg_workgroups_per_cu(info.max_waves, W, lds);
        const double waves_per_simd = std::max(1.0, per_cu * W / 4.0);
        const double instr = (f16 ? 8.5 : 10.0) * info.K + 12.0; // (packed-f16 cells where no score can reach 4096)
        const double thr = (rows * W * instr * 4.06 + (double)db->n_bins * W * 5000.0) / (4.0 * n_cu);
        // bins are whole work units of a workgroup: with few bins per workgroup the search lasts as many ROUNDS as the
        // busiest workgroup has bins -- the first of them the longest bin (bins go out longest first), the others about
        // average -- at the rate of a wavefront that shares its SIMD (300 000 sequences of ~250 residues, lq 64: 2 344
        // bins on 1 536 workgroups are two rounds, 0.97 ms measured where the throughput term alone says 0.58)
        const double wps = std::min(4.0, waves_per_simd);
        const double n_wgs = std::max(1.0, (double)n_cu * per_cu);
        const double rounds = std::ceil((double)db->n_bins / n_wgs);
        const double quant = (longest + (rounds - 1.0) * rows / (double)db->n_bins) * instr * 4.06 * wps;
        const double chain = std::max(longest * instr * 4.06 * wps, quant);
        // (the 24-column instantiation measures 30 % over its count -- peptides lq 128: 1.48 ms against 1.05 for 8 x 16 columns --
        // and is only picked where that still wins)
        const double ms = std::max(thr, chain) / 2.4e6 * (info.K == 24 ? 1.3 : 1.0);
        if (ms < best) best = ms, *best_K = info.K;
    }
    return best;
}

// The planner's estimate for the lane groups was fitted on BASELINE's length distribution (pairs of ~380 rows), where
// about 40 % of a wavefront's steps find one of its 64 lanes on a flagged row (a pair's two reset rows and its last row)
// and take the rare branch; its cost there is inside the fitted intercept.  A database of SHORT pairs takes that branch
// on nearly every step: 19 instructions more per wavefront-row than the fit knows, scaled by how much more often
// (peptides: K = 8, 98 fitted instructions per row, measured 1.56 ms where the unadjusted estimate says 1.41).  Used where
// the two engines are compared, not in the ranking of geometries (the term is the same for all of them).
double swg_diag_short_pair_factor(const swg_db *db, const SwgDiagPlan &pl, int form)
{
    const uint64_t n_pairs = swg_db_pair_count(db);
    if (n_pairs == 0) return 1.0;
    uint64_t longest = 0;
    const double L = std::max(4.0, (double)swg_db_pair_rows(db, 0, n_pairs, &longest) / (double)n_pairs);
    auto p_flag = [](double rows) { return 1.0 - std::pow(std::max(0.0, 1.0 - 3.0 / rows), 64.0); };
    const double extra = 19.0 * std::max(0.0, p_flag(L) - p_flag(380.0));
    return 1.0 + extra / instr_per_row(pl.K, pl.G, form, form == 2 && pl.fma);
}

// test hook: both engines' estimates for a database and a query length (cells: 0 int16, 2 packed f16), without a device:
// out[0] lane groups (us), out[1] systolic (us), out[2] its columns per wavefront, out[3] 1 = the model picks the systolic engine
extern "C" int swg_debug_engine(const swg_db *db, size_t lq, int n_cu, int form, int32_t *out)
{
    if (!db || !out || lq == 0 || n_cu <= 0) return SWG_ERR_ARG;
    SwgDiagWork wk;
    try {
        if (swg_plan_diag_work(db, lq, n_cu, 0, 0, 0, 0, true, true, &wk, 1.0, form) <= 0) return SWG_ERR_ARG;
    } catch (const std::exception &) {
        return SWG_ERR_NOMEM;
    }
    int K = 0;
    // (the hook has no scoring system: the f16 cells are assumed where BLOSUM62's largest entry, 11, keeps every score below 4096)
    const bool f16 = form == 2 && (uint64_t)db->max_nblk * SWG_ROWS_PER_BLK * 11ull < 4096ull;
    const double sys = swg_systolic_estimate_ms(db, lq, n_cu, &K, f16);
    const double diag = wk.plan[0].est_ms * swg_diag_short_pair_factor(db, wk.plan[0], form);
    out[0] = (int32_t)(diag * 1e3);
    out[1] = K > 0 ? (int32_t)std::min(sys * 1e3, 2.0e9) : -1;
    out[2] = K;
    out[3] = K > 0 && sys < SWG_SYSTOLIC_MARGIN * diag ? 1 : 0;
    return SWG_OK;
}

// Test hook (not part of the public ABI, declared in swg_host_internal.h): the cost model's first choice
// for a packed database and a query length on a device of n_cu compute units, without a device.
// out[0..12] = classes, K, G, W, passes, workgroups, long pairs, long K, long G, long W, long workgroups,
// estimated microseconds, columns per lane of the last pass (0: as the other passes).
static int debug_plan(const swg_db *db, size_t lq, int n_cu, int form, long f16_pair, int32_t *out)
{
    if (!db || !out || lq == 0 || n_cu <= 0 || f16_pair < 0 || f16_pair > 2) return SWG_ERR_ARG;
    SwgDiagWork wk;
    try {
        if (swg_plan_diag_work(db, lq, n_cu, 0, 0, 0, 0, true, true, &wk, 1.0, form, f16_pair) <= 0) return SWG_ERR_ARG;
    } catch (const std::exception &) {
        return SWG_ERR_NOMEM;
    }
    const SwgDiagPlan &b = wk.plan[0], &l = wk.plan[1];
    const bool two = wk.n_classes == 2;
    int last_variant = -1, last_K = 0;
    if (two || !swg_plan_last_pass(b, lq, &last_variant, &last_K)) last_K = 0;
    const int32_t v[13] = {wk.n_classes, b.K, b.G, b.W, b.npass, b.workgroups, two ? (int32_t)(wk.pair_end[1] - wk.pair_begin[1]) : 0,
                           two ? l.K : 0, two ? l.G : 0, two ? l.W : 0, two ? l.workgroups : 0, (int32_t)(b.est_ms * 1e3), last_K};
    memcpy(out, v, sizeof v);
    if (form == 2) {
        out[13] = b.fma;
        out[14] = (int32_t)swg_diag_dyn_lds_bytes(b.K, b.G, b.W, b.fma != 0);
        out[15] = two ? l.fma : 0;
    }
    return SWG_OK;
}

extern "C" int swg_debug_plan(const swg_db *db, size_t lq, int n_cu, int32_t *out) { return debug_plan(db, lq, n_cu, 0, 0, out); }

// Test hook: what a gapless search (swg_search_gapless) of a packed database would plan for a query of lq columns with
// default options, without a device.  out[0..4] = route (1: the gapless cells; 0: the gapped machinery with the gaps
// priced out), K, lanes per group, wavefronts per workgroup, workgroups (route 0: the int16 planner's first choice).
extern "C" int swg_debug_plan_gapless(const swg_db *db, size_t lq, int n_cu, int32_t *out)
{
    if (!db || !out || lq == 0 || n_cu <= 0) return SWG_ERR_ARG;
    SwgDiagWork wk;
    int route = 0;
    try {
        route = !db->tokens_only && lq <= 64u * 32u && swg_plan_diag_work(db, lq, n_cu, 0, 0, 0, 0, true, true, &wk, 1.0, 3, 1) > 0 ? 1 : 0;
        if (!route && swg_plan_diag_work(db, lq, n_cu, 0, 0, 0, 0, true, true, &wk, 1.0, 0, 0) <= 0) return SWG_ERR_ARG;
    } catch (const std::exception &) {
        return SWG_ERR_NOMEM;
    }
    const SwgDiagPlan &b = wk.plan[0];
    const int32_t v[6] = {route, b.K, b.G, b.W, b.workgroups, b.npass};
    memcpy(out, v, sizeof v);
    return SWG_OK;
}

extern "C" int swg_debug_plan_f16(const swg_db *db, size_t lq, int n_cu, long f16_pair, int32_t *out)
{
    return debug_plan(db, lq, n_cu, 2, f16_pair, out);
}

// Test hook: the planner's answer for a forced geometry, as a search with options cols_per_wave, group_lanes, max_waves,
// long_split = -1, f16_pair and last_pass asks it (plan_search in swg_api.cpp).  No plan: SWG_OK and out all zero.
extern "C" int swg_debug_plan_forced(const swg_db *db, size_t lq, int n_cu, long cols, long group, long waves, int form,
                                     long f16_pair, int last_pass, int32_t *out)
{
    if (!db || !out || lq == 0 || n_cu <= 0 || (form != 0 && form != 2 && form != 3) || f16_pair < 0 || f16_pair > 2 || cols < 0 ||
        group < 0 || waves < 0)
        return SWG_ERR_ARG;
    memset(out, 0, 16 * sizeof(int32_t));
    SwgDiagWork wk;
    try {
        if (swg_plan_diag_work(db, lq, n_cu, cols, group, waves, -1, true, true, &wk, 1.0, form, form == 3 ? 1 : f16_pair) <= 0) return SWG_OK;
    } catch (const std::exception &) {
        return SWG_ERR_NOMEM;
    }
    const SwgDiagPlan &b = wk.plan[0];
    int last_variant = -1, last_K = 0;
    if (!last_pass || wk.n_classes != 1 || !swg_plan_last_pass(b, lq, &last_variant, &last_K)) last_K = 0;
    const bool fma = form == 2 && b.fma != 0;
    const int32_t v[16] = {wk.n_classes, b.K, b.G, b.W, b.npass, b.workgroups, 0, 0, 0, 0, 0, (int32_t)(b.est_ms * 1e3), last_K,
                           fma ? 1 : 0, (int32_t)swg_diag_dyn_lds_bytes(b.K, b.G, b.W, fma), 0};
    memcpy(out, v, sizeof v);
    return SWG_OK;
}

// The launch log (test hook, swg_internal.h): which instantiation each launcher of a fill kernel was asked for.  Host-side
// bookkeeping: off by default, bounded, and nothing of what is launched depends on it.
static std::mutex g_launch_log_mutex;
static std::atomic<bool> g_launch_log_on{false};
static size_t g_launch_log_seen = 0;
static std::vector<int32_t> g_launch_log;

void swg_launch_log_add(int family, int K, int G, int W, int form, bool edges, bool flag, int workgroups, int grid_rows, bool list)
{
    if (!g_launch_log_on.load(std::memory_order_relaxed)) return;
    std::lock_guard<std::mutex> lock(g_launch_log_mutex);
    if (g_launch_log_seen++ >= SWG_LAUNCH_LOG_CAP) return;
    const int32_t r[SWG_LAUNCH_LOG_FIELDS] = {family, K, G, W, form, edges ? 1 : 0, flag ? 1 : 0, workgroups, grid_rows, list ? 1 : 0};
    g_launch_log.insert(g_launch_log.end(), r, r + SWG_LAUNCH_LOG_FIELDS);
}

extern "C" void swg_debug_launch_log(int on)
{
    std::lock_guard<std::mutex> lock(g_launch_log_mutex);
    g_launch_log_on = on != 0;
    g_launch_log_seen = 0;
    g_launch_log.clear();
    if (on) g_launch_log.reserve((size_t)SWG_LAUNCH_LOG_CAP * SWG_LAUNCH_LOG_FIELDS); // (the launchers never allocate)
}

extern "C" size_t swg_debug_launch_log_read(int32_t *out, size_t cap)
{
    std::lock_guard<std::mutex> lock(g_launch_log_mutex);
    const size_t held = g_launch_log.size() / SWG_LAUNCH_LOG_FIELDS, n = std::min(held, cap);
    if (out && n > 0) memcpy(out, g_launch_log.data(), n * SWG_LAUNCH_LOG_FIELDS * sizeof(int32_t));
    return g_launch_log_seen;
}
