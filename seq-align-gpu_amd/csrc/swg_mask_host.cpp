// swg_mask_host.cpp -- the host half of low-complexity masking (include/swg.h; no GPU needed): the integers of
// the rule (swg_mask_tables), the host twin of the device kernels (swg_seg_mask: also what masks a query), and
// swg_db_sequence, which reads one sequence back out of a database's host image.
#include "swg_host_internal.h"
#include "../../include/swg_host.h"

#include <cmath>
#include <cstring>
#include <exception>
#include <vector>

extern "C" void swg_mask_params_default(swg_mask_params *p)
{
    if (!p) return;
    p->window = SWG_MASK_WINDOW_DEFAULT;
    p->replace = SWG_MASK_REPLACE_DEFAULT;
    p->trigger = SWG_MASK_TRIGGER_DEFAULT;
    p->extend = SWG_MASK_EXTEND_DEFAULT;
}

extern "C" int swg_mask_tables(const swg_mask_params *p, int32_t T[65], int64_t *thr_trigger, int64_t *thr_extend)
{
    swg_mask_params d;
    swg_mask_params_default(&d);
    if (!p) p = &d;
    if (!T || !thr_trigger || !thr_extend) return swg_set_global_error(SWG_ERR_ARG, "swg_mask_tables: NULL argument");
    if (p->window < 4 || p->window > 64) return swg_set_global_error(SWG_ERR_ARG, "mask: window %d outside 4..64", (int)p->window);
    if (p->replace < 1 || p->replace > 31) return swg_set_global_error(SWG_ERR_ARG, "mask: replace %d outside 1..31", (int)p->replace);
    if (!std::isfinite(p->trigger) || !std::isfinite(p->extend) || p->trigger < 0.0 || p->trigger > p->extend)
        return swg_set_global_error(SWG_ERR_ARG, "mask: trigger %g and extend %g must satisfy 0 <= trigger <= extend", p->trigger, p->extend);
    const int W = p->window;
    memset(T, 0, 65 * sizeof(int32_t));
    for (int c = 1; c <= W; ++c) T[c] = (int32_t)std::rint((double)c * std::log2((double)c) * 65536.0);
    // (an entropy bound beyond log2 W holds for every window: the threshold is then not positive, and S >= 0 always)
    *thr_trigger = (int64_t)std::ceil((double)W * (std::log2((double)W) - p->trigger) * 65536.0);
    *thr_extend = (int64_t)std::ceil((double)W * (std::log2((double)W) - p->extend) * 65536.0);
    return SWG_OK;
}

// The twin: the weights by sliding (as the kernel slides them), the runs and the widening position by position.
static int seg_mask_impl(const int8_t *idx, size_t len, const swg_mask_params *p, uint8_t *mask_out, size_t *n_masked, size_t *n_segments)
{
    if (n_masked) *n_masked = 0;
    if (n_segments) *n_segments = 0;
    int32_t T[65];
    int64_t thr1, thr2;
    const int rc = swg_mask_tables(p, T, &thr1, &thr2);
    if (rc != SWG_OK) return rc;
    if (!idx && len > 0) return swg_set_global_error(SWG_ERR_ARG, "swg_seg_mask: NULL sequence");
    const size_t W = (size_t)(p ? p->window : SWG_MASK_WINDOW_DEFAULT);
    if (mask_out && len) memset(mask_out, 0, len);
    if (len < W) return SWG_OK;
    for (size_t i = 0; i < len; ++i)
        if (idx[i] < 0 || idx[i] > 31) return swg_set_global_error(SWG_ERR_RESIDUE, "swg_seg_mask: residue index outside 0..31 at position %zu", i);
    const size_t nw = len - W + 1;
    int cnt[32] = {0};
    int64_t S = 0;
    for (size_t j = 0; j < W; ++j) {
        const int c = cnt[idx[j]]++;
        S += T[c + 1] - T[c];
    }
    size_t masked = 0, segments = 0;
    size_t run_begin = 0, covered = 0; // covered: positions below it are decided
    bool in_run = false, run_kept = false;
    auto close_run = [&](size_t end) { // the run's starts are [run_begin, end)
        if (!run_kept) return;
        ++segments;
        const size_t a = std::max(run_begin, covered), b = end - 1 + W;
        for (size_t i = a; i < b; ++i) {
            if (mask_out) mask_out[i] = 1;
            ++masked;
        }
        covered = std::max(covered, b);
    };
    for (size_t s = 0; s < nw; ++s) {
        if (S >= thr2) {
            if (!in_run) in_run = true, run_kept = false, run_begin = s;
            run_kept = run_kept || S >= thr1;
        } else if (in_run) {
            close_run(s);
            in_run = false;
        }
        if (s + 1 < nw) {
            const int out = --cnt[idx[s]];
            S -= T[out + 1] - T[out];
            const int in = cnt[idx[s + W]]++;
            S += T[in + 1] - T[in];
        }
    }
    if (in_run) close_run(nw);
    if (n_masked) *n_masked = masked;
    if (n_segments) *n_segments = segments;
    return SWG_OK;
}

extern "C" int swg_seg_mask_segments(const int8_t *idx, size_t len, const swg_mask_params *p, uint8_t *mask_out, size_t *n_masked,
                                     size_t *n_segments)
{
    return seg_mask_impl(idx, len, p, mask_out, n_masked, n_segments);
}

extern "C" int swg_seg_mask(const int8_t *idx, size_t len, const swg_mask_params *p, uint8_t *mask_out, size_t *n_masked)
{
    return seg_mask_impl(idx, len, p, mask_out, n_masked, nullptr);
}

// The slot of an original index is found by a walk over the order: the database is const here, and the table that maps
// indices to slots (slot_of) is built only under a view's lock.
extern "C" int swg_db_sequence(const swg_db *db, uint32_t original_index, int8_t *idx_out, size_t cap, size_t *len)
{
    if (len) *len = 0;
    if (!db || !len) return swg_set_global_error(SWG_ERR_ARG, "swg_db_sequence: NULL argument");
    if (db->tokens_only) return swg_set_global_error(SWG_ERR_STATE, "swg_db_sequence: a database built from 16-lane batches has no residue bytes");
    if (original_index >= db->n_total)
        return swg_set_global_error(SWG_ERR_ARG, "swg_db_sequence: index %u is outside the database of %zu sequences", original_index, db->n_total);
    size_t slot = db->order.size();
    for (size_t s = 0; s < db->order.size(); ++s)
        if (db->order[s] == original_index) {
            slot = s;
            break;
        }
    if (slot == db->order.size())
        return swg_set_global_error(SWG_ERR_ARG, "swg_db_sequence: sequence %u is not held by this shard or view", original_index);
    const size_t n = db->lens[slot];
    *len = n;
    if (n > cap || (n > 0 && !idx_out)) return swg_set_global_error(SWG_ERR_ARG, "swg_db_sequence: room for %zu residues, the sequence has %zu", cap, n);
    const uint8_t *cd = swg_db_codes(db) + db->code_off[slot];
    for (size_t j = 0; j < n; ++j) idx_out[j] = (int8_t)(cd[j] >> 3);
    return SWG_OK;
}

// The twin over a whole database laid end to end (flat / offsets as swg_db_pack takes them), in place: what a caller
// without swg_db_mask does before swg_db_pack (tools/sweeps/db_mask_ab.py measures it).  totals: NULL or
// {residues_masked, sequences_masked, segments}.
extern "C" int swg_seg_mask_flat(int8_t *flat, const uint64_t *offsets, size_t n, const swg_mask_params *p, uint64_t totals[3])
{
    swg_mask_params d;
    swg_mask_params_default(&d);
    if (!p) p = &d;
    int32_t T[65];
    int64_t t1, t2;
    int rc = swg_mask_tables(p, T, &t1, &t2);
    if (rc != SWG_OK) return rc;
    if (n > 0 && (!flat || !offsets)) return swg_set_global_error(SWG_ERR_ARG, "swg_seg_mask_flat: NULL argument");
    unsigned long long res = 0, seqs = 0, segs = 0;
    int bad = 0; // 1: a residue outside 0..31, 2: out of memory (no exception leaves the parallel region)
#pragma omp parallel num_threads(swg_host_threads()) reduction(+ : res, seqs, segs) reduction(| : bad)
    {
        std::vector<uint8_t> m;
#pragma omp for schedule(dynamic, 256)
        for (long long i = 0; i < (long long)n; ++i) {
            const size_t len = (size_t)(offsets[i + 1] - offsets[i]);
            try {
                m.resize(len);
            } catch (const std::exception &) {
                bad |= 2;
                continue;
            }
            size_t nm = 0, ns = 0;
            if (seg_mask_impl(flat + offsets[i], len, p, m.data(), &nm, &ns) != SWG_OK) {
                bad |= 1;
                continue;
            }
            if (nm) {
                int8_t *s = flat + offsets[i];
                for (size_t j = 0; j < len; ++j)
                    if (m[j]) s[j] = (int8_t)p->replace;
            }
            res += nm, seqs += nm != 0, segs += ns;
        }
    }
    if (bad & 2) return swg_set_global_error(SWG_ERR_NOMEM, "swg_seg_mask_flat: out of memory");
    if (bad) return swg_set_global_error(SWG_ERR_RESIDUE, "swg_seg_mask_flat: residue index outside 0..31");
    if (totals) totals[0] = res, totals[1] = seqs, totals[2] = segs;
    return SWG_OK;
}
