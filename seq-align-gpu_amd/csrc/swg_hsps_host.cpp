// swg_hsps_host.cpp -- the host twin of swg_align_hsps* (include/swg.h; no GPU needed): the rule for one pair
// in plain C++, row by row over the whole matrix, as swg_seg_mask and swg_pssm_from_paths are twins of their kernels.
#include "swg_host_internal.h"

#include <cstring>
#include <exception>
#include <vector>

namespace {
const int32_t kUsed = -(1 << 29); // the H state of a used cell: never a maximum against 0, no overflow under a gap score

inline uint32_t pick(int32_t m, int32_t x, int32_t y) { return m == 0 ? 0u : x == m ? 1u : y == m ? 2u : 3u; }

int hsps_host(const int8_t sub[32][32], int gap_open, int gap_extend, const int8_t *query, const int8_t *pssm, size_t lq, const int8_t *seq,
              size_t len, uint32_t max_hsps, int32_t min_score, swg_alignment *out, swg_align_counts *counts, char *ops, size_t ops_stride,
              uint32_t *n_out)
{
    const int go = gap_open + gap_extend, ge = gap_extend;
    const size_t w = lq + 1;
    std::vector<uint8_t> ident(lq); // what identity is counted against: the residues, or a PSSM's consensus
    for (size_t i = 0; i < lq; ++i) {
        if (query) {
            ident[i] = (uint8_t)query[i];
            continue;
        }
        int at = 1;
        for (int b = 2; b < 32; ++b)
            if (pssm[i * 32 + b] > pssm[i * 32 + at]) at = b;
        ident[i] = (uint8_t)at;
    }
    std::vector<uint8_t> dir(lq * len), used(lq * len, 0);
    std::vector<int32_t> rows(6 * w);
    std::vector<char> path(lq + len + 1);
    for (uint32_t r = 0; r < max_hsps; ++r) {
        std::fill(rows.begin(), rows.end(), 0);
        int32_t best = 0;
        size_t bj = 0, bi = 0;
        for (size_t j = 1; j <= len; ++j) {
            // row j - 1 and row j of H, A, B; column 0 of both stays 0
            const int32_t *H1 = &rows[((j - 1) & 1) * 3 * w], *A1 = H1 + w, *B1 = A1 + w;
            int32_t *H0 = &rows[(j & 1) * 3 * w], *A0 = H0 + w, *B0 = A0 + w;
            for (size_t i = 1; i <= lq; ++i) {
                const int32_t s = query ? sub[query[i - 1]][seq[j - 1]] : pssm[(i - 1) * 32 + seq[j - 1]];
                const int32_t hd = H1[i - 1], ad = A1[i - 1], bd = B1[i - 1];
                const int32_t mh = std::max(std::max(hd, ad), std::max(bd, 0));
                const int32_t xa = H1[i] + go, ya = A1[i] + ge, za = B1[i] + go;
                const int32_t ma = std::max(std::max(xa, ya), std::max(za, 0));
                const int32_t xb = H0[i - 1] + go, yb = A0[i - 1] + go, zb = B0[i - 1] + ge;
                const int32_t mb = std::max(std::max(xb, yb), std::max(zb, 0));
                const size_t cell = (j - 1) * lq + (i - 1);
                dir[cell] = (uint8_t)(pick(mh, hd, ad) | pick(ma, xa, ya) << 2 | pick(mb, xb, yb) << 4);
                const int32_t h = used[cell] ? kUsed : mh + s;
                H0[i] = h, A0[i] = ma, B0[i] = mb;
                if (h > best) best = h, bj = j, bi = i; // row by row: the smallest database position, then query position
            }
        }
        if (best < min_score) break;
        swg_alignment a = {};
        uint32_t n = 0, same = 0, runs = 0;
        size_t j = bj, i = bi;
        a.score = best, a.q_end = (uint32_t)i, a.d_end = (uint32_t)j;
        uint32_t state = 1;
        char later = 0;
        while (j > 0 && i > 0 && n < lq + len) {
            const size_t cell = (j - 1) * lq + (i - 1);
            const uint32_t c = dir[cell];
            uint32_t from;
            char op;
            if (state == 1) {
                used[cell] = 1;
                same += ident[i - 1] == (uint8_t)seq[j - 1];
                op = 'M', from = c & 3, --j, --i;
            } else if (state == 2) op = 'I', from = (c >> 2) & 3, --j;
            else op = 'D', from = (c >> 4) & 3, --i;
            runs += op != 'M' && op != later;
            path[n++] = later = op;
            if (from == 0) break;
            state = from;
        }
        a.q_begin = (uint32_t)i, a.d_begin = (uint32_t)j, a.n_ops = n;
        if (ops && (size_t)n + 1 > ops_stride)
            return swg_set_global_error(SWG_ERR_ARG, "swg_align_hsps_host: ops_stride %zu too small for a path of %u steps", ops_stride, n);
        out[r] = a;
        if (counts) {
            swg_align_counts &c = counts[r];
            c.n_ident = same, c.n_gap_open = runs;
            c.n_match = (a.q_end - a.q_begin) + (a.d_end - a.d_begin) - n;
            c.n_gap = n - c.n_match;
        }
        if (ops) {
            char *o = ops + r * ops_stride;
            for (uint32_t k = 0; k < n; ++k) o[k] = path[n - 1 - k];
            o[n] = 0;
        }
        *n_out = r + 1;
    }
    return SWG_OK;
}
} // namespace

extern "C" int swg_align_hsps_host(const int8_t sub[32][32], int gap_open, int gap_extend, const int8_t *query, const int8_t *pssm, size_t lq,
                                   const int8_t *seq, size_t len, uint32_t max_hsps, int32_t min_score, swg_alignment *out,
                                   swg_align_counts *counts, char *ops, size_t ops_stride, uint32_t *n_out)
{
    const char *fn = "swg_align_hsps_host";
    if (n_out) *n_out = 0;
    if (max_hsps < 1 || max_hsps > SWG_MAX_HSPS) return swg_set_global_error(SWG_ERR_ARG, "%s: max_hsps %u outside 1..%d", fn, max_hsps, SWG_MAX_HSPS);
    if (min_score < 1) return swg_set_global_error(SWG_ERR_ARG, "%s: min_score %d below 1", fn, min_score);
    if (!out || !n_out || !seq || (!query) == (!pssm) || (query && !sub))
        return swg_set_global_error(SWG_ERR_ARG, "%s: NULL argument (one of query and pssm, and the table with a query)", fn);
    if (lq == 0 || len == 0 || (uint64_t)lq * len > (1ull << 30))
        return swg_set_global_error(SWG_ERR_ARG, "%s: pair (%zu x %zu) is empty or above 2^30 cells", fn, lq, len);
    if (ops && ops_stride == 0) return swg_set_global_error(SWG_ERR_ARG, "%s: ops_stride is 0", fn);
    for (size_t i = 0; i < lq && query; ++i)
        if (query[i] < 1 || query[i] > 31) return swg_set_global_error(SWG_ERR_RESIDUE, "%s: residue index %d in the query outside 1..31", fn, query[i]);
    for (size_t j = 0; j < len; ++j)
        if (seq[j] < 0 || seq[j] > 31) return swg_set_global_error(SWG_ERR_RESIDUE, "%s: residue index %d in the sequence outside 0..31", fn, seq[j]);
    try {
        return hsps_host(sub, gap_open, gap_extend, query, pssm, lq, seq, len, max_hsps, min_score, out, counts, ops, ops_stride, n_out);
    } catch (const std::exception &) {
        return swg_set_global_error(SWG_ERR_NOMEM, "%s: out of host memory", fn);
    }
}
