// swg_comp_host.cpp -- the host half of the composition-based score adjustment (include/swg.h): the count
// table of a query, lambda_std, and the twin of the device's kernels for one pair (swg_comp_adjust_host), which is also
// the route of the pairs the fill kernel cannot hold.  Host only: nothing here touches a GPU.
#if defined(__GNUC__) && !defined(__clang__)
#pragma GCC optimize("fp-contract=off") // no fused multiply-add: the device's iterates (swg_comp_rule.h)
#endif
#include "swg_host_internal.h"
#include "../../include/swg_host.h"
#include "swg_comp_rule.h"

#include <cmath>
#include <cstring>
#include <new>
#include <vector>

int swg_pssm_background(const char *fn, const double *freq, double P[32], uint32_t *mask); // swg_pssm_host.cpp

void swg_comp_counts(const int8_t sub[32][32], const int8_t *query, const int8_t *pssm, size_t lq, uint32_t *C)
{
    memset(C, 0, 32 * 256 * sizeof(uint32_t));
    for (size_t p = 0; p < lq; ++p) {
        const int8_t *row = pssm ? pssm + p * 32 : sub[(int)query[p]];
        for (int a = 0; a < 32; ++a) ++C[a * 256 + (int)row[a] + 128];
    }
}

// lambda of 256 weights by score + 128, bins ascending: 0, 1 (does not exist) or 2 (did not converge)
static int comp_lambda(const double w[256], double W, double *lambda)
{
    double mean = 0.0;
    int smax = -129;
    for (int s = 0; s < 256; ++s) {
        if (!(w[s] > 0.0)) continue;
        mean += (double)(s - 128) * w[s];
        smax = s - 128;
    }
    *lambda = 0.0;
    if (!(mean < 0.0) || smax <= 0) return 1;
    int iters;
    double lam = 0.0;
    const int st = swg_comp_solve(
        [&](double l, double *f, double *df) {
            double s0 = 0.0, s1 = 0.0;
            for (int s = 0; s < 256; ++s) {
                if (!(w[s] > 0.0)) continue;
                const double e = w[s] * std::exp(l * (double)(s - 128));
                s0 += e;
                s1 += (double)(s - 128) * e;
            }
            *f = s0, *df = s1;
        },
        W, smax, &lam, &iters);
    if (st == 0) *lambda = lam;
    return st;
}

int swg_comp_lambda_std(const uint32_t *C, const double P[32], uint32_t mask, double *lambda)
{
    double w[256], W = 0.0;
    for (int s = 0; s < 256; ++s) {
        double v = 0.0;
        for (int a = 1; a < 32; ++a)
            if (mask >> a & 1u) v += P[a] * (double)C[a * 256 + s];
        w[s] = v;
        W += v;
    }
    return comp_lambda(w, W, lambda);
}

// The recurrence of the library (src/alignment.c:124-161 as swg_bounds_kernel keeps it), score only: per column the
// diagonal reduction D of the row above and the vertical one V, the left one carried along the row.
static int32_t comp_fill(const int8_t sub[32][32], const int8_t *query, const int8_t *pssm, size_t lq, const int8_t *seq, size_t len,
                         const int16_t T[256], int go, int ge)
{
    const int32_t edge = std::max(std::max(go, ge), 0);
    std::vector<int32_t> D(lq + 1, 0), V(lq + 1, edge);
    int32_t best = 0;
    for (size_t j = 0; j < len; ++j) {
        const int d = seq[j];
        int32_t diag = 0, left = edge; // column 0 is the border
        for (size_t i = 1; i <= lq; ++i) {
            const int s = T[(pssm ? (int)pssm[(i - 1) * 32 + d] : (int)sub[(int)query[i - 1]][d]) + 128];
            const int32_t H = diag + s, A = V[i], B = left;
            diag = D[i];
            D[i] = std::max(std::max(std::max(H, A), B), 0);
            V[i] = std::max(std::max(std::max(H + go, A + ge), B + go), 0);
            left = std::max(std::max(std::max(H + go, A + go), B + ge), 0);
            best = std::max(best, H);
        }
    }
    return best;
}

void swg_comp_pair(const int8_t sub[32][32], int go, int ge, const int8_t *query, const int8_t *pssm, size_t lq, const uint32_t *C,
                   uint32_t mask, double lambda_std, int std_status, const int8_t *seq, size_t len, int F, swg_comp_result *out)
{
    uint64_t c[32] = {}, n = 0;
    for (size_t j = 0; j < len; ++j) ++c[seq[j] & 31];
    for (int a = 1; a < 32; ++a) n += (mask >> a & 1u) ? c[a] : 0;
    swg_comp_result r = {0, 0, 65536u, 1, 0.0};
    if (n > 0 && std_status == 0) {
        double w[256];
        for (int s = 0; s < 256; ++s) {
            uint64_t h = 0;
            for (int a = 1; a < 32; ++a)
                if (mask >> a & 1u) h += c[a] * (uint64_t)C[a * 256 + s];
            w[s] = (double)h;
        }
        double lam;
        r.status = comp_lambda(w, (double)n * (double)lq, &lam);
        if (r.status == 0) r.lambda_hit = lam, r.ratio16 = swg_comp_ratio16(lam, lambda_std);
    } else if (n > 0) {
        r.status = std_status;
    }
    int16_t T[256];
    for (int s = 0; s < 256; ++s) T[s] = swg_comp_rescale(s - 128, F, r.ratio16);
    r.scaled_score = comp_fill(sub, query, pssm, lq, seq, len, T, F * go, F * ge);
    r.adj_score = swg_comp_unscale(r.scaled_score, F);
    *out = r;
}

// the refusal of a pair whose int32 cells could wrap (swg.h)
bool swg_comp_pair_fits(size_t lq, size_t len, int go, int ge, int F)
{
    const uint64_t big = (uint64_t)std::max(127, std::max(std::abs(go), std::abs(ge)));
    return (uint64_t)(lq + len) * (uint64_t)F * big < (1ull << 31);
}

extern "C" int swg_comp_adjust_host(const int8_t sub[32][32], int gap_open, int gap_extend, const int8_t *query, const int8_t *pssm,
                                    size_t lq, const int8_t *seq, size_t len, const double *freq, int scale, swg_comp_result *out,
                                    double *lambda_std)
{
    const char *fn = "swg_comp_adjust_host";
    if (lambda_std) *lambda_std = 0.0;
    if (!out || (!seq && len) || (query != nullptr) == (pssm != nullptr) || (query && !sub) || lq == 0)
        return swg_set_global_error(SWG_ERR_ARG, "%s: NULL argument, an empty query, or not exactly one of query and pssm", fn);
    if (scale < 1 || scale > SWG_COMP_SCALE_MAX) return swg_set_global_error(SWG_ERR_ARG, "%s: scale must be 1..%d", fn, SWG_COMP_SCALE_MAX);
    if (gap_open < -32768 || gap_open > 32767 || gap_extend < -32768 || gap_extend > 32767)
        return swg_set_global_error(SWG_ERR_ARG, "%s: gap scores must fit an int16", fn);
    for (size_t p = 0; query && p < lq; ++p)
        if (query[p] < 1 || query[p] > 31) return swg_set_global_error(SWG_ERR_RESIDUE, "%s: residue index %d in the query outside 1..31", fn, query[p]);
    for (size_t j = 0; j < len; ++j)
        if (seq[j] < 0 || seq[j] > 31) return swg_set_global_error(SWG_ERR_RESIDUE, "%s: residue index %d in the sequence outside 0..31", fn, seq[j]);
    double P[32];
    uint32_t mask;
    const int rc = swg_pssm_background(fn, freq, P, &mask);
    if (rc != SWG_OK) return rc;
    const int go = gap_open + gap_extend, ge = gap_extend;
    if (!swg_comp_pair_fits(lq, len, go, ge, scale))
        return swg_set_global_error(SWG_ERR_ARG, "%s: a pair of %zu x %zu at scale %d could leave int32 cells", fn, lq, len, scale);
    try {
        std::vector<uint32_t> C(32 * 256);
        swg_comp_counts(sub, query, pssm, lq, C.data());
        double lam_std;
        const int st = swg_comp_lambda_std(C.data(), P, mask, &lam_std);
        if (lambda_std) *lambda_std = lam_std;
        swg_comp_pair(sub, go, ge, query, pssm, lq, C.data(), mask, lam_std, st, seq, len, scale, out);
    } catch (const std::exception &) {
        return swg_set_global_error(SWG_ERR_NOMEM, "%s: out of host memory", fn);
    }
    return SWG_OK;
}

int swg_comp_pairs_host(const swg_db *db, const int8_t sub[32][32], int go, int ge, const int8_t *src, bool pssm,
                        const uint64_t *q_offsets, const uint32_t *C, uint32_t mask, const double *lambda_std, const int *std_status,
                        int F, const SwgCompHostPair *pairs, size_t n, swg_comp_result *out)
{
    int bad = 0;
#pragma omp parallel for schedule(dynamic, 1) reduction(| : bad) num_threads(swg_host_threads())
    for (size_t h = 0; h < n; ++h) {
        try {
            const SwgCompHostPair &pr = pairs[h];
            size_t len = pr.len;
            std::vector<int8_t> seq(len + 1);
            if (swg_db_sequence(db, pr.index, seq.data(), len, &len) != SWG_OK) {
                bad |= 1;
                continue;
            }
            const size_t q0 = (size_t)(q_offsets[pr.query] - q_offsets[0]), lq = (size_t)(q_offsets[pr.query + 1] - q_offsets[pr.query]);
            const int8_t *q = src + (q_offsets[0] + q0) * (pssm ? 32 : 1);
            swg_comp_pair(sub, go, ge, pssm ? nullptr : q, pssm ? q : nullptr, lq, C + pr.cq * 32 * 256, mask, lambda_std[pr.cq],
                          std_status[pr.cq], seq.data(), len, F, &out[pr.dest]);
        } catch (const std::exception &) {
            bad |= 2;
        }
    }
    return bad;
}
