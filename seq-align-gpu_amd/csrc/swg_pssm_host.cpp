// swg_pssm_host.cpp -- the host half of the PSSM construction (include/swg.h "a PSSM from a query's hits"):
// the scale of a matrix (swg_matrix_lambda), the model on the host fed by the paths swg_align_hits* returns
// (swg_pssm_from_paths: the twin the device's kernels of swg_pssm.hip are held against, as swg_gumbel_fit_hist is the
// twin of the device's fit) and the writer of the file swg_pssm_load reads.  Host only: nothing here touches a GPU.
#include "swg_host_internal.h"
#include "../../include/swg_host.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

// The background of a call: P normalised, the mask of A.  SWG_ERR_ARG (with a message naming fn) for a malformed freq.
int swg_pssm_background(const char *fn, const double *freq, double P[32], uint32_t *mask)
{
    double w[32], tot;
    if (swg_freq_weights(freq, w, &tot) != SWG_OK)
        return swg_set_global_error(SWG_ERR_ARG, "%s: freq must be 32 finite, non-negative weights with freq[0] = 0 and a positive sum", fn);
    *mask = 0;
    for (int a = 0; a < 32; ++a) {
        P[a] = w[a] / tot;
        if (a >= 1 && P[a] > 0.0) *mask |= 1u << a;
    }
    return SWG_OK;
}

// sum_{a,b in A} P_a P_b exp(lam s_ab) - 1 and its derivative, rows and columns ascending
static void lambda_phi(const int8_t sub[32][32], const double P[32], uint32_t mask, double lam, double *phi, double *dphi)
{
    double s0 = 0.0, s1 = 0.0;
    for (int a = 1; a < 32; ++a) {
        if (!(mask >> a & 1u)) continue;
        for (int b = 1; b < 32; ++b) {
            if (!(mask >> b & 1u)) continue;
            const double e = P[a] * P[b] * std::exp(lam * (double)sub[a][b]);
            s0 += e;
            s1 += (double)sub[a][b] * e;
        }
    }
    *phi = s0 - 1.0;
    *dphi = s1;
}

int swg_pssm_lambda(const char *fn, const int8_t sub[32][32], const double P[32], uint32_t mask, double *lambda)
{
    double expected = 0.0;
    int best = -128;
    for (int a = 1; a < 32; ++a)
        for (int b = 1; b < 32; ++b)
            if ((mask >> a & 1u) && (mask >> b & 1u)) {
                expected += P[a] * P[b] * (double)sub[a][b];
                best = sub[a][b] > best ? sub[a][b] : best;
            }
    if (!(expected < 0.0) || best <= 0)
        return swg_set_global_error(SWG_ERR_ARG, "%s: the matrix has no lambda under this background (expected score %.6g, "
                                    "highest score %d: the first must be negative, the second positive)", fn, expected, best);
    // phi(0) = 0, phi'(0) = expected < 0, phi convex and unbounded: negative on (0, lambda), positive beyond.
    double lo = 0.0, hi = 1.0 / (double)best, phi, dphi;
    for (int i = 0;; ++i) {
        lambda_phi(sub, P, mask, hi, &phi, &dphi);
        if (phi > 0.0) break;
        if (i == 64 || !std::isfinite(phi)) return swg_set_global_error(SWG_ERR_ARG, "%s: no bracket for lambda", fn);
        lo = hi, hi *= 2.0;
    }
    // Newton from the right of the root (convex: the steps come down onto it), kept inside [lo, hi] by bisection
    double lam = hi;
    for (int it = 0; it < 200; ++it) {
        lambda_phi(sub, P, mask, lam, &phi, &dphi);
        if (std::fabs(phi) <= 1e-12) {
            *lambda = lam;
            return SWG_OK;
        }
        if (phi > 0.0) hi = lam;
        else lo = lam;
        double next = dphi > 0.0 ? lam - phi / dphi : 0.5 * (lo + hi);
        if (!(next > lo && next < hi)) next = 0.5 * (lo + hi);
        lam = next;
    }
    return swg_set_global_error(SWG_ERR_ARG, "%s: lambda did not converge (residual %.3g)", fn, phi);
}

extern "C" int swg_matrix_lambda(const int8_t sub[32][32], const double *freq, double *lambda)
{
    if (!sub || !lambda) return swg_set_global_error(SWG_ERR_ARG, "swg_matrix_lambda: NULL argument");
    *lambda = 0.0;
    double P[32];
    uint32_t mask;
    const int rc = swg_pssm_background("swg_matrix_lambda", freq, P, &mask);
    if (rc != SWG_OK) return rc;
    return swg_pssm_lambda("swg_matrix_lambda", sub, P, mask, lambda);
}

int swg_pssm_check_model(const char *fn, const int8_t sub[32][32], const double *freq, double pseudocount, double P[32],
                         uint32_t *mask, double *lambda)
{
    int rc = swg_pssm_background(fn, freq, P, mask);
    if (rc != SWG_OK) return rc;
    if (!(pseudocount > 0.0) || std::isinf(pseudocount))
        return swg_set_global_error(SWG_ERR_ARG, "%s: pseudocount must be finite and > 0", fn);
    return swg_pssm_lambda(fn, sub, P, *mask, lambda);
}

static inline int8_t pssm_round(double v, bool *clamped)
{
    const double r = v < 0.0 ? -std::floor(-v + 0.5) : std::floor(v + 0.5); // half away from zero
    *clamped = !(r >= -128.0 && r <= 127.0);
    return (int8_t)(r < -128.0 ? -128.0 : r > 127.0 ? 127.0 : r);
}

static int from_paths(const char *fn, const int8_t sub[32][32], const double *freq, double beta, const int8_t *query, size_t lq,
                      const int8_t *flat, const uint64_t *offsets, const swg_alignment *al, const char *ops, size_t ops_stride, size_t n_hits,
                      int blocks, int purge, int8_t *pssm_out, double *values_out, swg_pssm_info *info)
{
    if (!sub || !query || lq == 0 || !pssm_out || (n_hits && (!flat || !offsets || !al || !ops)))
        return swg_set_global_error(SWG_ERR_ARG, "%s: NULL argument or empty query", fn);
    if (blocks != 0 && blocks != 1) return swg_set_global_error(SWG_ERR_ARG, "%s: blocks must be 0 (the whole query) or 1 (per-column blocks)", fn);
    if (purge != 0 && (purge < 50 || purge > 100))
        return swg_set_global_error(SWG_ERR_ARG, "%s: purge must be 0 (off) or 50..100 (percent identity)", fn);
    double P[32], lambda;
    uint32_t mask;
    int rc = swg_pssm_check_model(fn, sub, freq, beta, P, &mask, &lambda);
    if (rc != SWG_OK) return rc;
    for (size_t p = 0; p < lq; ++p)
        if (query[p] < 1 || query[p] > 31)
            return swg_set_global_error(SWG_ERR_RESIDUE, "%s: residue index %d in the query outside 1..31", fn, query[p]);

    // the rows: 0 empty, 1..31 a residue, 32 a gap; row r's extent is [eb[r], ee[r]) (empty: a hit of score 0)
    const size_t R = n_hits + 1;
    std::vector<uint8_t> msa(R * lq, 0);
    std::vector<size_t> eb(R, 0), ee(R, 0);
    for (size_t p = 0; p < lq; ++p) msa[p] = (uint8_t)query[p];
    ee[0] = lq;
    uint32_t n_rows = 1, n_purged = 0;
    for (size_t h = 0; h < n_hits; ++h) {
        const swg_alignment &a = al[h];
        if (a.score <= 0 || a.n_ops == 0) continue;
        ++n_rows;
        const int8_t *d = flat + offsets[a.index];
        const size_t len = (size_t)(offsets[a.index + 1] - offsets[a.index]);
        const char *path = ops + h * ops_stride;
        if ((size_t)a.n_ops + 1 > ops_stride) return swg_set_global_error(SWG_ERR_ARG, "%s: hit %zu: n_ops %u does not fit ops_stride", fn, h, a.n_ops);
        uint8_t *row = msa.data() + (h + 1) * lq;
        size_t qp = a.q_begin, dp = a.d_begin;
        for (uint32_t s = 0; s < a.n_ops; ++s) {
            const char op = path[s];
            const bool uq = op == 'M' || op == 'D', ud = op == 'M' || op == 'I';
            if ((!uq && !ud) || (uq && qp >= lq) || (ud && dp >= len))
                return swg_set_global_error(SWG_ERR_ARG, "%s: hit %zu: the path leaves its pair at step %u", fn, h, s);
            if (op == 'M') row[qp] = (uint8_t)d[dp];
            else if (op == 'D') row[qp] = 32;
            qp += uq, dp += ud;
        }
        eb[h + 1] = a.q_begin, ee[h + 1] = qp;
    }
    const auto in_A = [&](uint8_t x) { return x >= 1 && x <= 31 && (mask >> x & 1u); };

    // the purge: rows in hit order, in integers; a purged row becomes a hit of score 0
    if (purge > 0) {
        const auto near = [&](size_t r, size_t s, bool to_query) {
            const uint8_t *x = msa.data() + r * lq, *y = msa.data() + s * lq;
            uint64_t c = 0, i = 0;
            for (size_t p = 0; p < lq; ++p) {
                const bool both = x[p] >= 1 && x[p] <= 31 && y[p] >= 1 && y[p] <= 31;
                c += both, i += both && x[p] == y[p];
            }
            return c >= 1 && (to_query ? i == c : 100u * i >= (uint64_t)purge * c);
        };
        std::vector<size_t> kept;
        for (size_t r = 1; r < R; ++r) {
            if (eb[r] >= ee[r]) continue;
            bool drop = near(r, 0, true);
            for (size_t j = 0; j < kept.size() && !drop; ++j) drop = near(r, kept[j], false);
            if (!drop) {
                kept.push_back(r);
                continue;
            }
            std::memset(msa.data() + r * lq, 0, lq);
            eb[r] = ee[r] = 0;
            --n_rows, ++n_purged;
        }
    }

    // exp(lambda sub[b][a]): b in the query's role
    double E[32][32];
    for (int b = 0; b < 32; ++b)
        for (int a = 0; a < 32; ++a) E[b][a] = std::exp(lambda * (double)sub[b][a]);
    uint32_t n_clamped = 0;
    // column p with m_p >= 1 from its frequencies and alpha_p: g, Q, v, the rounding
    const auto score_column = [&](size_t p, const double f[32], double alpha) {
        int8_t *out = pssm_out + p * 32;
        double *val = values_out ? values_out + p * 32 : nullptr;
        for (int a = 1; a < 32; ++a) {
            if (!(mask >> a & 1u)) continue;
            double g = 0.0;
            for (int b = 1; b < 32; ++b)
                if (mask >> b & 1u) g += f[b] * E[b][a];
            g *= P[a];
            const double Q = (alpha * f[a] + beta * g) / (alpha + beta);
            const double v = std::log(Q / P[a]) / lambda;
            bool clamped;
            out[a] = pssm_round(v, &clamped);
            n_clamped += clamped;
            if (val) val[a] = v;
        }
    };
    for (size_t p = 0; p < lq; ++p) { // the fallback every column starts from
        int8_t *out = pssm_out + p * 32;
        out[0] = 0;
        for (int a = 1; a < 32; ++a) out[a] = sub[query[p]][a];
        if (values_out)
            for (int a = 0; a < 32; ++a) values_out[p * 32 + a] = 0.0;
    }

    // counts over all rows: m_p and the columns some hit shows a residue in are the same under both models
    std::vector<uint32_t> n(lq * 32, 0), kp(lq, 0), mp(lq, 0);
    uint64_t sum_k = 0, n_m = 0, n_obs = 0;
    for (size_t p = 0; p < lq; ++p) {
        uint32_t m_hits = 0;
        for (size_t r = 0; r < R; ++r) {
            const uint8_t x = msa[r * lq + p];
            if (!in_A(x)) continue;
            ++n[p * 32 + x];
            m_hits += r > 0;
        }
        for (int a = 1; a < 32; ++a) kp[p] += n[p * 32 + a] > 0, mp[p] += n[p * 32 + a];
        if (mp[p] >= 1) sum_k += kp[p], ++n_m;
        n_obs += m_hits > 0;
    }
    double nbar = n_m ? (double)sum_k / (double)n_m : 0.0;

    if (!blocks) {
        // weights
        std::vector<double> w(R, 0.0);
        for (size_t r = 0; r < R; ++r) {
            double s = 0.0;
            for (size_t p = 0; p < lq; ++p) {
                const uint8_t x = msa[r * lq + p];
                if (in_A(x)) s += 1.0 / ((double)kp[p] * (double)n[p * 32 + x]);
            }
            w[r] = s;
        }
        for (size_t p = 0; p < lq; ++p) {
            if (mp[p] == 0) continue;
            double acc[32] = {0.0}, W = 0.0, f[32];
            for (size_t r = 0; r < R; ++r) {
                const uint8_t x = msa[r * lq + p];
                if (in_A(x)) acc[x] += w[r], W += w[r];
            }
            for (int a = 0; a < 32; ++a) f[a] = acc[a] / W;
            score_column(p, f, std::fmin(nbar, (double)mp[p]) - 1.0);
        }
    } else {
        // segments: the columns between two consecutive extent boundaries share R_p, hence the block and the weights
        std::vector<uint8_t> cut(lq + 1, 0);
        for (size_t r = 0; r < R; ++r)
            if (eb[r] < ee[r]) cut[eb[r]] = cut[ee[r]] = 1;
        std::vector<size_t> member;
        std::vector<uint32_t> bn, bk;
        std::vector<double> w;
        double sum_nbar = 0.0;
        for (size_t p0 = 0; p0 < lq;) {
            size_t p1 = p0 + 1;
            while (!cut[p1]) ++p1;
            member.clear();
            size_t L = 0, U = lq;
            for (size_t r = 0; r < R; ++r)
                if (eb[r] <= p0 && p0 < ee[r]) member.push_back(r), L = eb[r] > L ? eb[r] : L, U = ee[r] < U ? ee[r] : U;
            const size_t width = U - L;
            bn.assign(width * 32, 0), bk.assign(width, 0);
            uint64_t bsum_k = 0, bn_m = 0;
            for (size_t c = 0; c < width; ++c) {
                uint32_t m = 0;
                for (size_t r : member) {
                    const uint8_t x = msa[r * lq + L + c];
                    if (in_A(x)) ++bn[c * 32 + x];
                }
                for (int a = 1; a < 32; ++a) bk[c] += bn[c * 32 + a] > 0, m += bn[c * 32 + a];
                if (m >= 1) bsum_k += bk[c], ++bn_m;
            }
            const double bnbar = bn_m ? (double)bsum_k / (double)bn_m : 0.0;
            w.assign(member.size(), 0.0);
            for (size_t j = 0; j < member.size(); ++j) {
                double s = 0.0;
                for (size_t c = 0; c < width; ++c) {
                    const uint8_t x = msa[member[j] * lq + L + c];
                    if (in_A(x)) s += 1.0 / ((double)bk[c] * (double)bn[c * 32 + x]);
                }
                w[j] = s;
            }
            for (size_t p = p0; p < p1; ++p) {
                if (mp[p] == 0) continue;
                double acc[32] = {0.0}, W = 0.0, f[32];
                for (size_t j = 0; j < member.size(); ++j) {
                    const uint8_t x = msa[member[j] * lq + p];
                    if (in_A(x)) acc[x] += w[j], W += w[j];
                }
                for (int a = 0; a < 32; ++a) f[a] = acc[a] / W;
                score_column(p, f, std::fmin(bnbar, (double)mp[p]) - 1.0);
                sum_nbar += bnbar;
            }
            p0 = p1;
        }
        nbar = n_m ? sum_nbar / (double)n_m : 0.0;
    }
    if (info) {
        info->lambda = lambda, info->n_distinct = nbar;
        info->n_rows = n_rows, info->n_observed = (uint32_t)n_obs, info->n_clamped = n_clamped, info->n_purged = n_purged;
    }
    return SWG_OK;
}

extern "C" int swg_pssm_from_paths_ex(const int8_t sub[32][32], const double *freq, double pseudocount, const int8_t *query, size_t lq,
                                      const int8_t *flat, const uint64_t *offsets, const swg_alignment *al, const char *ops,
                                      size_t ops_stride, size_t n_hits, int blocks, int purge, int8_t *pssm_out, double *values_out,
                                      swg_pssm_info *info)
{
    try {
        return from_paths("swg_pssm_from_paths_ex", sub, freq, pseudocount, query, lq, flat, offsets, al, ops, ops_stride, n_hits, blocks, purge,
                          pssm_out, values_out, info);
    } catch (const std::bad_alloc &) {
        return swg_set_global_error(SWG_ERR_NOMEM, "swg_pssm_from_paths_ex: out of host memory");
    }
}

extern "C" int swg_pssm_from_paths(const int8_t sub[32][32], const double *freq, double pseudocount, const int8_t *query, size_t lq,
                                   const int8_t *flat, const uint64_t *offsets, const swg_alignment *al, const char *ops,
                                   size_t ops_stride, size_t n_hits, int8_t *pssm_out, double *values_out, swg_pssm_info *info)
{
    try {
        return from_paths("swg_pssm_from_paths", sub, freq, pseudocount, query, lq, flat, offsets, al, ops, ops_stride, n_hits, 0, 0, pssm_out,
                          values_out, info);
    } catch (const std::bad_alloc &) {
        return swg_set_global_error(SWG_ERR_NOMEM, "swg_pssm_from_paths: out of host memory");
    }
}

extern "C" int swg_pssm_save(const char *path, const int8_t *pssm, const int8_t *query, size_t lq)
{
    static const char cols[21] = "ARNDCQEGHILKMFPSTWYV";
    if (!path || !pssm || !query || lq == 0) return swg_set_global_error(SWG_ERR_ARG, "swg_pssm_save: NULL argument or empty PSSM");
    for (size_t p = 0; p < lq; ++p)
        if (!swg_index_letter(query[p]))
            return swg_set_global_error(SWG_ERR_ARG, "swg_pssm_save: query residue %d at position %zu has no letter", query[p], p + 1);
    FILE *f = fopen(path, "w");
    if (!f) return swg_set_global_error(SWG_ERR_IO, "swg_pssm_save: cannot write %s", path);
    fprintf(f, "\nPosition-specific scoring matrix built by swg_pssm_build\n          ");
    for (int c = 0; c < 20; ++c) fprintf(f, "   %c", cols[c]);
    fprintf(f, "\n");
    for (size_t p = 0; p < lq; ++p) {
        fprintf(f, "%5zu %c  ", p + 1, swg_index_letter(query[p]));
        for (int c = 0; c < 20; ++c) fprintf(f, " %3d", (int)pssm[p * 32 + swg_letter_index(cols[c])]);
        fprintf(f, "\n");
    }
    fprintf(f, "\n");
    const bool bad = ferror(f) != 0;
    if (fclose(f) != 0 || bad) return swg_set_global_error(SWG_ERR_IO, "swg_pssm_save: short write to %s", path);
    return SWG_OK;
}
