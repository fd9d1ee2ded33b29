/*
 * swg_evalue.c -- score statistics on the host: the Gumbel fit a calibration runs (the device's fit,
 * swg_calib_fit_kernel, is this one bin for bin; the tests hold the two against each other) and the pure helpers that
 * turn a fit into E-values, bit scores and score cut-offs.  Host-only C.
 */
#include "../../include/swg.h"
#include "../../include/swg_host.h"

#include <math.h>

int swg_gumbel_fit_hist(const uint32_t *hist, size_t n_bins, double *lambda, double *mu, int *n_iter)
{
    if (!lambda || !mu || !n_iter || (n_bins && !hist)) return SWG_ERR_ARG;
    *lambda = 0.0;
    *mu = 0.0;
    *n_iter = 0;
    /* the moments as exact integers (n_bins is a few thousand: a score squared times a count stays far below 2^64) */
    uint64_t n = 0, s1 = 0, s2 = 0;
    size_t x0 = 0, x1 = 0;
    for (size_t s = 0; s < n_bins; s++) {
        if (!hist[s]) continue;
        if (n == 0) x0 = s;
        x1 = s;
        n += hist[s];
        s1 += (uint64_t)s * hist[s];
        s2 += (uint64_t)s * s * hist[s];
    }
    if (n == 0 || x0 == x1) return 1;
    const double xbar = (double)s1 / (double)n;
    const double var = (double)s2 / (double)n - xbar * xbar;
    double lam = 3.14159265358979323846 / sqrt(6.0 * var);
    int status = 2, it = 0;
    while (it < 100) {
        double A = 0.0, B = 0.0, D = 0.0;
        for (size_t s = x0; s <= x1; s++) {
            if (!hist[s]) continue;
            const double e = (double)hist[s] * exp(-lam * (double)(s - x0));
            A += e;
            B += (double)s * e;
            D += (double)s * (double)s * e;
        }
        const double r = B / A;
        const double f = 1.0 / lam - xbar + r;
        const double fp = r * r - D / A - 1.0 / (lam * lam);
        double next = lam - f / fp;
        if (!(next > 0.0)) next = 0.5 * lam;
        const double step = fabs(next - lam);
        ++it;
        const int done = step <= 1e-12 * lam;
        lam = next;
        if (done) {
            status = 0;
            break;
        }
    }
    double A = 0.0;
    for (size_t s = x0; s <= x1; s++)
        if (hist[s]) A += (double)hist[s] * exp(-lam * (double)(s - x0));
    *lambda = lam;
    *mu = (double)x0 - log(A / (double)n) / lam;
    *n_iter = it;
    return status;
}

static int usable(const swg_evalue_params *p) { return p && p->status == 0 && p->lambda > 0.0 && p->K > 0.0; }

double swg_evalue(const swg_evalue_params *p, uint64_t db_residues, int32_t score)
{
    if (!usable(p)) return NAN;
    return p->K * (double)p->lq * (double)db_residues * exp(-p->lambda * (double)score);
}

double swg_bitscore(const swg_evalue_params *p, int32_t score)
{
    if (!usable(p)) return NAN;
    return (p->lambda * (double)score - log(p->K)) / 0.69314718055994530942;
}

int32_t swg_evalue_min_score(const swg_evalue_params *p, uint64_t db_residues, double E)
{
    if (!usable(p) || !(E > 0.0)) return -1;
    if (swg_evalue(p, db_residues, 1) <= E) return 1;
    /* an estimate from the logarithms, then the definition: the smallest S whose E-value is within E */
    const double est = ceil((log(p->K * (double)p->lq * (double)db_residues) - log(E)) / p->lambda);
    if (!(est < 2147483000.0)) return -1;
    int32_t S = est < 2.0 ? 2 : (int32_t)est;
    while (S > 1 && swg_evalue(p, db_residues, S - 1) <= E) --S;
    while (swg_evalue(p, db_residues, S) > E) {
        if (S >= 2147483000) return -1;
        ++S;
    }
    return S;
}
