// swg_comp_rule.h -- the parts of the composition-based score adjustment (include/swg.h) that the host twin
// (swg_comp_host.cpp) and the device's kernels (swg_comp.hip) share word for word: the lambda iteration and the integer
// formulas behind it.  Nothing here reads memory of its own: the caller supplies the two sums of an iteration.
#ifndef SWG_COMP_RULE_H
#define SWG_COMP_RULE_H

#include <stdint.h>

#ifdef __HIPCC__
#define SWG_COMP_HD __host__ __device__ inline
#else
#define SWG_COMP_HD inline
#endif

#define SWG_COMP_SCALE_DEFAULT 32
#define SWG_COMP_SCALE_MAX 64
#define SWG_COMP_NEWTON_STEPS 100

// lambda(w): the positive root of f(lam) = sum_s w[s] exp(lam s) - W, for weights with sum_s s w[s] < 0 and a largest
// populated score smax > 0 (the caller has checked both: then f(0) = 0, f'(0) < 0, f is convex and unbounded, so it is
// negative on (0, lambda) and positive beyond).  eval(lam, &f, &df) gives sum_s w[s] exp(lam s) and sum_s s w[s] exp(lam s),
// the same values in every thread that runs this.
//   bracket   hi = 1 / smax, doubled until f(hi) > W (at most 64 times): lo < lambda <= hi <= 2 lambda.
//   Newton    from hi, i.e. from the right of the root, where the steps of a convex function come down onto it; a step that
//             leaves (lo, hi), or a slope that is not positive, is replaced by the bracket's middle; each iterate narrows
//             the bracket from its side.
//   stop      the first Newton step with |step| <= 1e-12 lambda is taken and ends the iteration: status 0.  After
//             SWG_COMP_NEWTON_STEPS iterates without one, or a bracket that never closes: status 2.
// Returns the status; *lambda is written for status 0 only.  No fused multiply-add in here or in eval (the translation
// units that include this switch contraction off), so host and device walk through the same iterates up to the order of
// eval's additions and the last places of exp.
template <class Eval> SWG_COMP_HD int swg_comp_solve(Eval &&eval, double W, int smax, double *lambda, int *iters)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    double lo = 0.0, hi = 1.0 / (double)smax, f = 0.0, df = 0.0;
    *iters = 0;
    for (int i = 0;; ++i) {
        eval(hi, &f, &df);
        if (f - W > 0.0) break;
        if (i == 64) return 2;
        lo = hi, hi = hi * 2.0;
    }
    double lam = hi;
    for (int it = 1; it <= SWG_COMP_NEWTON_STEPS; ++it) {
        const double phi = f - W; // (f and df are the sums at lam)
        *iters = it;
        if (phi == 0.0) {
            *lambda = lam;
            return 0;
        }
        if (df > 0.0) {
            const double newton = lam - phi / df;
            const double step = newton > lam ? newton - lam : lam - newton;
            if (step <= 1e-12 * lam) {
                *lambda = newton;
                return 0;
            }
        }
        if (phi > 0.0) hi = lam;
        else lo = lam;
        double next = df > 0.0 ? lam - phi / df : 0.5 * (lo + hi);
        if (!(next > lo && next < hi)) next = 0.5 * (lo + hi);
        lam = next;
        eval(lam, &f, &df);
    }
    return 2;
}

// ratio16 of two lambdas that exist: floor(min(1, max(0.5, hit / std)) * 65536 + 0.5)
SWG_COMP_HD uint32_t swg_comp_ratio16(double lambda_hit, double lambda_std)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    double r = lambda_hit / lambda_std;
    r = r < 0.5 ? 0.5 : r;
    r = r > 1.0 ? 1.0 : r;
    return (uint32_t)(r * 65536.0 + 0.5);
}

// T[s] = floor((s F ratio16 + 32768) / 65536), floor toward minus infinity (|s F ratio16| <= 2^29: the shift of a negative
// int64 is arithmetic on every compiler this builds with)
SWG_COMP_HD int16_t swg_comp_rescale(int s, int F, uint32_t ratio16)
{
    const int64_t v = (int64_t)s * F * (int64_t)ratio16 + 32768;
    return (int16_t)(v >> 16);
}

// adj_score = floor((2 scaled + F) / (2 F)) for scaled >= 0
SWG_COMP_HD int32_t swg_comp_unscale(int32_t scaled, int F)
{
    return (int32_t)((2 * (int64_t)scaled + F) / (2 * F));
}

#endif /* SWG_COMP_RULE_H */
