"""A numpy restatement of the composition-based score adjustment of include/swg.h (swg_comp_adjust*), shared
by the CPU and GPU tests of that call family.  It restates the rule, not the library: lambda comes from bisection on
sum_s w[s] expm1(lambda s) = 0 (the same root, another formulation and another iteration than the library's Newton
steps), the score distributions are numpy's histograms, and the recurrence is stated twice -- a scalar int32 loop with
the int16 table, cell by cell, and a row-vectorised form (the left gap state as a running maximum) that the larger
cases use and that test_comp_host.py holds against the scalar one."""
import math

import numpy as np

import pssm_build_cases as pc

S = np.arange(-128, 128, dtype=np.int64)          # the scores, bin by bin


def background(freq=None):
    """(P normalised over A, the mask of A as a bool[32])."""
    f = pc.builtin_freq() if freq is None else np.asarray(freq, dtype=np.float64)
    A = f > 0
    A[0] = False
    return np.where(A, f, 0.0) / f[A].sum(), A


def profile_of(sub, query=None, pssm=None):
    """R[p, a] as int64[lq, 32]."""
    if pssm is not None:
        return np.asarray(pssm, dtype=np.int64).reshape(-1, 32)
    return np.asarray(sub, dtype=np.int64)[np.asarray(query, dtype=np.int64)]


def counts(R):
    """C[a, s + 128] = positions p with R[p, a] == s."""
    C = np.zeros((32, 256), dtype=np.int64)
    for a in range(32):
        C[a] = np.bincount(R[:, a] + 128, minlength=256)
    return C


def lambda_bisect(w):
    """The positive root of sum_s w[s] exp(lambda s) = sum_s w[s], to a relative width of 1e-13; None where it does not
    exist (the expected score is not negative, or no positive score has weight)."""
    w = np.asarray(w)
    pos = S[(w > 0) & (S > 0)]
    if w.dtype.kind in "iu":
        mean = int((w.astype(object) * S.astype(object)).sum())       # exact
    else:
        mean = math.fsum((w * S).tolist())
    if not mean < 0 or pos.size == 0:
        return None
    wf = w.astype(np.float64)

    def g(lam):
        return math.fsum((wf * np.expm1(lam * S)).tolist())

    lo, hi = 0.0, 1.0 / float(pos.max())
    while not g(hi) > 0.0:
        lo, hi = hi, 2.0 * hi
    while hi - lo > 1e-13 * hi:
        mid = 0.5 * (lo + hi)
        if g(mid) > 0.0:
            hi = mid
        else:
            lo = mid
    return 0.5 * (lo + hi)


def composition(seq, A):
    c = np.bincount(np.asarray(seq, dtype=np.int64), minlength=32)[:32].astype(np.int64)
    return np.where(A, c, 0)


def table(F, ratio16):
    """T[s + 128] = floor((s F ratio16 + 32768) / 65536), as int16 (Python's // floors toward minus infinity)."""
    T = np.array([(int(s) * F * ratio16 + 32768) // 65536 for s in S], dtype=np.int64)
    assert np.abs(T).max() <= 8192
    return T.astype(np.int16)


def fill_scalar(R, seq, T, go, ge):
    """The library's recurrence in scalar int32 cells with the int16 table: H, A and B floored at 0, go the score of a gap's
    first step, ge of every further one.  -> the best H."""
    lq, edge = R.shape[0], np.int32(max(go, ge, 0))
    go, ge = np.int32(go), np.int32(ge)
    D = np.zeros(lq + 1, dtype=np.int32)
    V = np.full(lq + 1, edge, dtype=np.int32)
    best = np.int32(0)
    zero = np.int32(0)
    for d in np.asarray(seq, dtype=np.int64):
        diag, left = zero, edge
        for i in range(1, lq + 1):
            H = np.int32(diag + np.int32(T[R[i - 1, d] + 128]))
            A, B = V[i], left
            diag = D[i]
            D[i] = max(H, A, B, zero)
            V[i] = max(np.int32(H + go), np.int32(A + ge), np.int32(B + go), zero)
            left = max(np.int32(H + go), np.int32(A + go), np.int32(B + ge), zero)
            best = max(best, H)
    return int(best)


def fill_rows(R, seq, T, go, ge):
    """The same recurrence a row at a time -> (best H, the best H of every query column).  Within a row H and A come from
    the row above; the left state is L_i = max(x_i, L_{i-1} + ge) with x_i = max(H_i + go, A_i + go, 0) and L_0 the
    border, i.e. i ge + the running maximum of x_k - k ge."""
    lq, edge = R.shape[0], max(go, ge, 0)
    Ts = T.astype(np.int64)[R + 128]                      # [lq, 32]
    D = np.zeros(lq + 1, dtype=np.int64)
    V = np.full(lq + 1, edge, dtype=np.int64)
    k = np.arange(lq + 1, dtype=np.int64)
    colbest = np.zeros(lq, dtype=np.int64)
    for d in np.asarray(seq, dtype=np.int64):
        H = D[:-1] + Ts[:, d]
        A = V[1:]
        x = np.empty(lq + 1, dtype=np.int64)
        x[0] = edge
        x[1:] = np.maximum(np.maximum(H, A) + go, 0)
        L = k * ge + np.maximum.accumulate(x - k * ge)
        B = L[:-1]
        newD = np.maximum(np.maximum(np.maximum(H, A), B), 0)
        newV = np.maximum(np.maximum(np.maximum(H + go, A + ge), B + go), 0)
        D[1:], V[1:] = newD, newV
        colbest = np.maximum(colbest, H)
    assert max(int(np.abs(D).max()), int(np.abs(V).max()), int(colbest.max())) < 2 ** 31
    return int(colbest.max()) if lq else 0, colbest


def adjust(sub, gap_open, gap_extend, seq, query=None, pssm=None, freq=None, F=32, scalar=False):
    """The whole rule for one pair -> dict: ratio16, status, lambda_hit, lambda_std (None where they do not exist), r65536
    (r x 65536 before it is rounded, None unless status is 0), scaled_score, adj_score, colbest."""
    R = profile_of(sub, query, pssm)
    P, A = background(freq)
    C = counts(R)
    lam_std = lambda_bisect(P[A] @ C[A].astype(np.float64))
    c = composition(seq, A)
    res = dict(ratio16=65536, status=1, lambda_hit=None, lambda_std=lam_std, r65536=None)
    if c.sum() > 0 and lam_std is not None:
        lam_hit = lambda_bisect(c[A] @ C[A])
        if lam_hit is not None:
            r = min(1.0, max(0.5, lam_hit / lam_std))
            res.update(status=0, lambda_hit=lam_hit, r65536=r * 65536.0, ratio16=int(math.floor(r * 65536.0 + 0.5)))
    T = table(F, res["ratio16"])
    go, ge = F * (gap_open + gap_extend), F * gap_extend
    if scalar:
        best, colbest = fill_scalar(R, seq, T, go, ge), None
    else:
        best, colbest = fill_rows(R, seq, T, go, ge)
    res.update(scaled_score=best, adj_score=(2 * best + F) // (2 * F), colbest=colbest, T=T)
    return res
