"""Shared helpers of the E-value tests (plain module, no tests of its own).

The truth of a calibration is computed on the host from the same random sequences the library scores
(swg.synth_db_iid with the context's calib_seed): the oracle's scores, histogrammed with scores of 4095 and more counted
as 4095, fitted by swg.gumbel_fit_hist -- which test_evalue_host.py holds against an independent numpy Newton.  The
device's fit differs from it only in the order of its additions and the last places of exp, so lambda, mu and K must
agree to REL = 1e-9 and everything else exactly."""
import math

import numpy as np

import gapless_cases as gc

REL = 1e-9
BINS = 4096
DEFAULTS = {"calib_seqs": 8192, "calib_len": 384, "calib_seed": 1}

# The self-consistency case at the default size (test_evalue_host.py computes these on the CPU with the oracle,
# test_gpu_calibrate.py asks the device for the same): a query of 200 residues, BLOSUM62 -11/-1, calibrated against
# 8192 x 384 (seed 1), then a fresh random database of 20 000 x 384 with another seed, cut at E = 20.
SELF_QUERY_SEED, SELF_LQ = 0xE7A1, 200
SELF_DB_SEED, SELF_DB_SEQS, SELF_DB_LEN = 20251, 20000, 384
SELF_E = 20.0
SELF_MIN_SCORE = 55   # swg_evalue_min_score at E = 20 under the host's fit (lambda 0.28069, K 0.05271) ...
SELF_COUNT = 15       # ... and the oracle's count of sequences at or above it; the fit predicts P = 15.98


def newton_numpy(hist):
    """The fit of swg_gumbel_fit_hist (include/swg_host.h) restated with numpy -> (lambda, mu, n_iter, status)."""
    c = np.asarray(hist, dtype=np.float64)
    s = np.arange(len(c), dtype=np.float64)
    pop = np.nonzero(c)[0]
    if len(pop) < 2:
        return 0.0, 0.0, 0, 1
    n = c.sum()
    x0 = float(pop[0])
    xbar = (s * c).sum() / n
    var = (s * s * c).sum() / n - xbar * xbar
    lam = math.pi / math.sqrt(6.0 * var)
    status, it = 2, 0
    while it < 100:
        e = c * np.exp(-lam * (s - x0))
        A, B, D = e.sum(), (s * e).sum(), (s * s * e).sum()
        f = 1.0 / lam - xbar + B / A
        fp = (B / A) ** 2 - D / A - 1.0 / lam ** 2
        nxt = lam - f / fp
        if not nxt > 0.0:
            nxt = 0.5 * lam
        it += 1
        done = abs(nxt - lam) <= 1e-12 * lam
        lam = nxt
        if done:
            status = 0
            break
    A = (c * np.exp(-lam * (s - x0))).sum()
    return lam, x0 - math.log(A / n) / lam, it, status


def histogram(scores):
    return np.bincount(np.minimum(np.asarray(scores, dtype=np.int64), BINS - 1), minlength=BINS).astype(np.uint32)


def params_of(swg, scores, lq, seq_len):
    """Scores of one query against the random sequences -> (what Context.calibrate* must return, n_iter)."""
    fit = swg.gumbel_fit_hist(histogram(scores))
    K = 0.0 if fit["status"] == 1 else math.exp(fit["lambda"] * fit["mu"]) / (float(lq) * float(seq_len))
    return {"lambda": fit["lambda"], "K": K, "mu": fit["mu"], "lq": int(lq), "n_seqs": len(scores), "seq_len": int(seq_len),
            "status": fit["status"]}, fit["n_iter"]


def truth(swg, orc, q, sub, gaps, seqs, seq_len, seed=1, freq=None, gapless=False):
    """The host's calibration of an index query q under (sub, gaps); a PSSM of at most 31 distinct rows goes in as its
    (q', sub') (test_gpu_pssm_multi._pssm31)."""
    flat, off = swg.synth_db_iid(seed, seqs, seq_len, freq)
    go, ge = gc.PRICED_OUT if gapless else gaps
    scores = orc.score_db(np.asarray(q, dtype=np.int8), flat, off, np.asarray(sub, dtype=np.int8), go, ge)
    return params_of(swg, scores, len(q), seq_len)


def close(a, b):
    return a == b or abs(a - b) <= REL * max(abs(a), abs(b))


def assert_same(got, got_iter, want, want_iter, label=""):
    for key in ("lambda", "mu", "K"):
        assert close(got[key], want[key]), (label, key, got, want)
    for key in ("status", "lq", "n_seqs", "seq_len"):
        assert got[key] == want[key], (label, key, got, want)
    assert got_iter == want_iter, (label, "n_iter", got_iter, want_iter)
