"""CPU: the host half of the E-value feature -- the Gumbel fit against an independent numpy Newton, the pure helpers
(swg_evalue, swg_bitscore, swg_evalue_min_score), the i.i.d. generator a calibration scores against, the new entry
points' argument checks, and the self-consistency case of the GPU tests computed with the oracle alone."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import evalue_cases as ec
from conftest import ROOT

NEW_SYMBOLS = ("swg_db_composition", "swg_calibrate", "swg_calibrate_multi", "swg_calibrate_multi_pssm", "swg_evalue", "swg_bitscore",
               "swg_evalue_min_score", "swg_synth_db_iid", "swg_gumbel_fit_hist")


def _gumbel_hist(lam, mu, n, seed):
    u = np.random.default_rng(seed).random(n)
    x = np.rint(mu - np.log(-np.log(u)) / lam).astype(np.int64)
    assert x.min() >= 0
    return np.bincount(x, minlength=int(x.max()) + 1)


def test_abi_and_binding(swg):
    text = open(os.path.join(ROOT, "include", "swg.h")).read() + open(os.path.join(ROOT, "include", "swg_host.h")).read()
    for name in NEW_SYMBOLS:
        assert name in swg.ABI_SYMBOLS and hasattr(swg.lib, name), name
        assert " %s(" % name in text, name
    assert swg.lib.swg_abi_version() == 3          # functions and a struct were added, no struct changed
    assert C.sizeof(swg.EvalueParams) == 40
    for method in ("calibrate", "calibrate_multi", "calibrate_multi_pssm"):
        assert callable(getattr(swg.Context, method, None)), method
    assert callable(getattr(swg.Database, "composition", None))
    for fn in ("evalue", "bitscore", "evalue_min_score", "gumbel_fit_hist", "synth_db_iid"):
        assert callable(getattr(swg, fn, None)), fn


def test_null_arguments_need_no_gpu(swg):
    p = swg.EvalueParams()
    counts = np.zeros(32, dtype=np.uint64)
    q = np.array([1, 2, 3, 4], dtype=np.int8)
    off = np.array([0, 2, 4], dtype=np.uint64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    calls = {
        "swg_calibrate": lambda: swg.lib.swg_calibrate(None, None, 0, C.byref(p)),
        "swg_calibrate_multi": lambda: swg.lib.swg_calibrate_multi(None, vp(q), vp(off), 2, None, 0, C.byref(p)),
        "swg_calibrate_multi_pssm": lambda: swg.lib.swg_calibrate_multi_pssm(None, vp(q), vp(off), 2, None, 0, C.byref(p)),
        "swg_db_composition": lambda: swg.lib.swg_db_composition(None, None, vp(counts)),
    }
    for name, call in calls.items():
        assert call() == swg.SWG_ERR_ARG, name
        assert name.encode() in swg.lib.swg_global_error(), name
    flat, offp = C.c_void_p(), C.c_void_p()
    assert swg.lib.swg_synth_db_iid(1, 4, 8, None, None, C.byref(offp)) == swg.SWG_ERR_ARG
    assert swg.lib.swg_synth_db_iid(1, 4, 8, None, C.byref(flat), None) == swg.SWG_ERR_ARG
    assert swg.lib.swg_synth_db_iid(1, 0, 8, None, C.byref(flat), C.byref(offp)) == swg.SWG_ERR_ARG
    assert swg.lib.swg_synth_db_iid(1, 4, 0, None, C.byref(flat), C.byref(offp)) == swg.SWG_ERR_ARG
    h = np.ones(4, dtype=np.uint32)
    lam, mu, it = C.c_double(), C.c_double(), C.c_int()
    assert swg.lib.swg_gumbel_fit_hist(vp(h), 4, None, C.byref(mu), C.byref(it)) == swg.SWG_ERR_ARG
    assert swg.lib.swg_gumbel_fit_hist(None, 4, C.byref(lam), C.byref(mu), C.byref(it)) == swg.SWG_ERR_ARG
    assert math.isnan(swg.lib.swg_evalue(None, 1, 1)) and math.isnan(swg.lib.swg_bitscore(None, 1))
    assert swg.lib.swg_evalue_min_score(None, 1, 1.0) == -1


# ---- the fit ------------------------------------------------------------------------------------------------------
def test_fit_recovers_a_known_gumbel_and_agrees_with_numpy(swg):
    lam0, mu0, n = 0.3, 30.0, 20000
    hist = _gumbel_hist(lam0, mu0, n, seed=2024)
    fit = swg.gumbel_fit_hist(hist)
    lam, mu, it, status = ec.newton_numpy(hist)
    print("library", fit, "numpy", (lam, mu, it, status))
    assert fit["status"] == 0 and status == 0
    se = 0.78 * lam0 / math.sqrt(n)
    assert abs(fit["lambda"] - lam0) <= 4 * se and abs(lam - lam0) <= 4 * se, (fit, lam, se)
    assert abs(fit["lambda"] - lam) <= 1e-9 * lam and abs(fit["mu"] - mu) <= 1e-9 * mu, (fit, lam, mu)
    assert fit["n_iter"] == it and 2 <= it <= 8, (fit, it)
    assert abs(fit["mu"] - mu0) < 0.1                      # (rounding to integers adds no bias to the location)


@pytest.mark.parametrize("lam0,mu0,n", [(0.27, 45.0, 8192), (0.7, 12.0, 500), (0.05, 300.0, 3000)])
def test_fit_agrees_with_numpy_on_other_shapes(swg, lam0, mu0, n):
    hist = _gumbel_hist(lam0, mu0, n, seed=n)
    fit = swg.gumbel_fit_hist(hist)
    lam, mu, it, status = ec.newton_numpy(hist)
    assert (fit["status"], fit["n_iter"]) == (status, it) == (0, it)
    assert ec.close(fit["lambda"], lam) and ec.close(fit["mu"], mu), (fit, lam, mu)
    # trailing empty bins change nothing, bit for bit
    assert swg.gumbel_fit_hist(np.concatenate([hist, np.zeros(4096 - len(hist))])) == fit


def test_fit_without_two_distinct_scores(swg):
    for hist in (np.zeros(0), np.zeros(64), [0, 0, 7, 0], [9]):
        assert swg.gumbel_fit_hist(hist) == {"lambda": 0.0, "mu": 0.0, "n_iter": 0, "status": 1}, hist
        assert ec.newton_numpy(hist)[3] == 1
    two = swg.gumbel_fit_hist([0, 3, 0, 5])
    assert two["status"] == 0 and two["lambda"] > 0


# ---- the helpers --------------------------------------------------------------------------------------------------
PARAMS = {"lambda": 0.285, "K": 0.058, "mu": 29.0, "lq": 200, "n_seqs": 8192, "seq_len": 384, "status": 0}


@pytest.mark.parametrize("residues", [1, 384 * 20000, 3_800_000_000, 2 ** 40])
def test_min_score_is_the_smallest_score_within_E(swg, residues):
    for E in (1e-300, 1e-50, 1e-10, 1e-3, 0.5, 1.0, 10.0, 20.0, 1e3, 1e9, 1e30):
        S = swg.evalue_min_score(PARAMS, residues, E)
        assert S >= 1, (residues, E, S)
        assert swg.evalue(PARAMS, residues, S) <= E, (residues, E, S)
        assert S == 1 or swg.evalue(PARAMS, residues, S - 1) > E, (residues, E, S)
    for E in (0.0, -1.0, float("nan")):
        assert swg.evalue_min_score(PARAMS, residues, E) == -1


def test_bitscore_and_evalue_are_consistent(swg):
    m, n = PARAMS["lq"], 384 * 20000
    for S in (1, 30, 55, 120, 900):
        E, bits = swg.evalue(PARAMS, n, S), swg.bitscore(PARAMS, S)
        assert E == pytest.approx(PARAMS["K"] * m * n * math.exp(-PARAMS["lambda"] * S), rel=1e-14)
        assert E == pytest.approx(m * n * 2.0 ** (-bits), rel=1e-12), (S, E, bits)


@pytest.mark.parametrize("status", [1, 2, -1])
def test_helpers_without_a_fit(swg, status):
    p = dict(PARAMS, status=status)
    assert math.isnan(swg.evalue(p, 1000, 50)) and math.isnan(swg.bitscore(p, 50))
    assert swg.evalue_min_score(p, 1000, 10.0) == -1
    none = dict(PARAMS, status=1)
    none.update({"lambda": 0.0, "K": 0.0, "mu": 0.0})
    assert math.isnan(swg.evalue(none, 1000, 50)) and swg.evalue_min_score(none, 1000, 10.0) == -1


# ---- the generator ------------------------------------------------------------------------------------------------
def _builtin_freq(swg):
    flat, _ = swg.synth_db(7, 4000, median=300.0)           # (the table swg_synth_db draws from, as it draws)
    return np.bincount(flat, minlength=32) / float(len(flat))


def test_iid_is_deterministic_and_of_exact_lengths(swg):
    flat, off = swg.synth_db_iid(5, 300, 77)
    assert np.array_equal(off, np.arange(301, dtype=np.uint64) * 77) and len(flat) == 300 * 77
    again, _ = swg.synth_db_iid(5, 300, 77)
    assert np.array_equal(flat, again)
    other, _ = swg.synth_db_iid(6, 300, 77)
    assert not np.array_equal(flat, other)
    # residue j of sequence i depends only on (seed, i, j): a larger and longer database begins alike
    big, _ = swg.synth_db_iid(5, 400, 100)
    assert np.array_equal(big.reshape(400, 100)[:300, :77], flat.reshape(300, 77))


def test_iid_follows_the_composition(swg):
    rough = _builtin_freq(swg)
    freq = np.zeros(32)
    freq[[1, 3, 5, 23, 31]] = [5.0, 1.0, 0.25, 2.0, 0.5]
    for f, n, length in ((None, 2000, 384), (freq, 3000, 100), (freq * 1e-200, 500, 64)):
        flat, _ = swg.synth_db_iid(11, n, length, f)
        share = np.bincount(flat, minlength=32) / float(len(flat))
        if f is None:
            assert ((share > 0) == (rough > 0)).all() and share[0] == 0
            assert np.abs(share - rough).max() < 0.01       # (the built-in table, seen through swg_synth_db's own draws)
            continue
        want = f / f.sum()
        assert (share[want == 0] == 0).all(), share
        sigma = np.sqrt(want * (1 - want) / len(flat))
        assert (np.abs(share - want) <= 5 * sigma).all(), (share, want, sigma)


def test_iid_refuses_malformed_compositions(swg):
    good = np.zeros(32)
    good[1:21] = 1.0
    bad = []
    for i, v in ((0, 1.0), (3, -0.5), (4, float("nan")), (5, float("inf"))):
        f = good.copy()
        f[i] = v
        bad.append(f)
    bad.append(np.zeros(32))
    for f in bad:
        with pytest.raises(swg.SwgError) as e:
            swg.synth_db_iid(1, 10, 10, f)
        assert e.value.code == swg.SWG_ERR_ARG
    with pytest.raises(ValueError):
        swg.synth_db_iid(1, 10, 10, np.ones(20))
    swg.synth_db_iid(1, 10, 10, good)


# ---- the self-consistency case of the GPU tests, with the oracle alone -------------------------------------------
def test_self_consistency_of_the_fit_on_the_cpu(swg, orc):
    """A query of 200 against the default 8192 x 384, then the count at E = 20 on a fresh 20 000 x 384: the oracle's
    count must lie in [P/4, 2.5 P] around the fit's prediction P (Poisson puts under 1e-4 outside for P near 18), and
    the constants test_gpu_calibrate.py holds the device to are these."""
    sc = swg.load_scoring("BLOSUM62")
    q = swg.synth_query(ec.SELF_QUERY_SEED, ec.SELF_LQ)
    p, it = ec.truth(swg, orc, q, sc.table(), (-11, -1), **{"seqs": 8192, "seq_len": 384, "seed": 1})
    assert p["status"] == 0 and 3 <= it <= 5, (p, it)
    assert 0.267 < p["lambda"] < 0.30 and 0.03 < p["K"] < 0.09, p          # (above the asymptotic 0.267: finite length)
    flat, off = swg.synth_db_iid(ec.SELF_DB_SEED, ec.SELF_DB_SEQS, ec.SELF_DB_LEN)
    residues = int(off[-1])
    S = swg.evalue_min_score(p, residues, ec.SELF_E)
    P = swg.evalue(p, residues, S)
    count = int((orc.score_db(q, flat, off, sc.table(), -11, -1) >= S).sum())
    print("fit", p, "S", S, "predicted", P, "observed", count)
    assert (S, count) == (ec.SELF_MIN_SCORE, ec.SELF_COUNT)
    assert P / 4 <= count <= 2.5 * P, (P, count)
