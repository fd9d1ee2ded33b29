"""GPU (-m gpu): swg_calibrate / _multi / _multi_pssm -- the scores left on the device, histogrammed and fitted there.
Truth everywhere is evalue_cases.truth: the oracle's scores of the same swg_synth_db_iid sequences, histogrammed with
the 4095 clamp and fitted on the host; lambda, mu and K within 1e-9 relative, everything else equal.  The random
database is calib_len 64 and the query 50 residues unless a test says otherwise."""
import functools

import numpy as np
import pytest

import evalue_cases as ec
from test_gpu_parity import _reset_options
from test_gpu_pssm_multi import _pssm31

pytestmark = pytest.mark.gpu

LEN = 64


@pytest.fixture(autouse=True)
def _options(ctx):
    def reset():
        _reset_options(ctx)
        ctx.set_option("batch_geometry", 0)
        for key, v in ec.DEFAULTS.items():
            ctx.set_option(key, v)

    reset()
    ctx.set_option("autotune", 0)
    yield
    reset()
    ctx.set_option("autotune", 1)


@functools.lru_cache(maxsize=None)
def _table(name):
    import swg_loader
    t = swg_loader.load().load_scoring(name).table()
    t.setflags(write=False)
    return t


def _size(ctx, seqs, length=LEN, seed=1):
    ctx.set_option("calib_seqs", seqs)
    ctx.set_option("calib_len", length)
    ctx.set_option("calib_seed", seed)


def _query(swg, lq):
    return swg.synth_query(0xCA11B + lq, lq)


def _flat_pssm(value, lq=50):
    """A PSSM whose every entry is `value`, and the (q', sub') the oracle takes it as."""
    sub = np.zeros((32, 32), dtype=np.int8)
    sub[1:, 1:] = value
    q = np.ones(lq, dtype=np.int8)
    return sub[q.astype(np.int64)], q, sub


def _one(ctx):
    got = ctx.calibrate()
    return got, ctx.debug_calib_iters()[0]


# ---- 1. one query ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("matrix,gaps,seqs", [("BLOSUM62", (-11, -1), 200), ("BLOSUM62", (-11, -1), 16), ("PAM250", (-10, -2), 200),
                                              ("BLOSUM62", (-11, -1), 129)])
def test_index_query(swg, orc, ctx, matrix, gaps, seqs):
    """200 sequences: two bins and 56 empty slots that must not be counted; 16: one bin, 112 empty slots."""
    sub, q = _table(matrix), _query(swg, 50)
    _size(ctx, seqs)
    ctx.set_scoring(sub, *gaps)
    ctx.set_query(q)
    got, it = _one(ctx)
    want, want_it = ec.truth(swg, orc, q, sub, gaps, seqs, LEN)
    print(matrix, seqs, got, it)
    ec.assert_same(got, it, want, want_it, (matrix, seqs))
    assert got["status"] == 0 and got["n_seqs"] == seqs and got["lambda"] > 0 and got["K"] > 0


def test_pssm_query(swg, orc, ctx):
    pssm, qp, subp = _pssm31(np.random.default_rng(77), 50, lo=-9, hi=6)
    _size(ctx, 200)
    ctx.set_scoring(_table("BLOSUM62"), -11, -1)
    ctx.set_query_pssm(pssm)
    got, it = _one(ctx)
    ec.assert_same(got, it, *ec.truth(swg, orc, qp, subp, (-11, -1), 200, LEN), "pssm")
    assert got["status"] == 0


@pytest.mark.parametrize("kind", ["index", "pssm"])
def test_gapless(swg, orc, ctx, kind):
    sub, q = _table("BLOSUM62"), _query(swg, 50)
    _size(ctx, 200)
    ctx.set_scoring(sub, -11, -1)
    if kind == "pssm":
        pssm, q, sub = _pssm31(np.random.default_rng(78), 50, lo=-9, hi=6)
        ctx.set_query_pssm(pssm)
    else:
        ctx.set_query(q)
    got = ctx.calibrate(gapless=True)
    want, want_it = ec.truth(swg, orc, q, sub, (-11, -1), 200, LEN, gapless=True)
    ec.assert_same(got, ctx.debug_calib_iters()[0], want, want_it, kind)
    gapped, _ = ec.truth(swg, orc, q, sub, (-11, -1), 200, LEN)
    assert got["status"] == 0 and got["lambda"] != gapped["lambda"]


def test_a_callers_composition_of_three_residues(swg, orc, ctx):
    freq = np.zeros(32)
    freq[[1, 12, 23]] = [3.0, 2.0, 1.0]          # A, L, W
    sub, q = _table("BLOSUM62"), _query(swg, 50)
    _size(ctx, 200)
    ctx.set_scoring(sub, -11, -1)
    ctx.set_query(q)
    got = ctx.calibrate(freq=freq)
    ec.assert_same(got, ctx.debug_calib_iters()[0], *ec.truth(swg, orc, q, sub, (-11, -1), 200, LEN, freq=freq), "three residues")
    # a multiple of the same weights is the same composition, and the built-in one differs
    assert ctx.calibrate(freq=freq * 17.0) == got
    assert ctx.calibrate()["lambda"] != got["lambda"]
    for bad in (np.ones(32), -freq, np.zeros(32)):
        with pytest.raises(swg.SwgError) as e:
            ctx.calibrate(freq=bad)
        assert e.value.code == swg.SWG_ERR_ARG


def test_every_score_at_the_clamp_is_no_fit(swg, orc, ctx):
    """A PSSM of all 127s: every sequence scores 127 x 50 = 6350, every score counts as 4095: one bin, status 1."""
    pssm, q, sub = _flat_pssm(127)
    _size(ctx, 200)
    ctx.set_scoring(_table("BLOSUM62"), -11, -1)
    ctx.set_query_pssm(pssm)
    got, it = _one(ctx)
    want, want_it = ec.truth(swg, orc, q, sub, (-11, -1), 200, LEN)
    assert want["status"] == 1 and (want["lambda"], want["K"], want["mu"]) == (0.0, 0.0, 0.0)
    ec.assert_same(got, it, want, want_it, "all 127")
    assert np.isnan(swg.evalue(got, 1000, 50)) and swg.evalue_min_score(got, 1000, 10.0) == -1


# ---- 2. batches ------------------------------------------------------------------------------------------------------
def _index_batch(swg, fourth):
    """Lengths 30, 50, 50, a fourth (2100: several passes, so the whole batch goes one by one; 64: five queries in one
    launch, the last without a partner where two queries share a lane) and a degenerate query of '*'s, which scores 0
    against every sequence of the built-in composition."""
    qs = [_query(swg, 30), _query(swg, 50), swg.synth_query(5, 50)] + ([_query(swg, fourth)] if fourth else [])
    return qs + [np.full(50, 31, dtype=np.int8)]


def _pssm_batch(fourth):
    """The same lengths as PSSMs; the degenerate one is a PSSM of all 5s: every score equal."""
    rng = np.random.default_rng(79)
    trip = [_pssm31(rng, lq, lo=-9, hi=6) for lq in [30, 50, 50] + ([fourth] if fourth else [])]
    return trip + [_flat_pssm(5)]


def _launched_rows(swg):
    return max([r["grid_rows"] for r in swg.debug_launch_log_read()] or [0])


ROUTES = {"one_by_one": ({}, 2100), "one_launch": ({"engine": 2}, 0), "one_launch_odd": ({"engine": 2}, 64),
          "one_launch_qq0": ({"engine": 2, "qq": 0}, 64),
          "one_launch_geometry": ({"engine": 2, "batch_geometry": 1, "group_lanes": 16, "cols_per_wave": 4}, 0)}


@pytest.mark.parametrize("kind", ["index", "pssm"])
@pytest.mark.parametrize("route", list(ROUTES))
def test_batch(swg, orc, ctx, route, kind):
    opts, fourth = ROUTES[route]
    sub, gaps = _table("BLOSUM62"), (-11, -1)
    _size(ctx, 200)
    ctx.set_scoring(sub, *gaps)
    own = _query(swg, 41)
    ctx.set_query(own)
    for key, v in opts.items():
        ctx.set_option(key, v)
    swg.debug_launch_log(True)
    if kind == "index":
        qs = _index_batch(swg, fourth)
        got = ctx.calibrate_multi(qs)
        wants = [ec.truth(swg, orc, q, sub, gaps, 200, LEN) for q in qs]
    else:
        ps = _pssm_batch(fourth)
        got = ctx.calibrate_multi_pssm([p[0] for p in ps])
        wants = [ec.truth(swg, orc, p[1], p[2], gaps, 200, LEN) for p in ps]
    rows = _launched_rows(swg)
    swg.debug_launch_log(False)
    iters = ctx.debug_calib_iters()
    assert len(got) == len(wants) == len(iters)
    for i, (want, want_it) in enumerate(wants):
        ec.assert_same(got[i], iters[i], want, want_it, (route, kind, i))
    assert [g["status"] for g in got] == [0] * (len(got) - 1) + [1], got        # the degenerate one, neighbours unaffected
    assert (rows == 1) if fourth == 2100 else (rows >= 2), (route, rows)              # the route the test is named after
    # the context's own query is where it was
    _reset_options(ctx)
    mine, it = _one(ctx)
    ec.assert_same(mine, it, *ec.truth(swg, orc, own, sub, gaps, 200, LEN), "own query")
    assert mine["lq"] == 41


def test_an_empty_batch_and_a_batch_of_one(swg, orc, ctx):
    sub, gaps = _table("BLOSUM62"), (-11, -1)
    _size(ctx, 200)
    ctx.set_scoring(sub, *gaps)
    assert ctx.calibrate_multi([]) == [] and ctx.calibrate_multi_pssm([]) == []
    q = _query(swg, 50)
    got = ctx.calibrate_multi([q])
    ec.assert_same(got[0], ctx.debug_calib_iters()[0], *ec.truth(swg, orc, q, sub, gaps, 200, LEN), "one")


# ---- 3. determinism, options, state ---------------------------------------------------------------------------------
def test_two_calls_are_bit_equal_and_another_seed_is_not(swg, orc, ctx):
    sub, gaps = _table("BLOSUM62"), (-11, -1)
    qs = _index_batch(swg, 0)
    _size(ctx, 200)
    ctx.set_option("engine", 2)
    ctx.set_scoring(sub, *gaps)
    ctx.set_query(qs[1])
    first, first_one = ctx.calibrate_multi(qs), ctx.calibrate()
    assert ctx.calibrate_multi(qs) == first and ctx.calibrate() == first_one
    _size(ctx, 200, seed=2)
    other = ctx.calibrate()
    assert other["lambda"] != first_one["lambda"] and other["mu"] != first_one["mu"]
    ec.assert_same(other, ctx.debug_calib_iters()[0], *ec.truth(swg, orc, qs[1], sub, gaps, 200, LEN, seed=2), "seed 2")
    _size(ctx, 200, seed=1)
    assert ctx.calibrate() == first_one


def test_option_ranges(swg, ctx):
    for key, bad in (("calib_seqs", (1, 0, -5, (1 << 20) + 1)), ("calib_len", (7, 0, -1, (1 << 14) + 1)), ("calib_seed", (-1,))):
        for v in bad:
            with pytest.raises(swg.SwgError) as e:
                ctx.set_option(key, v)
            assert e.value.code == swg.SWG_ERR_ARG, (key, v)
    for key, ok in (("calib_seqs", (2, 1 << 20)), ("calib_len", (8, 1 << 14)), ("calib_seed", (0, 12345))):
        for v in ok:
            ctx.set_option(key, v)


def test_state_errors(swg, ctx):
    _size(ctx, 200)
    q = _query(swg, 50)
    fresh = swg.Context(0)
    try:
        fresh.set_option("calib_seqs", 16)
        fresh.set_option("calib_len", LEN)
        with pytest.raises(swg.SwgError) as e:
            fresh.calibrate()
        assert e.value.code == swg.SWG_ERR_STATE          # no scoring
        fresh.set_scoring(_table("BLOSUM62"), -11, -1)
        with pytest.raises(swg.SwgError) as e:
            fresh.calibrate()
        assert e.value.code == swg.SWG_ERR_STATE          # no query
        assert fresh.calibrate_multi([q])[0]["status"] == 0
    finally:
        fresh.close()
    # a search in flight
    ctx.set_scoring(_table("BLOSUM62"), -11, -1)
    ctx.set_query(q)
    flat, off = swg.synth_db_iid(9, 64, 40)
    db = swg.Database(flat, off).upload(ctx)
    ticket = ctx.search_begin(db, k=3)
    try:
        for call in (lambda: ctx.calibrate(), lambda: ctx.calibrate_multi([q, q]), lambda: ctx.calibrate_multi_pssm([np.zeros((4, 32), dtype=np.int8)])):
            with pytest.raises(swg.SwgError) as e:
                call()
            assert e.value.code == swg.SWG_ERR_STATE
    finally:
        ctx.search_end(ticket)
    assert ctx.calibrate()["status"] == 0
    db.close()


def test_calibrating_against_a_databases_own_composition(swg, orc, ctx):
    flat, off = swg.synth_db(3, 500, median=80.0, max_len=400)
    db = swg.Database(flat, off).upload(ctx)
    counts = db.composition(ctx)
    sub, q = _table("BLOSUM62"), _query(swg, 50)
    _size(ctx, 200)
    ctx.set_scoring(sub, -11, -1)
    ctx.set_query(q)
    got = ctx.calibrate(freq=counts)
    ec.assert_same(got, ctx.debug_calib_iters()[0], *ec.truth(swg, orc, q, sub, (-11, -1), 200, LEN, freq=counts.astype(np.float64)), "composition")
    db.close()


# ---- 4. self-consistency at the default size -----------------------------------------------------------------------
def test_self_consistency_at_the_default_size(swg, orc, ctx):
    """A query of 200, BLOSUM62 -11/-1, calibrated at the defaults (8192 x 384, seed 1); then a fresh random database of
    20 000 x 384 with another seed, cut at S = swg_evalue_min_score(E = 20).  swg_search_above's count must be the
    oracle's exactly -- 15 at S = 55, computed on the CPU (test_evalue_host.py) -- and lie in [P/4, 2.5 P] around the
    fit's own prediction P = swg_evalue(S) = 15.98: Poisson puts under 1e-4 outside, a K wrong by a factor of m or L or a
    lambda wrong by 3 % falls outside."""
    sub, gaps = _table("BLOSUM62"), (-11, -1)
    q = swg.synth_query(ec.SELF_QUERY_SEED, ec.SELF_LQ)
    ctx.set_scoring(sub, *gaps)
    ctx.set_query(q)
    got, it = _one(ctx)
    ec.assert_same(got, it, *ec.truth(swg, orc, q, sub, gaps, 8192, 384), "default size")
    assert (got["n_seqs"], got["seq_len"], got["lq"]) == (8192, 384, 200)
    flat, off = swg.synth_db_iid(ec.SELF_DB_SEED, ec.SELF_DB_SEQS, ec.SELF_DB_LEN)
    db = swg.Database(flat, off).upload(ctx)
    residues = int(off[-1])
    S = swg.evalue_min_score(got, residues, ec.SELF_E)
    P = swg.evalue(got, residues, S)
    hits, n_total, _ = ctx.search_above(db, S, cap=0)
    oracle_count = int((orc.score_db(q, flat, off, sub, *gaps) >= S).sum())
    print("fit", got, "S", S, "predicted", P, "device", n_total, "oracle", oracle_count)
    assert S == ec.SELF_MIN_SCORE
    assert n_total == oracle_count == ec.SELF_COUNT
    assert P / 4 <= n_total <= 2.5 * P, (P, n_total)
    assert swg.evalue(got, residues, S) <= ec.SELF_E < swg.evalue(got, residues, S - 1)
    db.close()
