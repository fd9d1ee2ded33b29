"""GPU (-m gpu): the gapless prefilter search (swg_search_gapless, its batch forms, Context.search_gapless*).  Truth
everywhere is the oracle with the gaps priced out (gapless_cases.oracle_gapless); every comparison is bit-exact.  Route 1
is the gapless cells on the work queue (swg_stats.cell_form 6), route 0 the gapped machinery with the gaps priced out."""
import ctypes as C
import functools

import numpy as np
import pytest

import gapless_cases as gc
import scoring_edges as se
from conftest import load_golden
from test_gpu_parity import _reset_options
from test_gpu_pssm_multi import _pssm31

pytestmark = pytest.mark.gpu

GOLDENS = ("blosum62_lq1", "blosum62_tiny_db", "pam250_partial_lanes", "pam250_lq128", "blosum45_lq200", "blosum62_lq367",
           "blosum62_query_bzx")


@pytest.fixture(autouse=True)
def _options(ctx):
    _reset_options(ctx)
    ctx.set_option("autotune", 0)
    yield
    _reset_options(ctx)
    ctx.set_option("autotune", 1)
    ctx.set_option("side_readout", 1)


@functools.lru_cache(maxsize=None)
def _golden(name):
    import swg_loader
    g = load_golden(name)
    truth = gc.oracle_gapless(swg_loader.oracle(), g["query"], g["flat"], g["offsets"], g["sub"])
    truth.setflags(write=False)
    return g, truth


def _geometries(lq):
    geo = [(0, 0)]
    for lanes in (16, 32, 64):
        k = -(-lq // lanes)
        if 2 <= k <= 32:
            geo.append((lanes, k))
    return geo


def _check(ctx, db, truth, label, form6=True, ks=None):
    n = len(truth)
    for k in ks or (10, n + 3):
        scores, hits, st = ctx.search_gapless(db, k=k)
        assert np.array_equal(scores, truth), (label, k, st, np.nonzero(scores != truth)[0][:8])
        assert hits == gc.expected_hits(truth, k), (label, k, st)
        assert (st["cell_form"] == 6) == form6, (label, st)
    return st


# ---- 1. parity over geometries ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLDENS)
def test_gapless_goldens_over_geometries(swg, ctx, name):
    g, truth = _golden(name)
    lq = len(g["query"])
    ctx.set_scoring(g["sub"], int(g["gaps"][0]), int(g["gaps"][1]))
    ctx.set_query(g["query"])
    db = swg.Database(g["flat"], g["offsets"]).upload(ctx)
    seen = set()
    for lanes, k in _geometries(lq):
        ctx.set_option("group_lanes", lanes)
        ctx.set_option("cols_per_wave", k)
        for batch in (8, 1):
            ctx.set_option("batch", batch)
            st = _check(ctx, db, truth, (name, lanes, k, batch))
            assert st["path_bits"] == 16 and st["engine"] == 2 and st["work_queue"] == 1 and st["passes"] == 1, st
            assert st["fill_launches"] >= 1 and st["cells"] == lq * len(g["flat"]), st
            assert st["group_lanes"] * st["cols_per_wave"] >= lq, st
            if lanes:
                assert (st["group_lanes"], st["cols_per_wave"]) == (lanes, k), st
            seen.add(st["cols_per_wave"])
    print(name, "lq", lq, "K run:", sorted(seen))
    db.close()


def test_gapless_geometries_reach_every_chunk_remainder():
    """The forced geometries above cover K = 1, 2, 3 and 0 mod 4 (the cells' last profile chunk is partly used)."""
    ks = set()
    for name in GOLDENS:
        ks |= {k for _, k in _geometries(len(_golden(name)[0]["query"])) if k}
    assert {13, 23, 6, 2, 8, 12} <= ks, sorted(ks)


# ---- 2. ceilings --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ceiling_case():
    import swg_loader
    rng = np.random.default_rng(4096)
    sub = se.diag127(zero0=True)
    q = rng.integers(1, 32, size=300).astype(np.int8)
    flat, off, copy_len = gc.ceiling_db(rng, q)
    truth = gc.oracle_gapless(swg_loader.oracle(), q, flat, off, sub)
    truth.setflags(write=False)
    return sub, q, flat, off, copy_len, truth


@pytest.mark.parametrize("wide16", [1, 0], ids=["rerun_wide", "rerun_int16_int32"])
def test_gapless_ceilings(swg, ctx, wide16):
    sub, q, flat, off, copy_len, truth = _ceiling_case()
    for n, want in ((32, 4064), (33, 4191), (258, 32766), (259, 32893)):
        assert (truth[copy_len == n] == want).all(), n
    ctx.set_scoring(sub, -11, -1)
    ctx.set_query(q)
    ctx.set_option("wide16", wide16)
    db = swg.Database(flat, off).upload(ctx)
    st = _check(ctx, db, truth, ("ceilings", wide16), ks=(10,))
    assert st["n_rescored"] == int((truth >= 4096).sum()), st
    scores, _, _ = ctx.search_gapless(db)
    assert (scores[copy_len == 32] == 127 * 32).all()
    db.close()


# ---- 3. nothing leaks from pair to pair ---------------------------------------------------------------------------
@pytest.mark.parametrize("copy", [31, 37], ids=["below_flag", "flagged"])
def test_gapless_nothing_leaks_between_pairs(swg, orc, ctx, copy):
    """Every sequence has 37 residues, so the sorted order is the input order and a lane group streams copies and
    random sequences back to back: runs of 2 and 2, later of 16 and 16.  copy = 31: a 31-residue copy of a query
    stretch and 6 random residues (127 x 31 = 3937, below the flag); copy = 37: a whole stretch (4699, flagged)."""
    rng = np.random.default_rng(copy)
    sub = se.diag127(zero0=True)
    q = rng.integers(1, 32, size=300).astype(np.int8)
    L, n = 37, 3000
    seqs = []
    for i in range(n):
        run = 2 if i < n // 2 else 16
        if (i // run) % 2 == 0:
            a = int(rng.integers(0, len(q) - copy + 1))
            seqs.append(np.concatenate([q[a:a + copy], rng.integers(1, 32, size=L - copy)]).astype(np.int8))
        else:
            seqs.append(rng.integers(1, 32, size=L).astype(np.int8))
    flat, off = gc.pack(seqs)
    truth = gc.oracle_gapless(orc, q, flat, off, sub)
    assert int((truth >= 127 * copy).sum()) >= n // 2 - 16 and int((truth < 1000).sum()) >= n // 3
    ctx.set_scoring(sub, -11, -1)
    ctx.set_query(q)
    ctx.set_option("workgroups", 2)
    db = swg.Database(flat, off).upload(ctx)
    for batch in (8, 1):
        ctx.set_option("batch", batch)
        st = _check(ctx, db, truth, ("leak", copy, batch), ks=(10,))
        assert st["workgroups"] <= 2 and st["n_rescored"] == int((truth >= 4096).sum()), st
    db.close()


# ---- 4. gap independence, and not the gapped score ----------------------------------------------------------------
def test_gapless_does_not_read_the_gap_scores(swg, ctx):
    g, truth = _golden("blosum62_lq367")
    db = None
    outs = []
    for go, ge in ((-11, -1), (0, -2048), (-32768, -32768)):
        ctx.set_scoring(g["sub"], go, ge)
        ctx.set_query(g["query"])
        if db is None:
            db = swg.Database(g["flat"], g["offsets"]).upload(ctx)
        scores, hits, st = ctx.search_gapless(db, k=20)
        assert st["cell_form"] == 6, (go, ge, st)
        outs.append((scores, hits))
    for scores, hits in outs:
        assert np.array_equal(scores, truth) and hits == gc.expected_hits(truth, 20)
    db.close()


def test_gapless_is_below_the_gapped_score_of_relatives_with_an_indel(swg, orc, ctx):
    rng = np.random.default_rng(40)
    sub = swg.load_scoring("BLOSUM62").table()
    q = swg.synth_query(40, 80)
    flat0, off0 = swg.synth_db(41, 600)
    seqs = se.seqs_of(flat0, off0)
    planted = list(range(0, 600, 25))
    for i in planted:                     # the two 40-residue flanks with one inserted residue between them
        seqs[i] = np.concatenate([q[:40], rng.integers(1, 21, size=1), q[40:]]).astype(np.int8)
    flat, off = gc.pack(seqs)
    ctx.set_scoring(sub, -11, -1)
    ctx.set_query(q)
    db = swg.Database(flat, off).upload(ctx)
    gapped, _, _ = ctx.search(db)
    gapless, _, st = ctx.search_gapless(db)
    assert np.array_equal(gapped, orc.score_db(q, flat, off, sub, -11, -1))
    assert np.array_equal(gapless, gc.oracle_gapless(orc, q, flat, off, sub)), st
    assert (gapless[planted] < gapped[planted]).all() and (gapless <= gapped).all()
    db.close()


# ---- 5. PSSM query ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lo,hi", [(-12, 12), (-128, 127)], ids=["small", "int8"])
def test_gapless_pssm_query(swg, orc, ctx, lo, hi):
    rng = np.random.default_rng(hi + 200)
    pssm, qp, subp = _pssm31(rng, 150, lo, hi)
    flat, off = swg.synth_db(0x955, 700)
    ctx.set_scoring(np.zeros((32, 32), dtype=np.int8), -11, -1)       # (the table is not the PSSM's: only the PSSM scores)
    ctx.set_query_pssm(pssm)
    db = swg.Database(flat, off).upload(ctx)
    truth = gc.oracle_gapless(orc, qp, flat, off, subp)
    _check(ctx, db, truth, ("pssm", lo, hi), ks=(7,))
    db.close()


# ---- 6. views and shards ------------------------------------------------------------------------------------------
def _search_prefilled(swg, ctx, db, k, fill=-7):
    scores = np.full(db.total_count, fill, dtype=np.int32)
    hits = (swg.Hit * max(k, 1))()
    nh = C.c_size_t(0)
    st = swg.Stats()
    rc = swg.lib.swg_search_gapless(ctx.handle, db.handle, scores.ctypes.data_as(C.c_void_p), C.cast(hits, C.c_void_p) if k else None, k,
                                    C.byref(nh), C.byref(st))
    assert rc == swg.SWG_OK, swg.lib.swg_last_error(ctx.handle)
    return scores, [(int(hits[i].score), int(hits[i].index)) for i in range(nh.value)], st.as_dict()


def test_gapless_views_and_shards(swg, ctx):
    g, truth = _golden("blosum62_lq367")
    n = len(truth)
    ctx.set_scoring(g["sub"], -11, -1)
    ctx.set_query(g["query"])
    db = swg.Database(g["flat"], g["offsets"]).upload(ctx)
    rng = np.random.default_rng(6)
    for sel in (np.arange(0, n, 3), rng.choice(n, size=129, replace=False), np.array([n // 2]), np.zeros(0, dtype=np.int64)):
        view = db.view(ctx, sel)
        scores, hits, st = _search_prefilled(swg, ctx, view, 10)
        want = np.full(n, -7, dtype=np.int32)
        want[sel] = truth[sel]
        assert np.array_equal(scores, want), (len(sel), st)
        assert hits == gc.expected_hits(truth, 10, sel), (len(sel), st)
        view.close()
    db.close()
    written = np.zeros(n, dtype=np.int64)
    for r in range(2):
        shard = swg.Database(g["flat"], g["offsets"], r, 2).upload(ctx)
        scores, hits, st = _search_prefilled(swg, ctx, shard, 10)
        mine = np.sort(shard.order().astype(np.int64))
        assert np.array_equal(np.nonzero(scores != -7)[0], mine) and np.array_equal(scores[mine], truth[mine]), (r, st)
        assert hits == gc.expected_hits(truth, 10, mine), (r, st)
        written[mine] += 1
        shard.close()
    assert (written == 1).all()


# ---- 7. top-K edges -----------------------------------------------------------------------------------------------
def test_gapless_topk_edges(swg, orc, ctx):
    rng = np.random.default_rng(77)
    sub = se.diag127(zero0=True)
    q = rng.integers(1, 32, size=60).astype(np.int8)
    seqs = [rng.integers(1, 32, size=int(rng.integers(5, 50))).astype(np.int8) for _ in range(500)]
    tie = np.concatenate([rng.integers(1, 32, size=3), q[10:30]]).astype(np.int8)
    for i in (3, 77, 78, 250, 499):        # planted ties: the SAME sequence (a 20-residue copy: 2540 or a little more) at five indices
        seqs[i] = tie.copy()
    flat, off = gc.pack(seqs)
    truth = gc.oracle_gapless(orc, q, flat, off, sub)
    top = int(truth[3])
    assert top >= 2540 and top == int(truth.max()) and (truth[[3, 77, 78, 250, 499]] == top).all() and int((truth == top).sum()) == 5
    ctx.set_scoring(sub, -2, -1)
    ctx.set_query(q)
    db = swg.Database(flat, off).upload(ctx)
    for k in (3, 5, 6, 500, 900):
        none, hits, st = ctx.search_gapless(db, want_scores=False, k=k)
        assert none is None and hits == gc.expected_hits(truth, k), (k, st)
    assert [i for _, i in ctx.search_gapless(db, want_scores=False, k=5)[1]] == [3, 77, 78, 250, 499]
    scores, hits, _ = ctx.search_gapless(db, k=0)
    assert hits == [] and np.array_equal(scores, truth)
    # a search in flight: SWG_ERR_STATE, and the same call once it has ended
    ticket = ctx.search_begin(db, k=1)
    nh = C.c_size_t(0)
    rc = swg.lib.swg_search_gapless(ctx.handle, db.handle, None, None, 0, C.byref(nh), None)
    assert rc == swg.SWG_ERR_STATE and "in flight" in swg.lib.swg_last_error(ctx.handle).decode()
    rc = swg.lib.swg_search_gapless_multi(ctx.handle, db.handle, q.ctypes.data_as(C.c_void_p), np.array([0, 60], dtype=np.uint64).ctypes.data_as(C.c_void_p),
                                          1, None, None, 0, None, None)
    assert rc == swg.SWG_ERR_STATE
    ctx.search_end(ticket)
    assert np.array_equal(ctx.search_gapless(db)[0], truth)
    db.close()


# ---- 8. route 0 is exact ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["multipass", "engine1", "f16_0"])
def test_gapless_route_0_forced_by_options(swg, ctx, how):
    g, truth = _golden("pam250_lq128")
    ctx.set_scoring(g["sub"], -11, -1)
    ctx.set_query(g["query"])
    if how == "multipass":
        ctx.set_option("group_lanes", 16)
        ctx.set_option("cols_per_wave", 2)
    elif how == "engine1":
        ctx.set_option("engine", 1)
    else:
        ctx.set_option("f16", 0)
    db = swg.Database(g["flat"], g["offsets"]).upload(ctx)
    st = _check(ctx, db, truth, how, form6=False, ks=(10,))
    if how == "multipass":
        assert st["passes"] == 4, st
    db.close()


def test_gapless_route_0_query_beyond_one_pass(swg, orc, ctx):
    g = load_golden("blosum62_tiny_db")
    q = swg.synth_query(2100, 2100)
    ctx.set_scoring(g["sub"], -11, -1)
    ctx.set_query(q)
    db = swg.Database(g["flat"], g["offsets"]).upload(ctx)
    truth = gc.oracle_gapless(orc, q, g["flat"], g["offsets"], g["sub"])
    st = _check(ctx, db, truth, "lq2100", form6=False, ks=(10,))
    assert st["passes"] >= 2, st
    db.close()


def test_gapless_route_0_ceilings(swg, ctx):
    sub, q, flat, off, copy_len, truth = _ceiling_case()
    ctx.set_scoring(sub, -2, -1)
    ctx.set_query(q)
    ctx.set_option("f16", 0)
    db = swg.Database(flat, off).upload(ctx)
    _check(ctx, db, truth, "ceilings_f16_0", form6=False, ks=(10,))
    db.close()


# ---- 9. batches ---------------------------------------------------------------------------------------------------
def test_gapless_batches_are_the_loop_of_single_searches(swg, orc, ctx):
    rng = np.random.default_rng(9)
    sc = swg.load_scoring("BLOSUM62").table()
    flat, off = swg.synth_db(0x9A, 900)
    own = swg.synth_query(5, 90)
    ctx.set_scoring(sc, -11, -1)
    ctx.set_query(own)
    db = swg.Database(flat, off).upload(ctx)
    before = ctx.search(db, k=5)
    lens = (1, 30, 64, 128, 128, 150, 200, 200)
    queries = [swg.synth_query(100 + i, L) for i, L in enumerate(lens)]
    got, hits, st = ctx.search_gapless_multi(db, queries, k=4)
    assert st["cells"] == sum(lens) * len(flat) and st["cell_form"] == 6, st
    again = ctx.search(db, k=5)
    assert np.array_equal(before[0], again[0]) and before[1] == again[1]          # the context's own query was kept
    pssms = [_pssm31(rng, L, -10, 10) for L in lens]
    pgot, phits, _ = ctx.search_gapless_multi_pssm(db, [p[0] for p in pssms], k=4)
    again = ctx.search(db, k=5)
    assert np.array_equal(before[0], again[0]) and before[1] == again[1]
    for i, qi in enumerate(queries):
        ctx.set_query(qi)
        one, one_hits, _ = ctx.search_gapless(db, k=4)
        assert np.array_equal(got[i], one) and hits[i] == one_hits, i
        assert np.array_equal(one, gc.oracle_gapless(orc, qi, flat, off, sc)), i
        ctx.set_query_pssm(pssms[i][0])
        one, one_hits, _ = ctx.search_gapless(db, k=4)
        assert np.array_equal(pgot[i], one) and phits[i] == one_hits, i
        assert np.array_equal(one, gc.oracle_gapless(orc, pssms[i][1], flat, off, pssms[i][2])), i
    db.close()
