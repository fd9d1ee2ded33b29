"""GPU (-m gpu): views -- a chosen subset of a resident database searched as a database of its own (swg_db_view,
Database.view, Group.select).  A view reads its parent's residue bytes where they lie; what it reports must be what a
search of the same sequences reports: the oracle's scores (goldens: oracle32; planted databases: the analytic scores)
for the selected sequences, every other entry of scores_out untouched, and hits = the selected (score, index) pairs
sorted by score descending, index ascending."""
import numpy as np
import pytest

import topk_cases as tc
from conftest import load_golden
from test_gpu_parity import _reset_options

pytestmark = pytest.mark.gpu

GOLDENS = ("blosum62_tiny_db", "pam250_partial_lanes", "blosum62_f16_boundary", "pam250_overflow_w",
           "blosum62_gap_pos1_m3", "blosum62_lq3000", "gapedge_32767_1")
PLAN_FIELDS = ("engine", "cell_form", "cols_per_wave", "group_lanes", "waves", "passes", "fill_launches", "n_rescored")


@pytest.fixture(autouse=True)
def _options(ctx):
    _reset_options(ctx)
    ctx.set_option("autotune", 0)
    yield
    _reset_options(ctx)
    ctx.set_option("autotune", 1)
    ctx.set_option("side_readout", 1)


def _setup(ctx, g):
    ctx.set_scoring(g["sub"], int(g["gaps"][0]), int(g["gaps"][1]))
    ctx.set_query(g["query"])


def _expected_hits(truth, sel, k):
    sel = np.unique(np.asarray(sel, dtype=np.int64))
    return [(-s, i) for s, i in sorted((-int(truth[i]), int(i)) for i in sel)[:k]]


def _search_prefilled(swg, ctx, db, k, fill=-7):
    """ctx.search with scores_out pre-filled: what the search does not write stays `fill`."""
    import ctypes as C
    scores = np.full(db.total_count, fill, dtype=np.int32)
    hits = (swg.Hit * max(k, 1))()
    nh = C.c_size_t(0)
    st = swg.Stats()
    rc = swg.lib.swg_search(ctx.handle, db.handle, scores.ctypes.data_as(C.c_void_p), C.cast(hits, C.c_void_p) if k else None, k,
                            C.byref(nh), C.byref(st))
    assert rc == swg.SWG_OK, swg.lib.swg_last_error(ctx.handle)
    return scores, [(int(hits[i].score), int(hits[i].index)) for i in range(nh.value)], st.as_dict()


def _check_view(swg, ctx, view, truth, sel, lens, lq, label):
    sel_u = np.unique(np.asarray(sel, dtype=np.int64))
    assert view.count == len(sel_u) and view.total_count == len(truth), label
    assert view.residues == int(lens[sel_u].sum()), label
    assert sorted(int(v) for v in view.order()) == [int(v) for v in sel_u], label
    for k in (10, len(sel_u) + 5):
        scores, hits, st = _search_prefilled(swg, ctx, view, k)
        want = np.full(len(truth), -7, dtype=np.int32)
        want[sel_u] = truth[sel_u]
        assert np.array_equal(scores, want), (label, k, st)
        assert hits == _expected_hits(truth, sel_u, k), (label, k, st)
        assert st["cells"] == lq * int(lens[sel_u].sum()), (label, st)


def _selections(n, rng):
    sels = {"third": np.arange(0, n, 3), "one": np.array([n // 2]), "all": np.arange(n),
            "all_but_one": np.delete(np.arange(n), n // 3)}
    for size in (127, 128, 129):                       # either side of one bin
        if n >= size:
            sels["bin%d" % size] = rng.choice(n, size=size, replace=False)
    pick = rng.choice(n, size=max(2, n // 2), replace=False)
    sels["shuffled_dups"] = rng.permutation(np.concatenate([pick, pick[: len(pick) // 2], pick[:1]]))
    return sels


# ---- 1. goldens x selections --------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", [1, 2])
@pytest.mark.parametrize("name", GOLDENS)
def test_goldens_through_views(swg, ctx, name, engine):
    g = load_golden(name)
    _setup(ctx, g)
    ctx.set_option("engine", engine)
    truth = g["oracle32"]
    lens = np.diff(g["offsets"].astype(np.int64))
    n = len(lens)
    db = swg.Database(g["flat"], g["offsets"]).upload(ctx)
    rng = np.random.default_rng(len(name) * 7 + engine)
    for label, sel in _selections(n, rng).items():
        view = db.view(ctx, sel)
        _check_view(swg, ctx, view, truth, sel, lens, len(g["query"]), (name, engine, label))
        view.close()
    scores, _, _ = ctx.search(db)                      # the parent is what it was
    assert np.array_equal(scores, truth)
    db.close()


# ---- 2. same plan, same kernels -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pam250_partial_lanes", "blosum62_f16_boundary", "blosum62_lq3000", "pam250_overflow_w"])
def test_view_of_everything_plans_like_its_parent(swg, ctx, name):
    g = load_golden(name)
    _setup(ctx, g)
    n = len(g["offsets"]) - 1
    db = swg.Database(g["flat"], g["offsets"]).upload(ctx)
    view = db.view(ctx, np.arange(n))
    s_p, h_p, st_p = ctx.search(db, k=10)
    s_v, h_v, st_v = ctx.search(view, k=10)
    assert {f: st_v[f] for f in PLAN_FIELDS} == {f: st_p[f] for f in PLAN_FIELDS}
    assert np.array_equal(s_v, s_p) and h_v == h_p and np.array_equal(s_p, g["oracle32"])
    assert np.array_equal(view.order(), db.order())
    view.close()
    db.close()


@pytest.mark.parametrize("name", ["pam250_partial_lanes", "blosum62_f16_boundary", "blosum62_lq3000"])
def test_view_equals_a_packed_database_of_the_subset(swg, ctx, name):
    g = load_golden(name)
    _setup(ctx, g)
    off = g["offsets"].astype(np.int64)
    n = len(off) - 1
    sel = np.sort(np.random.default_rng(3).choice(n, size=n * 2 // 3, replace=False))
    sub_flat = np.concatenate([g["flat"][off[i]:off[i + 1]] for i in sel])
    sub_off = np.zeros(len(sel) + 1, dtype=np.uint64)
    sub_off[1:] = np.cumsum(off[sel + 1] - off[sel])
    db = swg.Database(g["flat"], g["offsets"]).upload(ctx)
    fresh = swg.Database(sub_flat, sub_off).upload(ctx)
    view = db.view(ctx, sel)
    s_f, h_f, st_f = ctx.search(fresh, k=10)
    s_v, h_v, st_v = ctx.search(view, k=10)
    assert np.array_equal(s_v[sel], s_f) and np.array_equal(s_f, g["oracle32"][sel])
    assert h_v == [(s, int(sel[i])) for s, i in h_f]
    assert np.array_equal(view.order(), sel[fresh.order()])          # slot for slot the same sequences
    assert {f: st_v[f] for f in PLAN_FIELDS} == {f: st_f[f] for f in PLAN_FIELDS}
    assert st_v["cells"] == st_f["cells"] and st_v["cells_padded"] == st_f["cells_padded"]
    assert view.packed_bytes < fresh.packed_bytes
    for d in (view, fresh, db):
        d.close()


# ---- 3. planted scores --------------------------------------------------------------------------------------------
def _planted(ctx):
    ctx.set_scoring(tc.table(), *tc.GAPS)
    ctx.set_query(tc.query())


def test_planted_best_score_left_out(swg, ctx):
    case = tc.threshold_case(4096)
    _planted(ctx)
    ctx.set_option("engine", 2)                        # (the lane groups: the engine whose f16 cells flag and re-run)
    ctx.set_option("f16", 2)
    truth = case["scores"]
    best = int(np.nonzero(truth == 4199)[0][0])
    sel = np.delete(np.arange(case["n"]), best)
    db = swg.Database(case["flat"], case["offsets"]).upload(ctx)
    view = db.view(ctx, sel)
    for k in case["ks"]:
        scores, hits, st = _search_prefilled(swg, ctx, view, k)
        assert scores[best] == -7 and np.array_equal(scores[sel], truth[sel]), k
        assert best not in [i for _, i in hits] and hits == _expected_hits(truth, sel, k), k
        assert st["cell_form"] == 2 and st["n_rescored"] == int((truth[sel] >= 4096).sum()), st
    _, _, st_p = ctx.search(db, k=5)
    assert st_p["n_rescored"] == int((truth >= 4096).sum()) == st["n_rescored"] + 1
    view.close()
    db.close()


def test_planted_tie_member_left_out(swg, ctx):
    case = tc.ties_case(8093)
    _planted(ctx)
    truth = case["scores"]
    gone = int(np.nonzero(truth == tc.TIES_T)[0][7])       # one of the tie, neither its first nor its last index
    sel = np.delete(np.arange(case["n"]), gone)
    db = swg.Database(case["flat"], case["offsets"]).upload(ctx)
    view = db.view(ctx, sel)
    for k in tc.TIES_KS:
        none, hits, _ = ctx.search(view, want_scores=False, k=k)
        assert none is None and hits == _expected_hits(truth, sel, k), k
    view.close()
    db.close()


# ---- 4. in flight together ----------------------------------------------------------------------------------------
def test_parent_and_view_in_flight_together(swg, ctx):
    g = load_golden("pam250_partial_lanes")
    _setup(ctx, g)
    truth = g["oracle32"]
    n = len(truth)
    sel = np.arange(1, n, 2)
    db = swg.Database(g["flat"], g["offsets"]).upload(ctx)
    view = db.view(ctx, sel)
    t = [ctx.search_begin(db, k=10, want_scores=True), ctx.search_begin(view, k=10, want_scores=True),
         ctx.search_begin(db, k=3, want_scores=True)]
    s2, h2, _ = ctx.search_end(t[1])
    s1, h1, _ = ctx.search_end(t[0])
    s3, h3, _ = ctx.search_end(t[2])
    assert np.array_equal(s1, truth) and h1 == _expected_hits(truth, np.arange(n), 10)
    assert np.array_equal(s3, truth) and h3 == _expected_hits(truth, np.arange(n), 3)
    want = np.zeros(n, dtype=np.int32)
    want[sel] = truth[sel]
    assert np.array_equal(s2, want) and h2 == _expected_hits(truth, sel, 10)
    view.close()
    db.close()


# ---- 5. everything else takes a view ------------------------------------------------------------------------------
def test_multi_searches_and_alignments_take_a_view(swg, ctx, orc):
    g = load_golden("pam250_partial_lanes")
    _setup(ctx, g)
    n = len(g["offsets"]) - 1
    sel = np.random.default_rng(11).choice(n, size=150, replace=False)
    sel_u = np.unique(sel)
    go, ge = int(g["gaps"][0]), int(g["gaps"][1])
    queries = [g["query"], swg.synth_query(501, 40), swg.synth_query(502, 77)]
    db = swg.Database(g["flat"], g["offsets"]).upload(ctx)
    view = db.view(ctx, sel)
    scores, hits, _ = ctx.search_multi(view, queries, k=6)
    for qi, q in enumerate(queries):
        want = orc.score_db(q, g["flat"], g["offsets"], g["sub"], go, ge)
        assert np.array_equal(scores[qi][sel_u], want[sel_u]) and hits[qi] == _expected_hits(want, sel_u, 6), qi
        assert not np.delete(scores[qi], sel_u).any()                 # (the binding's zeros: not written)
    pssms = [g["sub"][q.astype(np.int64)] for q in queries]             # row x = the table's row of residue x
    scores_p, hits_p, _ = ctx.search_multi_pssm(view, pssms, k=6)
    assert np.array_equal(scores_p, scores) and hits_p == hits
    # alignments: field for field, path for path what the parent gives
    _, h, _ = ctx.search(view, k=8)
    assert ctx.align_hits(view, h) == ctx.align_hits(db, h)
    assert ctx.align_hits_multi(view, queries, hits) == ctx.align_hits_multi(db, queries, hits)
    outside = int(np.setdiff1d(np.arange(n), sel_u)[0])
    with pytest.raises(swg.SwgError) as e:
        ctx.align_hits(view, [(0, outside)])
    assert e.value.code == swg.SWG_ERR_ARG
    view.close()
    db.close()


# ---- 6. shards ----------------------------------------------------------------------------------------------------
def test_shards_take_one_global_list(swg, ctx):
    g = load_golden("pam250_partial_lanes")
    _setup(ctx, g)
    truth = g["oracle32"]
    n = len(truth)
    sel = np.random.default_rng(12).choice(n, size=90, replace=False)
    keys, merged, counts = [], np.full(n, -7, dtype=np.int32), 0
    for r in range(3):
        shard = swg.Database(g["flat"], g["offsets"], r, 3).upload(ctx)
        view = shard.view(ctx, sel)
        assert set(int(v) for v in view.order()) == set(int(v) for v in shard.order()) & set(int(v) for v in sel)
        counts += view.count
        sc_r, hits_r, _ = _search_prefilled(swg, ctx, view, 20)
        mine = view.order()
        assert np.array_equal(np.nonzero(sc_r != -7)[0], np.sort(mine))     # only this shard's selected entries are written
        merged[mine] = sc_r[mine]
        keys += [swg.hit_key(a, b) for a, b in hits_r]
        view.close()
        shard.close()
    assert counts == len(sel)
    want = np.full(n, -7, dtype=np.int32)
    want[sel] = truth[sel]
    assert np.array_equal(merged, want)
    assert swg.topk_merge_keys(np.array(keys, dtype=np.uint64), 20) == _expected_hits(truth, sel, 20)


# ---- 7. lifetime and errors ---------------------------------------------------------------------------------------
def test_lifetime_and_errors(swg, ctx):
    g = load_golden("pam250_partial_lanes")
    _setup(ctx, g)
    truth = g["oracle32"]
    n = len(truth)
    sel = np.arange(0, n, 2)
    db = swg.Database(g["flat"], g["offsets"])
    with pytest.raises(swg.SwgError) as e:             # a parent that is not resident
        db.view(ctx, sel)
    assert e.value.code == swg.SWG_ERR_STATE
    db.upload(ctx)
    with pytest.raises(swg.SwgError) as e:             # an index >= total
        db.view(ctx, [0, n])
    assert e.value.code == swg.SWG_ERR_ARG
    db.upload(ctx)                                     # no view alive (the refused ones left none): allowed
    view = db.view(ctx, sel)
    with pytest.raises(swg.SwgError) as e:             # re-upload of a parent with a live view
        db.upload(ctx)
    assert e.value.code == swg.SWG_ERR_STATE
    with pytest.raises(swg.SwgError) as e:             # a view is resident from creation
        view.upload(ctx)
    assert e.value.code == swg.SWG_ERR_STATE
    with pytest.raises(swg.SwgError) as e:
        view.save("/dev/null")
    assert e.value.code == swg.SWG_ERR_ARG
    # view of a view: the intersection, a view of the root
    sub = view.view(ctx, np.arange(0, n, 3))
    both = np.arange(0, n, 6)
    assert sorted(int(v) for v in sub.order()) == [int(v) for v in both]
    # an empty view: no hits, no score written
    for empty in (db.view(ctx, np.zeros(0, dtype=np.uint32)), view.view(ctx, [1])):
        assert empty.count == 0 and empty.residues == 0 and empty.total_count == n
        scores, hits, st = _search_prefilled(swg, ctx, empty, 5)
        assert hits == [] and (scores == -7).all() and st["cells"] == 0
        empty.close()
    # the parent goes first, then the first view: the view of the view still reads the bytes
    db.close()
    scores, hits, _ = _search_prefilled(swg, ctx, view, 10)
    assert np.array_equal(scores[sel], truth[sel]) and hits == _expected_hits(truth, sel, 10)
    view.close()
    scores, hits, _ = _search_prefilled(swg, ctx, sub, 10)
    assert np.array_equal(scores[both], truth[both]) and hits == _expected_hits(truth, both, 10)
    assert (np.delete(scores, both) == -7).all()
    sub.close()
    # and the other order: views first
    db = swg.Database(g["flat"], g["offsets"]).upload(ctx)
    v = db.view(ctx, sel)
    v.close()
    v.close()
    assert np.array_equal(ctx.search(db)[0], truth)
    db.upload(ctx)                                     # its views are gone: allowed again
    assert np.array_equal(ctx.search(db)[0], truth)
    db.close()


# ---- 8. group -----------------------------------------------------------------------------------------------------
def test_group_select(swg, orc):
    g = load_golden("pam250_partial_lanes")
    truth = g["oracle32"]
    n = len(truth)
    go, ge = int(g["gaps"][0]), int(g["gaps"][1])
    sel = np.random.default_rng(13).choice(n, size=70, replace=False)
    grp = swg.Group([0, 0, 0])
    try:
        grp.set_option("autotune", 0)
        grp.set_scoring(g["sub"], go, ge)
        grp.set_query(g["query"])
        grp.load(g["flat"], g["offsets"])
        grp.select(sel)
        scores, hits, stats = grp.search(k=12)
        want = np.zeros(n, dtype=np.int32)
        want[sel] = truth[sel]
        assert np.array_equal(scores, want) and hits == _expected_hits(truth, sel, 12)
        lens = np.diff(g["offsets"].astype(np.int64))
        assert sum(st["cells"] for st in stats) == len(g["query"]) * int(lens[sel].sum())
        off = g["offsets"].astype(np.int64)
        for a, (s_, i_) in zip(grp.align_hits(hits[:5]), hits[:5]):
            sc_, co, ops = orc.pair_trace(g["query"], g["flat"][off[i_]:off[i_ + 1]], g["sub"], go, ge)
            assert (a["score"], a["index"], a["ops"]) == (s_, i_, ops) and sc_ == s_
            assert (a["q_begin"], a["q_end"], a["d_begin"], a["d_end"]) == co
        outside = int(np.setdiff1d(np.arange(n), sel)[0])
        with pytest.raises(swg.SwgError) as e:
            grp.align_hits([(0, outside)])
        assert e.value.code == swg.SWG_ERR_ARG
        with pytest.raises(swg.SwgError) as e:         # a refused list leaves the selection as it was
            grp.select([n])
        assert e.value.code == swg.SWG_ERR_ARG
        assert grp.search(k=12)[1] == hits
        grp.select(None)
        scores, hits, _ = grp.search(k=12)
        assert np.array_equal(scores, truth) and hits == _expected_hits(truth, np.arange(n), 12)
    finally:
        grp.close()
