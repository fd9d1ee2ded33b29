"""GPU (-m gpu): every query of a batch against its own candidate list in one pass (swg_search_lists,
Context.search_lists, search_lists_pssm).

The result for query i is by definition what a view of list i searched with query i reports.  Truth is the oracle's:
orc.score_db per query over the whole database on the CPU (computed once per golden and batch, shared by the cases);
PSSM truth as tests/test_gpu_pssm_multi.py derives it (a PSSM of at most 31 distinct columns is an index query over a
synthetic table).  Everything is bit-exact.  scores_out is parallel to the lists: entry j of list i holds query i against
candidate j, duplicates included; entries the library ignores keep the pre-filled -7.  stats["fill_launches"] tells the
routes apart: the chunks launched on the one-launch route, 0 where the batch went one list after another."""
import numpy as np
import pytest

from conftest import load_golden
from test_gpu_parity import _reset_options
from test_gpu_pssm_multi import _pssm31

pytestmark = pytest.mark.gpu

FILL = -7
LENGTHS = (1, 30, 64, 128, 128, 150, 200, 200)
_TRUTH = {}


@pytest.fixture(autouse=True)
def _options(ctx):
    _reset_options(ctx)
    ctx.set_option("autotune", 0)
    yield
    _reset_options(ctx)
    ctx.set_option("autotune", 1)
    ctx.set_option("side_readout", 1)


def _queries(swg, g, lengths=LENGTHS):
    """Synthetic queries of the given lengths; the golden's own query stands in where its length is asked for."""
    qs = [swg.synth_query(0xA11 + 31 * i, lq) for i, lq in enumerate(lengths)]
    for i, lq in enumerate(lengths):
        if lq == len(g["query"]):
            qs[i] = g["query"].copy()
            break
    return qs


def _truth(orc, name, g, qs, tag="q"):
    key = (name, tag, len(qs))
    if key not in _TRUTH:
        go, ge = int(g["gaps"][0]), int(g["gaps"][1])
        t = np.stack([orc.score_db(q, g["flat"], g["offsets"], g["sub"], go, ge) for q in qs])
        t.setflags(write=False)
        _TRUTH[key] = t
    return _TRUTH[key]


def _expected_hits(truth_row, held, k):
    sel = np.unique(np.asarray(held, dtype=np.int64))
    return [(-s, i) for s, i in sorted((-int(truth_row[i]), int(i)) for i in sel)[:k]]


def _check(ctx, db, qs, lists, truth, lens, label, launches=1, form=None, held=None, search=None):
    """One call per k: scores at every entry, hits, n_hits (the hits' count), cells and the route."""
    held = held if held is not None else (lambda ix: np.ones(len(ix), dtype=bool))
    search = search or ctx.search_lists
    most = max([len(np.unique(l)) for l in lists] + [1])
    for k in (10, most + 3):
        scores, hits, st = search(db, qs, lists, k=k, fill=FILL)
        cells = 0
        for i, l in enumerate(lists):
            l = np.asarray(l, dtype=np.int64)
            mine = held(l)
            want = np.where(mine, truth[i][l], FILL) if len(l) else np.zeros(0, dtype=np.int32)
            assert np.array_equal(scores[i], want), (label, k, i, st)
            assert hits[i] == _expected_hits(truth[i], l[mine], k), (label, k, i, st)
            assert len(hits[i]) == min(k, len(np.unique(l[mine]))), (label, k, i)
            cells += len(qs[i]) * int(lens[np.unique(l[mine])].sum())
        assert st["cells"] == cells, (label, st)
        assert st["fill_launches"] == launches, (label, st)
        if launches:
            assert (st["engine"], st["work_queue"], st["path_bits"], st["passes"]) == (2, 1, 16, 1), (label, st)
            assert st["cell_form"] in (0, 2) and (form is None or st["cell_form"] == form), (label, st)
    _, hits0, _ = search(db, qs, lists, k=0, want_scores=False)
    assert hits0 == [[] for _ in lists], label
    return st


def _list_shapes(n, nq, lens, rng):
    third = n // 3
    shapes = {
        "disjoint_thirds": [np.arange(n)[(i % 3) * third:(i % 3 + 1) * third][i // 3::3] for i in range(nq)],
        "overlapping": [rng.choice(n // 2, size=n // 3, replace=False) for _ in range(nq)],
        "identical": [np.arange(5, n, 4)] * nq,
        "one_with_everything": [np.arange(n) if i == 3 else rng.choice(n, size=9, replace=False) for i in range(nq)],
        "sizes": [rng.choice(n, size=s, replace=False) for s in (0, 1, 2, 3, 127, 128, 129)] + [rng.choice(n, size=5, replace=False)],
    }
    dups = []
    for _ in range(nq):
        pick = rng.choice(n, size=41, replace=False)
        dups.append(rng.permutation(np.concatenate([pick, pick[:20], pick[:1], pick[:1]])))
    shapes["shuffled_dups"] = dups
    longest, shortest = int(np.argmax(lens)), int(np.argmin(lens))
    shapes["longest_next_to_shortest"] = [np.array([shortest]) if i % 2 else np.array([longest, shortest, (longest + 1) % n])
                                          for i in range(nq)]
    return shapes


# ---- 1. + 2. parity over list shapes, on both cell forms ----------------------------------------------------------------
@pytest.mark.parametrize("f16", [1, 0])
@pytest.mark.parametrize("name", ["pam250_lq128", "blosum45_lq200"])
def test_parity_over_list_shapes(swg, orc, ctx, name, f16):
    g = load_golden(name)
    ctx.set_scoring(g["sub"], int(g["gaps"][0]), int(g["gaps"][1]))
    ctx.set_option("f16", f16)
    qs = _queries(swg, g)
    truth = _truth(orc, name, g, qs)
    lens = np.diff(g["offsets"].astype(np.int64))
    n = len(lens)
    db = swg.Database(g["flat"], g["offsets"]).upload(ctx)
    rng = np.random.default_rng(len(name) + f16)
    for label, lists in _list_shapes(n, len(qs), lens, rng).items():
        # (no query of these batches can reach 4096: 200 columns x the table's best entry, 17, is 3400)
        _check(ctx, db, qs, lists, truth, lens, (name, f16, label), form=2 if f16 else 0)
    db.close()


def test_a_query_that_can_pass_4096_takes_the_int16_cells(swg, orc, ctx):
    g = load_golden("blosum62_f16_boundary")
    ctx.set_scoring(g["sub"], int(g["gaps"][0]), int(g["gaps"][1]))
    n = len(g["offsets"]) - 1
    qs = [swg.synth_query(0xB0B, 90), g["query"].copy(), swg.synth_query(0xB0C, 200)]
    truth = _truth(orc, "blosum62_f16_boundary", g, qs)
    assert int(truth[1].max()) == 6410 == int(g["oracle32"].max())
    lens = np.diff(g["offsets"].astype(np.int64))
    lists = [np.arange(0, n, 2), np.arange(n)[::-1], np.arange(1, n, 3)]
    db = swg.Database(g["flat"], g["offsets"]).upload(ctx)
    _check(ctx, db, qs, lists, truth, lens, "f16_boundary", form=0)
    db.close()


# ---- 3. chunk edges ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [1, 2, 255, 256, 257])
def test_chunk_edges(swg, orc, ctx, nq):
    g = load_golden("blosum62_tiny_db")
    ctx.set_scoring(g["sub"], int(g["gaps"][0]), int(g["gaps"][1]))
    lens = np.diff(g["offsets"].astype(np.int64))
    n = len(lens)
    rng = np.random.default_rng(257)
    all_q = [swg.synth_query(0xC0DE + i, 8 + (i * 7) % 17) for i in range(257)]
    truth = _truth(orc, "blosum62_tiny_db", g, all_q, tag="chunks")
    sizes = rng.integers(0, 41, size=257)
    sizes[[0, 255, 256]] = (7, 0, 12)                        # (the first and the 257th have work; the 256th is empty)
    all_lists = [rng.choice(n, size=int(s), replace=False) for s in sizes]
    db = swg.Database(g["flat"], g["offsets"]).upload(ctx)
    _check(ctx, db, all_q[:nq], all_lists[:nq], truth, lens, nq, launches=2 if nq == 257 else 1)
    if nq == 257:                                            # the second chunk's rows are the chunk's own: query 256 alone
        _check(ctx, db, all_q[256:], all_lists[256:], truth[256:], lens, "last_alone")
    db.close()


def test_all_lists_empty_launches_nothing(swg, ctx):
    g = load_golden("blosum62_tiny_db")
    ctx.set_scoring(g["sub"], int(g["gaps"][0]), int(g["gaps"][1]))
    db = swg.Database(g["flat"], g["offsets"]).upload(ctx)
    qs = [swg.synth_query(1, 10), swg.synth_query(2, 12)]
    scores, hits, st = ctx.search_lists(db, qs, [[], []], k=4, fill=FILL)
    assert hits == [[], []] and st["fill_launches"] == 0 and st["cells"] == 0 and all(s.size == 0 for s in scores)
    db.close()


# ---- 4. fall-backs give the same answers ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["blosum62_lq3000", "blosum62_gap_pos1_m3", "pam250_overflow_w", "engine1"])
def test_fall_backs_are_oracle_exact(swg, orc, ctx, case):
    name = "pam250_lq128" if case == "engine1" else case
    g = load_golden(name)
    ctx.set_scoring(g["sub"], int(g["gaps"][0]), int(g["gaps"][1]))
    if case == "engine1":
        ctx.set_option("engine", 1)
    lens = np.diff(g["offsets"].astype(np.int64))
    n = len(lens)
    qs = [swg.synth_query(0xFA11, 40), g["query"].copy(), swg.synth_query(0xFA12, 75)]
    truth = _truth(orc, name, g, qs, tag=case)
    assert np.array_equal(truth[1], g["oracle32"])
    rng = np.random.default_rng(4)
    lists = [rng.choice(n, size=n // 2, replace=False), np.concatenate([np.arange(n), [0, n - 1]]), np.zeros(0, dtype=np.int64)]
    db = swg.Database(g["flat"], g["offsets"]).upload(ctx)
    _check(ctx, db, qs, lists, truth, lens, case, launches=0)
    db.close()


# ---- 5. equivalence with the existing route; the context's own query survives -------------------------------------------
def test_equals_a_view_per_list_and_keeps_the_contexts_query(swg, orc, ctx):
    g = load_golden("pam250_lq128")
    ctx.set_scoring(g["sub"], int(g["gaps"][0]), int(g["gaps"][1]))
    qs = _queries(swg, g)
    lens = np.diff(g["offsets"].astype(np.int64))
    lists = _list_shapes(len(lens), len(qs), lens, np.random.default_rng(5))["shuffled_dups"]
    db = swg.Database(g["flat"], g["offsets"]).upload(ctx)
    ctx.set_query(g["query"])
    scores, hits, st = ctx.search_lists(db, qs, lists, k=12, fill=FILL)
    assert st["fill_launches"] == 1
    s_own, _, _ = ctx.search(db)                             # the context's own query still answers
    assert np.array_equal(s_own, g["oracle32"])
    for i, (q, l) in enumerate(zip(qs, lists)):
        view = db.view(ctx, l)
        ctx.set_query(q)
        s_v, h_v, _ = ctx.search(view, k=12)
        assert h_v == hits[i], i
        assert np.array_equal(scores[i], s_v[np.asarray(l, dtype=np.int64)]), i
        view.close()
    db.close()


# ---- 6. a view as the database ----------------------------------------------------------------------------------------
def test_a_view_as_the_database(swg, orc, ctx):
    g = load_golden("blosum45_lq200")
    ctx.set_scoring(g["sub"], int(g["gaps"][0]), int(g["gaps"][1]))
    qs = _queries(swg, g)
    truth = _truth(orc, "blosum45_lq200", g, qs)
    lens = np.diff(g["offsets"].astype(np.int64))
    n = len(lens)
    inside = np.ones(n, dtype=bool)
    inside[n // 3:2 * n // 3] = False                         # everything but a third
    db = swg.Database(g["flat"], g["offsets"]).upload(ctx)
    view = db.view(ctx, np.nonzero(inside)[0])
    rng = np.random.default_rng(6)
    lists = [rng.choice(n, size=60 + i, replace=False) for i in range(len(qs))]
    lists[2] = np.arange(n // 3, n // 3 + 9)                  # wholly outside the view: nothing written, nothing reported
    _check(ctx, view, qs, lists, truth, lens, "view", held=lambda ix: inside[ix])
    view.close()
    db.close()


def test_a_shard_ignores_what_it_does_not_hold(swg, orc, ctx):
    g = load_golden("pam250_lq128")
    ctx.set_scoring(g["sub"], int(g["gaps"][0]), int(g["gaps"][1]))
    qs = _queries(swg, g)
    truth = _truth(orc, "pam250_lq128", g, qs)
    lens = np.diff(g["offsets"].astype(np.int64))
    n = len(lens)
    rng = np.random.default_rng(7)
    lists = [rng.choice(n, size=80, replace=False) for _ in qs]
    seen = np.zeros((len(qs), n), dtype=int)
    for r in range(3):                                       # every rank passes the same lists
        shard = swg.Database(g["flat"], g["offsets"], shard_rank=r, shard_count=3).upload(ctx)
        mine = np.zeros(n, dtype=bool)
        mine[shard.order()] = True
        _check(ctx, shard, qs, lists, truth, lens, ("shard", r), held=lambda ix: mine[ix])
        for i, l in enumerate(lists):
            seen[i, l[mine[l]]] += 1
        shard.close()
    for i, l in enumerate(lists):
        assert np.all(seen[i, l] == 1)                       # each entry scored by exactly one rank


# ---- 7. PSSMs -----------------------------------------------------------------------------------------------------------
def test_pssm_lists(swg, orc, ctx):
    g = load_golden("pam250_lq128")
    go, ge = int(g["gaps"][0]), int(g["gaps"][1])
    ctx.set_scoring(g["sub"], go, ge)
    qs = _queries(swg, g)
    lens = np.diff(g["offsets"].astype(np.int64))
    n = len(lens)
    rng = np.random.default_rng(8)
    lists = [rng.choice(n, size=50 + 3 * i, replace=True) for i in range(len(qs))]
    db = swg.Database(g["flat"], g["offsets"]).upload(ctx)
    sub = np.asarray(g["sub"], dtype=np.int8)
    a = ctx.search_lists(db, qs, lists, k=9, fill=FILL)
    b = ctx.search_lists_pssm(db, [sub[q.astype(np.int64)] for q in qs], lists, k=9, fill=FILL)
    assert all(np.array_equal(x, y) for x, y in zip(a[0], b[0])) and a[1] == b[1]
    assert a[2]["fill_launches"] == b[2]["fill_launches"] == 1 and a[2]["cells"] == b[2]["cells"]
    # random int8 PSSMs of at most 31 distinct columns: index queries over a table of their own, which the oracle takes
    pssms, truth = [], []
    for i, lq in enumerate((17, 40, 96)):
        p, qp, subp = _pssm31(rng, lq, lo=-20, hi=12)
        pssms.append(p)
        truth.append(orc.score_db(qp, g["flat"], g["offsets"], subp, go, ge))
    _check(ctx, db, pssms, lists[:3], np.stack(truth), lens, "pssm31", search=ctx.search_lists_pssm)
    db.close()


# ---- 8. into alignment ------------------------------------------------------------------------------------------------
def test_hits_go_into_align_hits_multi(swg, ctx):
    g = load_golden("blosum45_lq200")
    ctx.set_scoring(g["sub"], int(g["gaps"][0]), int(g["gaps"][1]))
    qs = _queries(swg, g)[1:]                                 # (a one-residue query aligns too, but says little)
    n = len(g["offsets"]) - 1
    rng = np.random.default_rng(9)
    lists = [rng.choice(n, size=30, replace=False) for _ in qs]
    lists[4] = np.zeros(0, dtype=np.int64)
    db = swg.Database(g["flat"], g["offsets"]).upload(ctx)
    _, hits, st = ctx.search_lists(db, qs, lists, k=6, want_scores=False)
    assert st["fill_launches"] == 1 and [len(h) for h in hits] == [6, 6, 6, 6, 0, 6, 6]
    alns = ctx.align_hits_multi(db, qs, hits, want_ops=False)
    for h_row, a_row in zip(hits, alns):
        assert [(a["score"], a["index"]) for a in a_row] == h_row
    db.close()


# ---- 9. arguments -----------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing(swg, ctx):
    import ctypes as C
    g = load_golden("blosum62_tiny_db")
    ctx.set_scoring(g["sub"], int(g["gaps"][0]), int(g["gaps"][1]))
    n = len(g["offsets"]) - 1
    db = swg.Database(g["flat"], g["offsets"]).upload(ctx)
    q = swg.synth_query(3, 12)
    vp = C.c_void_p

    def call(queries, qoff, lists, coff, k=0, topk=None, database=db):
        qf = np.ascontiguousarray(queries, dtype=np.int8)
        qo = np.asarray(qoff, dtype=np.uint64)
        cf = np.ascontiguousarray(lists if len(lists) else [0], dtype=np.uint32)
        co = np.asarray(coff, dtype=np.uint64)
        scores = np.full(max(int(co[-1]), 1), FILL, dtype=np.int32)
        st = swg.Stats()
        rc = swg.lib.swg_search_lists(ctx.handle, database.handle, qf.ctypes.data_as(vp), qo.ctypes.data_as(vp), len(qo) - 1,
                                      cf.ctypes.data_as(vp), co.ctypes.data_as(vp), scores.ctypes.data_as(vp), topk, k, None, C.byref(st))
        assert np.all(scores == FILL) and st.fill_launches == 0          # nothing was launched, nothing written
        return rc, swg.lib.swg_last_error(ctx.handle).decode()

    rc, msg = call(q, [0, 12], [1, 2], [0, 2], k=3, topk=None)
    assert rc == swg.SWG_ERR_ARG and "topk_out" in msg
    rc, msg = call(q, [0, 12, 12], [1, 2], [0, 1, 2])
    assert rc == swg.SWG_ERR_ARG and "query 1 is empty" in msg
    bad = q.copy()
    bad[5] = 0
    rc, msg = call(bad, [0, 12], [1], [0, 1])
    assert rc == swg.SWG_ERR_RESIDUE and "outside 1..31" in msg
    rc, msg = call(np.concatenate([q, q]), [0, 12, 24], [1, 2, n], [0, 1, 3])
    assert rc == swg.SWG_ERR_ARG and "query 1" in msg and "entry 1" in msg and "outside the database" in msg
    cold = swg.Database(g["flat"], g["offsets"])                          # packed, never uploaded
    rc, msg = call(q, [0, 12], [1], [0, 1], database=cold)
    assert rc == swg.SWG_ERR_STATE and "not resident" in msg
    cold.close()
    ctx.set_query(g["query"])
    ticket = ctx.search_begin(db, k=1)
    rc, msg = call(q, [0, 12], [1], [0, 1])
    assert rc == swg.SWG_ERR_STATE and "in flight" in msg
    ctx.search_end(ticket)
    scores, hits, st = ctx.search_lists(db, [q], [[1]], k=1)              # (and the same call once nothing is in flight)
    assert st["fill_launches"] == 1 and len(hits[0]) == 1
    db.close()
