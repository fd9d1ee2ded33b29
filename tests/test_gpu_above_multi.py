"""GPU (-m gpu): every hit at or above a score, per query of a batch (swg_search_above_multi and its PSSM and gapless
forms; DESIGN 4.2.1, "A caller's threshold, per query of a batch"), on the inputs of tests/above_multi_cases.py.

Row i of a call must be what set_query(query i) + search_above(min_scores[i]) gives, which is the oracle's answer: n_total
the sequences that score at least min_scores[i], the hits those sequences in the library's order.  Both routes -- the one
launch per class with the per-row read-out on the device (option above_batch = 1), and one query after another
(above_batch = 2), unpruned and pruned -- give it, for index and PSSM queries, plain databases, views and shards, through
every capacity, and the route taken is pinned from swg_stats and swg_prune_last."""
import ctypes as C

import numpy as np
import pytest

import above_multi_cases as amc
import gapless_cases as gc
import instantiation_cases as ic
from test_gpu_parity import _reset_options

pytestmark = pytest.mark.gpu

N, GO, GE = amc.N, amc.GO, amc.GE
ROUTES = {"one_launch": {"above_batch": 1}, "one_by_one": {"above_batch": 2, "prune": 0}, "one_by_one_pruned": {"above_batch": 2, "prune": 2}}
VP = C.c_void_p


@pytest.fixture(autouse=True)
def _options(ctx):
    def reset():
        _reset_options(ctx)
        ctx.set_option("above_batch", 0)
        ctx.set_option("prune", 1)
        ctx.set_option("prune_head", 4)
        ctx.set_option("prune_kmer", 0)
        ctx.set_option("prune_segments", 0)
        ctx.set_option("prune_refine", 0)
        ctx.set_option("prune_cut", 0)

    reset()
    ctx.set_option("autotune", 0)
    yield
    reset()
    ctx.set_option("autotune", 1)


@pytest.fixture(scope="module")
def data(swg, orc):
    """Database A, the five queries and every oracle score the module needs, computed once and left unchanged."""
    sub = amc.table(swg)
    flat, off, qA = amc.database(swg)
    qs = amc.queries(swg, qA)
    truths = [orc.score_db(q, flat, off, sub, GO, GE) for q in qs]
    gapless = [gc.oracle_gapless(orc, q, flat, off, sub) for q in qs]
    for t in truths + gapless:
        t.setflags(write=False)
    return dict(sub=sub, flat=flat, off=off, qs=qs, pssms=amc.pssms(sub, qs), truths=truths, T=amc.level_table(truths), gapless=gapless,
                TG=amc.level_table(gapless))


def _set(ctx, opts):
    for key, v in opts.items():
        ctx.set_option(key, v)


def _call(ctx, db, data, kind, min_scores, cap=None, gapless=False, sel=None):
    sel = range(len(data["qs"])) if sel is None else sel
    if kind == "pssm":
        return ctx.search_above_multi_pssm(db, [data["pssms"][i] for i in sel], min_scores, cap=cap, gapless=gapless)
    return ctx.search_above_multi(db, [data["qs"][i] for i in sel], min_scores, cap=cap, gapless=gapless)


def _pin_route(ctx, route, st, label, want_skips=True):
    info = ctx.prune_last()
    if route == "one_launch":
        assert st["fill_launches"] >= 1 and st["cell_form"] in (3, 2, 0) and not info["pruned"], (label, st, info)
        assert info["pairs_skipped"] == 0 and info["pair_rows"] == 0, (label, info)
    elif route == "one_by_one":
        assert st["fill_launches"] == 0 and not info["pruned"] and info["pairs_skipped"] == 0, (label, st, info)
    else:
        assert st["fill_launches"] == 0 and info["pruned"], (label, st, info)
        assert info["pair_rows_skipped"] <= info["pair_rows"], (label, info)
        if want_skips:
            assert info["pairs_skipped"] > 0, (label, info)
    return info


def _levels(T):
    """The six calls: the five levels, and the mixed one in which query i takes level i."""
    return [(amc.LEVELS[l], [t[l] for t in T]) for l in range(len(amc.LEVELS))] + [("mixed", amc.mixed(T))]


# ---- 1. routes x query kinds -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["index", "pssm"])
@pytest.mark.parametrize("route", list(ROUTES))
def test_rows_equal_the_oracle_on_every_route(swg, ctx, data, route, kind):
    ctx.set_scoring(data["sub"], GO, GE)
    db = swg.Database(data["flat"], data["off"]).upload(ctx)
    _set(ctx, ROUTES[route])
    for name, ms in _levels(data["T"]):
        hits, n_total, st = _call(ctx, db, data, kind, ms)
        for i, truth in enumerate(data["truths"]):
            want = amc.above(truth, ms[i])
            assert n_total[i] == len(want), (route, kind, name, i, n_total[i], len(want))
            assert hits[i] == want, (route, kind, name, i, hits[i][:5], want[:5])
        info = _pin_route(ctx, route, st, (route, kind, name), want_skips=name in ("above_best", "best", "tenth", "mixed"))
        assert info["threshold"] == ms[-1], (route, kind, name, info)
    db.close()


# ---- 2. the batch in reversed order ----------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["one_launch", "one_by_one_pruned"])
def test_reversed_batch_gives_reversed_rows(swg, ctx, data, route):
    ctx.set_scoring(data["sub"], GO, GE)
    db = swg.Database(data["flat"], data["off"]).upload(ctx)
    _set(ctx, ROUTES[route])
    ms = [t[2] for t in data["T"]]
    sel = list(range(5))[::-1]
    hits, n_total, st = _call(ctx, db, data, "index", [ms[i] for i in sel], sel=sel)
    _pin_route(ctx, route, st, route)
    for row, i in enumerate(sel):
        want = amc.above(data["truths"][i], ms[i])
        assert hits[row] == want and n_total[row] == len(want), (route, row, i)
    # and an even batch (no query is paired with itself): the first four
    hits, n_total, _ = _call(ctx, db, data, "index", ms[:4], sel=range(4))
    assert hits == [amc.above(data["truths"][i], ms[i]) for i in range(4)]
    db.close()


# ---- 3. capacity and layout ------------------------------------------------------------------------------------------
def _raw(swg, ctx, db, data, ms, cap, hits_buf, sentinel=None):
    qs = data["qs"]
    qoff = np.zeros(len(qs) + 1, dtype=np.uint64)
    qoff[1:] = np.cumsum([len(q) for q in qs])
    qflat = np.ascontiguousarray(np.concatenate(qs), dtype=np.int8)
    msa = np.ascontiguousarray(ms, dtype=np.int32)
    nh = np.full(len(qs), 99, dtype=np.uintp)
    nt = np.full(len(qs), 99, dtype=np.uint64)
    rc = swg.lib.swg_search_above_multi(ctx.handle, db.handle, qflat.ctypes.data_as(VP), qoff.ctypes.data_as(VP), len(qs), msa.ctypes.data_as(VP),
                                        hits_buf.ctypes.data_as(VP) if hits_buf is not None else None, cap, nh.ctypes.data_as(VP),
                                        nt.ctypes.data_as(VP), None)
    return rc, nh, nt


@pytest.mark.parametrize("route", ["one_launch", "one_by_one_pruned"])
def test_capacity_and_layout(swg, ctx, data, route):
    ctx.set_scoring(data["sub"], GO, GE)
    db = swg.Database(data["flat"], data["off"]).upload(ctx)
    _set(ctx, ROUTES[route])
    ms = [t[2] for t in data["T"]]
    wants = [amc.above(t, m) for t, m in zip(data["truths"], ms)]
    counts = [len(w) for w in wants]
    assert counts == [10, 10, 3795, 10, 10]
    # a pure count: cap 0 and no room at all
    rc, nh, nt = _raw(swg, ctx, db, data, ms, 0, None)
    assert rc == swg.SWG_OK and not nh.any() and nt.tolist() == counts, (route, nt)
    hits, n_total, _ = _call(ctx, db, data, "index", ms, cap=0)
    assert hits == [[]] * 5 and n_total == counts
    # less room than hits: the best three per row, the counts unchanged
    hits, n_total, _ = _call(ctx, db, data, "index", ms, cap=3)
    assert hits == [w[:3] for w in wants] and n_total == counts, route
    # a sentinel survives in every slot past n_hits[i]
    cap = 12
    dt = np.dtype([("score", np.int32), ("index", np.uint32)])
    buf = np.zeros(5 * cap, dtype=dt)
    buf["score"], buf["index"] = -77, 0xABCDEF01
    rc, nh, nt = _raw(swg, ctx, db, data, ms, cap, buf)
    assert rc == swg.SWG_OK and nt.tolist() == counts and nh.tolist() == [min(cap, c) for c in counts]
    for i in range(5):
        row = buf[i * cap:(i + 1) * cap]
        assert list(zip(row["score"][:nh[i]].tolist(), row["index"][:nh[i]].tolist())) == wants[i][:cap], (route, i)
        assert np.all(row["score"][nh[i]:] == -77) and np.all(row["index"][nh[i]:] == 0xABCDEF01), (route, i)
    # room but no buffer; a threshold below 1 names its query
    rc, nh, nt = _raw(swg, ctx, db, data, ms, 5, None)
    assert rc == swg.SWG_ERR_ARG and not nh.any() and not nt.any()
    bad = list(ms)
    bad[2] = 0
    rc, nh, nt = _raw(swg, ctx, db, data, bad, cap, buf)
    assert rc == swg.SWG_ERR_ARG and not nh.any() and not nt.any()
    assert b"query 2" in swg.lib.swg_last_error(ctx.handle), swg.lib.swg_last_error(ctx.handle)
    # min_scores may be one int for all
    hits, n_total, _ = _call(ctx, db, data, "index", 393, cap=4)
    assert hits == [amc.above(t, 393)[:4] for t in data["truths"]]
    db.close()


def test_no_device_room_for_the_keys_selects_on_the_host(swg, ctx, data):
    """The key pool's growth refused once (test hook): that chunk's score rows go to the host, the answer is the same, and
    the next call grows the pool and reads its keys from the device."""
    ctx.set_scoring(data["sub"], GO, GE)
    db = swg.Database(data["flat"], data["off"]).upload(ctx)
    ctx.set_option("above_batch", 1)
    ms = [1] * 5
    wants = [amc.above(t, 1) for t in data["truths"]]
    assert sum(len(w) for w in wants) == 19995                    # (beyond the 8 192 keys the pool starts with)
    for refuse in (True, False):
        if refuse:
            swg.lib.swg_debug_fail_alloc(4)
        hits, n_total, st = _call(ctx, db, data, "index", ms)
        assert hits == wants and n_total == [len(w) for w in wants] and st["fill_launches"] == 1, refuse
    swg.lib.swg_debug_fail_alloc(4)
    hits, n_total, _ = _call(ctx, db, data, "index", ms, cap=3)
    swg.lib.swg_debug_fail_alloc(0)
    assert hits == [w[:3] for w in wants] and n_total == [len(w) for w in wants]
    db.close()


# ---- 4. two chunks ---------------------------------------------------------------------------------------------------
def test_two_chunks(swg, ctx, orc, data):
    """257 queries of 1 to 64 columns: a chunk of 256 and a chunk of one, each query at its own 10th-best score."""
    flat, off = ic.database()
    assert len(off) - 1 == 151
    rng = np.random.default_rng(0x5EED0C21)
    qs = [rng.choice(np.array(ic.AMINO, dtype=np.int8), size=1 + (i * 7) % 64) for i in range(257)]
    assert {len(q) for q in qs} == set(range(1, 65))
    truths = [orc.score_db(q, flat, off, data["sub"], GO, GE) for q in qs]
    ms = [max(1, int(np.sort(t)[-10])) for t in truths]
    assert len(set(ms)) > 20
    ctx.set_scoring(data["sub"], GO, GE)
    db = swg.Database(flat, off).upload(ctx)
    ctx.set_option("above_batch", 1)
    hits, n_total, st = ctx.search_above_multi(db, qs, ms)
    assert st["fill_launches"] == 2 and not ctx.prune_last()["pruned"], st
    assert n_total == [len(amc.above(t, m)) for t, m in zip(truths, ms)]
    for i in (0, 1, 255, 256):
        assert hits[i] == amc.above(truths[i], ms[i]), i
    db.close()


# ---- 5. a view and two shards ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["one_launch", "one_by_one_pruned"])
def test_view_and_shards(swg, ctx, data, route):
    flat, off = data["flat"], data["off"]
    ctx.set_scoring(data["sub"], GO, GE)
    _set(ctx, ROUTES[route])
    ms = [t[2] for t in data["T"]]
    members = np.delete(np.arange(N), np.arange(0, N, 3))
    parent = swg.Database(flat, off).upload(ctx)
    view = parent.view(ctx, members)
    hits, n_total, st = _call(ctx, view, data, "index", ms)
    _pin_route(ctx, route, st, (route, "view"))
    for i, truth in enumerate(data["truths"]):
        want = amc.above(truth, ms[i], members)
        assert hits[i] == want and n_total[i] == len(want), (route, "view", i)
    assert hits[0] != amc.above(data["truths"][0], ms[0])          # (the view's answer is its own)
    view.close()
    parent.close()
    o64 = off.astype(np.int64)
    merged, totals = [[] for _ in range(5)], [0] * 5
    for part in (np.arange(0, N, 2), np.arange(1, N, 2)):
        loc = np.concatenate([flat[o64[i]:o64[i + 1]] for i in part]).astype(np.int8)
        loff = np.zeros(len(part) + 1, dtype=np.uint64)
        loff[1:] = np.cumsum(np.diff(o64)[part])
        db = swg.Database(loc, loff, index=part.astype(np.uint32), n_total=N).upload(ctx)
        hits, n_total, st = _call(ctx, db, data, "index", ms)
        _pin_route(ctx, route, st, (route, "shard"))
        for i, truth in enumerate(data["truths"]):
            assert hits[i] == amc.above(truth, ms[i], part) and n_total[i] == len(hits[i]), (route, "shard", i)
            merged[i] += hits[i]
            totals[i] += n_total[i]
        db.close()
    for i, truth in enumerate(data["truths"]):
        keys = sorted((swg.lib.swg_hit_key(s, j) for s, j in merged[i]), reverse=True)
        assert [(k >> 32, 0xFFFFFFFF - (k & 0xFFFFFFFF)) for k in keys] == amc.above(truth, ms[i]), (route, i)
        assert totals[i] == len(keys)


# ---- 6. what the launch refuses --------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["long_query", "positive_gap", "force_bits_32", "beyond_int16", "one_query"])
def test_what_the_launch_refuses_goes_one_by_one(swg, ctx, orc, data, case):
    """plan_batch's refusals -- a query of several passes, gap scores outside the packed form, the int32 path, scores that
    may pass 32 767, a batch of one -- under above_batch 0 and 1: one query after another, exact."""
    part = np.arange(0, N, 10)
    sub, gaps, qs = data["sub"], (GO, GE), list(data["qs"])
    flat, off = data["flat"], data["off"]
    if case == "beyond_int16":
        qB = swg.synth_query(0x5EED0B01, 1000)
        flat, off = swg.synth_db(0x5EED0B02, N, median=60, max_len=1200, query=qB, fraction=0.01, subst=0.05)[:2]
        sub = (sub.astype(np.int32) * 8).astype(np.int8)
        qs = [qB, qB[100:400].copy(), qs[3]]
    elif case == "long_query":
        qs = [qs[1], swg.synth_query(0x5EED0C13, 2500), qs[3]]
    elif case == "positive_gap":
        gaps = (-3, 1)
    elif case == "one_query":
        qs = qs[:1]
    o64 = off.astype(np.int64)
    pflat = np.concatenate([flat[o64[i]:o64[i + 1]] for i in part]).astype(np.int8)
    poff = np.concatenate([[0], np.cumsum(np.diff(o64)[part])]).astype(np.uint64)
    truths = [orc.score_db(q, pflat, poff, sub, *gaps) for q in qs]
    ms = [max(1, int(np.sort(t)[-10])) if i % 2 == 0 else 1 for i, t in enumerate(truths)]
    ctx.set_scoring(sub, *gaps)
    if case == "force_bits_32":
        ctx.set_option("force_bits", 32)
    db = swg.Database(pflat, poff).upload(ctx)
    for option in (0, 1):
        ctx.set_option("above_batch", option)
        hits, n_total, st = ctx.search_above_multi(db, qs, ms)
        assert st["fill_launches"] == 0, (case, option, st)
        for i, truth in enumerate(truths):
            want = amc.above(truth, ms[i])
            assert hits[i] == want and n_total[i] == len(want), (case, option, i)
    db.close()


# ---- 7. the gapless forms --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["index", "pssm"])
def test_gapless_forms(swg, ctx, data, kind):
    ctx.set_scoring(data["sub"], GO, GE)
    db = swg.Database(data["flat"], data["off"]).upload(ctx)
    for opts in ({"above_batch": 0, "prune": 1}, {"above_batch": 1, "prune": 2}):
        _set(ctx, opts)
        for name, ms in _levels(data["TG"]):
            hits, n_total, st = _call(ctx, db, data, kind, ms, gapless=True)
            info = ctx.prune_last()
            assert st["fill_launches"] == 0 and not info["pruned"] and info["pairs_skipped"] == 0, (kind, name, st, info)
            for i, truth in enumerate(data["gapless"]):
                want = amc.above(truth, ms[i])
                assert hits[i] == want and n_total[i] == len(want), (kind, opts, name, i)
    assert [len(h) for h in _call(ctx, db, data, kind, [t[2] for t in data["TG"]], gapless=True)[0]] == [10, 10, 3795, 10, 11]
    db.close()


# ---- 8. the accounting ---------------------------------------------------------------------------------------------
def test_accounting_of_the_pruned_route(swg, ctx, data):
    """pairs_skipped is the sum, over the batch's queries, of the pairs whose colmax bound is below that query's
    threshold; pair_rows is five times one search's; the threshold reported is the last query's."""
    flat, off, sub = data["flat"], data["off"], data["sub"]
    ctx.set_scoring(sub, GO, GE)
    db = swg.Database(flat, off).upload(ctx)
    order = np.array([int(v) for v in db.order()], dtype=np.int64)
    assert len(order) == N
    _set(ctx, {"above_batch": 2, "prune": 2, "prune_kmer": 1, "prune_refine": 1})
    ms = [t[2] for t in data["T"]]
    below = [int((amc.pair_order_bounds(swg, sub, q, flat, off, order) < m).sum()) for q, m in zip(data["qs"], ms)]
    assert below == [1861, 1233, 2, 1, 272]
    ctx.set_query(data["qs"][0])
    ctx.search_above(db, ms[0])
    one = ctx.prune_last()
    assert one["pruned"] and one["pairs_skipped"] == below[0] and one["pair_rows"] > 0, one
    hits, n_total, st = _call(ctx, db, data, "index", ms)
    info = ctx.prune_last()
    assert hits == [amc.above(t, m) for t, m in zip(data["truths"], ms)]
    assert info["pruned"] and info["pairs_skipped"] == sum(below), (info, below)
    assert info["pair_rows"] == 5 * one["pair_rows"] and 0 < info["pair_rows_skipped"] < info["pair_rows"], (info, one)
    assert info["threshold"] == ms[-1] and st["fill_launches"] == 0
    db.close()


# ---- 9. state and pipeline -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["one_launch", "one_by_one_pruned"])
def test_the_contexts_own_query_survives(swg, ctx, orc, data, route):
    flat, off, sub = data["flat"], data["off"], data["sub"]
    own = swg.synth_query(0x5EED0C14, 90)
    truth = orc.score_db(own, flat, off, sub, GO, GE)
    ctx.set_scoring(sub, GO, GE)
    db = swg.Database(flat, off).upload(ctx)
    ms = [t[2] for t in data["T"]]
    for as_pssm in (False, True):
        _set(ctx, {"above_batch": 0, "prune": 1})
        if as_pssm:
            ctx.set_query_pssm(sub[own.astype(np.int64)])
        else:
            ctx.set_query(own)
        before = ctx.search(db, k=10)
        assert np.array_equal(before[0], truth)
        _set(ctx, ROUTES[route])
        for kind in ("index", "pssm"):
            _call(ctx, db, data, kind, ms)
        _set(ctx, {"above_batch": 0, "prune": 1})
        after = ctx.search(db, k=10)
        assert np.array_equal(after[0], truth) and after[1] == before[1], (route, as_pssm)
    db.close()


def test_state_and_option(swg, ctx, data):
    ctx.set_scoring(data["sub"], GO, GE)
    ctx.set_query(data["qs"][0])
    db = swg.Database(data["flat"], data["off"]).upload(ctx)
    ms = [t[2] for t in data["T"]]
    want = [amc.above(t, m) for t, m in zip(data["truths"], ms)]
    t = ctx.search_begin(db, k=10)
    for gapless in (False, True):
        for kind in ("index", "pssm"):
            with pytest.raises(swg.SwgError) as e:
                _call(ctx, db, data, kind, ms, gapless=gapless)
            assert e.value.code == swg.SWG_ERR_STATE
    _, top, _ = ctx.search_end(t)
    assert top == amc.above(data["truths"][0], 1)[:10]
    assert _call(ctx, db, data, "index", ms)[0] == want
    for bad in (3, -1):
        with pytest.raises(swg.SwgError) as e:
            ctx.set_option("above_batch", bad)
        assert e.value.code == swg.SWG_ERR_ARG
    assert _call(ctx, db, data, "index", ms)[0] == want          # (the option kept its value)
    # no queries: nothing to do, nothing written
    assert ctx.search_above_multi(db, [], [])[:2] == ([], [])
    db.close()


@pytest.mark.parametrize("route", ["one_launch", "one_by_one"])
def test_rows_feed_the_multi_aligners(swg, ctx, data, route):
    ctx.set_scoring(data["sub"], GO, GE)
    db = swg.Database(data["flat"], data["off"]).upload(ctx)
    _set(ctx, ROUTES[route])
    ms = [t[2] for t in data["T"]]
    hits, n_total, _ = _call(ctx, db, data, "index", ms, cap=10)
    assert [len(h) for h in hits] == [10] * 5
    stats = ctx.align_stats_multi(db, data["qs"], hits)
    for i, row in enumerate(hits):
        assert [(a["score"], a["index"]) for a in stats[i]] == row, (route, i)
    db.close()
