"""GPU (-m gpu): every hit at or above a caller's score (swg_search_above, swg_search_gapless_above; DESIGN 4.2.1,
"A caller's threshold"), on the databases of test_gpu_prune.py.

What a search_above returns must be the oracle's answer -- n_total = the sequences whose score is at least T, the hits
those sequences in the library's order -- with pruning off (option prune = 0) and on wherever it is structurally possible
(prune = 2: the fill is cut at T from its first launch on), through every geometry and 16-bit cell form, for thresholds
from above the best score down to 1.  Under prune = 2 the pairs a search left out are exactly the pairs whose bound (the
host mirrors') is below T, in every stage, the first and the only one included."""
import ctypes as C

import numpy as np
import pytest

import gapless_cases as gc
from test_gpu_parity import _reset_options
from test_gpu_prune import FORMS, GE, GEOMETRIES, GO, N, _case, _expected, _segment_blocks
from test_gpu_prune import data  # noqa: F401  (the module's databases and oracle scores, as a fixture of this module)
from test_gpu_prune_kmer import _pair_sequences

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _options(ctx):
    def reset():
        _reset_options(ctx)
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


def _above(truth, members, T):
    """The oracle's answer: the members that score at least T, higher score first, ties by lower index."""
    members = np.asarray(members, dtype=np.int64)
    return [(-s, i) for s, i in sorted((-int(truth[i]), int(i)) for i in members if truth[i] >= T)]


def _thresholds(truth, members):
    """From the truth: above the best (no hit), the best, the 10th best (its ties come along), the median, and 1."""
    s = np.sort(np.asarray(truth)[np.asarray(members, dtype=np.int64)])
    return [int(s[-1]) + 1, int(s[-1]), int(s[-10]), max(1, int(s[len(s) // 2])), 1]


def _both_ways(ctx, db, truth, members, label, thresholds=None, want_skips=False, pruned=True, gapless=False):
    """search_above under prune = 0 and prune = 2 for every threshold: both the oracle's answer."""
    skipped = 0
    st = None
    for T in thresholds or _thresholds(truth, members):
        want = _above(truth, members, T)
        for mode in (0, 2):
            ctx.set_option("prune", mode)
            hits, n_total, st = ctx.search_above(db, T, gapless=gapless)
            info = ctx.prune_last()
            assert n_total == len(want), (label, T, mode, n_total, len(want), info)
            assert hits == want, (label, T, mode, info, hits[:5], want[:5])
            assert info["pruned"] == (mode == 2 and pruned), (label, T, mode, info)
            if info["pruned"]:
                assert info["threshold"] == T, (label, T, info)
                assert info["pair_rows_skipped"] <= info["pair_rows"] and (info["pairs_skipped"] > 0) == (info["pair_rows_skipped"] > 0), (label, info)
                skipped = max(skipped, info["pairs_skipped"])
            else:
                assert info["pairs_skipped"] == 0 and info["pair_rows_skipped"] == 0, (label, info)
    if want_skips:
        assert skipped > 0, label
    return st


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_hits_equal_the_oracle_pruned_and_not(swg, ctx, data, geometry, form):
    flat, off, q, sub, truth = _case(data, geometry, form)
    ctx.set_scoring(sub, GO, GE)
    ctx.set_query(q)
    for key, v in {**GEOMETRIES[geometry](off), **FORMS[form][0]}.items():
        ctx.set_option(key, v)
    db = swg.Database(flat, off).upload(ctx)
    ths = _thresholds(truth, np.arange(N))
    assert len(_above(truth, np.arange(N), ths[2])) >= 10 and len(_above(truth, np.arange(N), ths[0])) == 0
    st = _both_ways(ctx, db, truth, np.arange(N), (geometry, form), thresholds=ths, want_skips=True)
    assert st["cell_form"] in FORMS[form][1] and st["engine"] == 2 and st["work_queue"] == 1, (geometry, form, st)
    if geometry.startswith("four_passes") and len(q) == 200:
        assert st["passes"] == 4, st
    if geometry == "four_passes_segments":
        assert st["fill_launches"] >= 5 * st["passes"], st              # (five stages at least)
    if geometry == "last_pass_28":
        assert st["passes"] == 2 and st["last_pass_cols"] == 28, st
    db.close()


@pytest.mark.parametrize("geometry", ["one_pass", "four_passes_segments"])
def test_flags_behind_a_cut(swg, ctx, data, geometry):
    """Database B on the f16 cells with T above their ceiling of 4096: the pairs kept are flagged and run again on the
    int16 cells, the pairs cut were never filled -- and under the table times 8, on the wide form, T above 32767: the int32
    level behind a cut."""
    flat, off = data["B"]
    db = swg.Database(flat, off).upload(ctx)
    for sub, truth, T, opts, forms in ((data["sub"], data["truthB"], 4097, {"f16": 2}, (2,)), (data["sub8"], data["truthB8"], 32768, {"f16": 0}, (1,))):
        ctx.set_scoring(sub, GO, GE)
        ctx.set_query(data["qB"])
        for key, v in {**GEOMETRIES[geometry](off), **opts}.items():
            ctx.set_option(key, v)
        want = _above(truth, np.arange(N), T)
        assert 10 <= len(want) < N // 10
        st = _both_ways(ctx, db, truth, np.arange(N), ("flags", geometry, T), thresholds=[T, int(np.sort(truth)[-10])], want_skips=True)
        assert st["cell_form"] in forms and (st["n_rescored"] >= 10 or forms == (1,)), st    # (the wide form holds scores to 65535)
    db.close()


def _stage_check(ctx, db, bound, T, label):
    """The stages of the search last ended against the mirror's pair bounds: together they cover the fill's pairs from the
    first on, each one's list is the ids of its pairs whose bound reaches T, and swg_prune_last counts the others.
    -> (stages, pairs skipped)"""
    got = ctx.debug_prune_refine_read(db)
    info = ctx.prune_last()
    n = len(bound)
    full = np.zeros(got["pairs"], dtype=np.int64)                        # (the pair of two empty slots: bound 0)
    full[:n] = bound
    assert got["stages"] and got["stages"][0][0] == 0, label
    at = skipped = 0
    for begin, end, t, lst in got["stages"]:
        assert begin == at and end > begin and t == T, (label, begin, end, t, at)
        at = end
        want = begin + np.flatnonzero(full[begin:end] >= T)
        assert np.array_equal(lst.astype(np.int64), want), (label, begin, end, len(lst), len(want))
        skipped += end - begin - len(want)
    assert n <= at <= got["pairs"], (label, at, n, got["pairs"])
    assert skipped == int(np.sum(full[:at] < T))
    assert info["pruned"] and info["threshold"] == T and info["pairs_skipped"] == skipped, (label, info, skipped)
    return got["stages"], skipped


@pytest.mark.parametrize("geometry", ["one_pass", "four_passes_segments"])
def test_pairs_skipped_are_the_pairs_below_the_threshold(swg, ctx, data, geometry):
    """The accounting identity.  T is fixed, so a search skips exactly the pairs whose final bound is below it: under the
    colmax bound the pairs with max(U_x, U_y) < T, under the k-mer bound of k = 4 in 8 segments the same of its mirror,
    and behind a second level of 64 segments at least as many as its first level alone."""
    flat, off = data["A"]
    truth, sub, q = data["truthA"], data["sub"], data["qA"]
    ctx.set_scoring(sub, GO, GE)
    ctx.set_query(q)
    db = swg.Database(flat, off).upload(ctx)
    order = np.array([int(v) for v in db.order()], dtype=np.int64)
    assert len(order) == N
    T = int(np.sort(truth)[-10])
    _, u = swg.debug_prune_bound(sub, q, flat, off)
    u = u.astype(np.int64)
    colmax = np.maximum(u[order[0::2]], u[order[1::2]])
    pflat, poff = _pair_sequences(db, flat, off)
    _, u8 = swg.debug_prune_kmer_seg(sub, q, GO, GE, 4, 8, pflat, poff, table=False)
    kmer = np.maximum(u8[0::2], u8[1::2]).astype(np.int64)
    # on the CPU first: neither case can pass with nothing or with everything skipped
    for b in (colmax, kmer):
        assert 0 < int(np.sum(b < T)) < len(b), (T, int(np.sum(b < T)))
    assert np.all(kmer <= colmax)
    want = _above(truth, np.arange(N), T)
    for key, v in GEOMETRIES[geometry](off).items():
        ctx.set_option(key, v)
    ctx.set_option("prune", 2)
    first_level = {}
    for name, bound, opts in (("colmax", colmax, {"prune_kmer": 1, "prune_refine": 1}),
                              ("kmer", kmer, {"prune_kmer": 4, "prune_segments": 8, "prune_refine": 1})):
        for key, v in opts.items():
            ctx.set_option(key, v)
        hits, n_total, st = ctx.search_above(db, T)
        assert hits == want and n_total == len(want), (geometry, name)
        stages, skipped = _stage_check(ctx, db, bound, T, (geometry, name))
        info = ctx.prune_last()
        assert 0 < info["pair_rows_skipped"] < info["pair_rows"], info
        first_level[name] = skipped
        if geometry == "one_pass":
            # one segment: one stage, the first and only one, and it is cut
            assert len(stages) == 1 and st["fill_launches"] == st["passes"] and skipped > 0, (stages[0][:3], st)
        else:
            assert len(stages) >= 5, (len(stages), geometry)
    ctx.set_option("prune_kmer", 4)
    ctx.set_option("prune_segments", 8)
    ctx.set_option("prune_refine", 64)
    hits, n_total, _ = ctx.search_above(db, T)
    info = ctx.prune_last()
    assert hits == want and info["pruned"] and info["pairs_skipped"] >= first_level["kmer"], (info, first_level)
    db.close()


def test_capacity(swg, ctx, data):
    flat, off = data["A"]
    truth = data["truthA"]
    ctx.set_scoring(data["sub"], GO, GE)
    ctx.set_query(data["qA"])
    db = swg.Database(flat, off).upload(ctx)
    T = int(np.sort(truth)[-10])
    want = _above(truth, np.arange(N), T)
    assert len(want) > 3
    for mode in (0, 2):
        ctx.set_option("prune", mode)
        # a pure count: cap 0 with no room at all
        nh, nt = C.c_size_t(9), C.c_uint64(0)
        assert swg.lib.swg_search_above(ctx.handle, db.handle, T, None, 0, C.byref(nh), C.byref(nt), None) == swg.SWG_OK
        assert (nh.value, nt.value) == (0, len(want))
        assert ctx.search_above(db, T, cap=0)[:2] == ([], len(want))
        # less room than hits: the best three, the count unchanged
        hits, n_total, _ = ctx.search_above(db, T, cap=3)
        assert hits == want[:3] and n_total == len(want), mode
        hits, n_total, _ = ctx.search_above(db, T, cap=len(want))
        assert hits == want and n_total == len(want), mode
        # room but no buffer
        assert swg.lib.swg_search_above(ctx.handle, db.handle, T, None, 5, C.byref(nh), C.byref(nt), None) == swg.SWG_ERR_ARG
    db.close()


def test_more_hits_than_the_key_buffers_floor(swg, ctx, orc):
    """9000 short sequences, nearly every one of which scores: T = 1 counts more than the 8192 keys the read-out starts
    with, so the first search selects from the score array and the buffer grows; the next ones read their keys from the
    device.  Every hit is checked, each time, and then with room for one more than the floor."""
    rng = np.random.default_rng(0x5EED0C01)
    q = swg.synth_query(0x5EED0C02, 64)
    lens = rng.integers(20, 41, size=9000)
    flat = rng.integers(1, 21, size=int(lens.sum())).astype(np.int8)
    off = np.zeros(len(lens) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens)
    sub = np.asarray(swg.load_scoring("BLOSUM62").table(), dtype=np.int8).reshape(32, 32)
    truth = orc.score_db(q, flat, off, sub, GO, GE)
    want = _above(truth, np.arange(9000), 1)
    assert len(want) > 8192
    ctx.set_scoring(sub, GO, GE)
    ctx.set_query(q)
    db = swg.Database(flat, off).upload(ctx)
    # little room, before the buffer has grown: the keys the device dropped are any of them, the best three are still found
    hits, n_total, _ = ctx.search_above(db, 1, cap=3)
    assert n_total == len(want) and hits == want[:3]
    db.close()
    db = swg.Database(flat, off).upload(ctx)
    assert ctx.search_above(db, 1, cap=0)[:2] == ([], len(want))          # (a count alone needs no keys; the buffer grows)
    for mode in (1, 1, 2, 0):
        ctx.set_option("prune", mode)
        hits, n_total, _ = ctx.search_above(db, 1)
        assert n_total == len(want) and hits == want, mode
    hits, n_total, _ = ctx.search_above(db, 1, cap=8193)
    assert n_total == len(want) and hits == want[:8193]
    T = int(np.sort(truth)[-100])
    assert ctx.search_above(db, T)[:2] == (_above(truth, np.arange(9000), T), len(_above(truth, np.arange(9000), T)))
    db.close()


@pytest.mark.parametrize("dbkind", ["plain", "view", "shards"])
@pytest.mark.parametrize("kind", ["index", "pssm"])
def test_query_kinds_and_databases(swg, ctx, data, kind, dbkind):
    flat, off = data["A"]
    truth = data["truthA"]
    ctx.set_scoring(data["sub"], GO, GE)
    if kind == "pssm":
        ctx.set_query_pssm(data["sub"][data["qA"].astype(np.int64)])
    else:
        ctx.set_query(data["qA"])
    for key, v in GEOMETRIES["four_passes_segments"](off).items():
        ctx.set_option(key, v)
    ths = [int(np.sort(truth)[-10]), int(np.sort(truth)[N // 2])]
    if dbkind == "plain":
        db = swg.Database(flat, off).upload(ctx)
        _both_ways(ctx, db, truth, np.arange(N), (kind, dbkind), thresholds=ths, want_skips=True)
        db.close()
    elif dbkind == "view":
        want = np.delete(np.arange(N), np.arange(0, N, 3))
        parent = swg.Database(flat, off).upload(ctx)
        db = parent.view(ctx, want)
        ctx.set_option("segment_blocks", _segment_blocks(off, members=want))
        _both_ways(ctx, db, truth, want, (kind, dbkind), thresholds=ths, want_skips=True)
        db.close()
        parent.close()
    else:
        # two shards of one database: each gives its own hits, and the union sorted by swg_hit_key is the oracle's list
        o64 = off.astype(np.int64)
        for mode in (0, 2):
            merged = {T: [] for T in ths}
            totals = {T: 0 for T in ths}
            for part in (np.arange(0, N, 2), np.arange(1, N, 2)):
                loc = np.concatenate([flat[o64[i]:o64[i + 1]] for i in part]).astype(np.int8)
                loff = np.zeros(len(part) + 1, dtype=np.uint64)
                loff[1:] = np.cumsum(np.diff(o64)[part])
                db = swg.Database(loc, loff, index=part.astype(np.uint32), n_total=N).upload(ctx)
                ctx.set_option("segment_blocks", _segment_blocks(off, members=part))
                ctx.set_option("prune", mode)
                for T in ths:
                    hits, n_total, _ = ctx.search_above(db, T)
                    assert hits == _above(truth, part, T) and n_total == len(hits), (kind, mode, T)
                    assert ctx.prune_last()["pruned"] == (mode == 2)
                    merged[T] += hits
                    totals[T] += n_total
                db.close()
            for T in ths:
                keys = sorted((swg.lib.swg_hit_key(s, i) for s, i in merged[T]), reverse=True)
                assert [(k >> 32, 0xFFFFFFFF - (k & 0xFFFFFFFF)) for k in keys] == _above(truth, np.arange(N), T), (kind, mode, T)
                assert totals[T] == len(keys)


@pytest.mark.parametrize("route", ["positive_gaps", "force_bits_32", "engine_1"])
def test_routes_the_plan_refuses_run_unpruned_and_exact(swg, ctx, data, orc, route):
    flat, off = data["A"]
    q, sub = data["qA"], data["sub"]
    if route == "positive_gaps":
        # a positive gap extension on a small part of A (scores grow with every gap: the int32 path)
        part = np.arange(0, N, 20)
        o64 = off.astype(np.int64)
        flat = np.concatenate([flat[o64[i]:o64[i + 1]] for i in part]).astype(np.int8)
        off = np.concatenate([[0], np.cumsum(np.diff(o64)[part])]).astype(np.uint64)
        gaps = (-3, 1)
        truth = orc.score_db(q, flat, off, sub, *gaps)
    else:
        gaps = (GO, GE)
        truth = data["truthA"]
        ctx.set_option("force_bits" if route == "force_bits_32" else "engine", 32 if route == "force_bits_32" else 1)
    ctx.set_scoring(sub, *gaps)
    ctx.set_query(q)
    db = swg.Database(flat, off).upload(ctx)
    n = len(truth)
    st = _both_ways(ctx, db, truth, np.arange(n), route, thresholds=[int(np.sort(truth)[-10]), max(1, int(np.sort(truth)[n // 2])), 1], pruned=False)
    if route == "force_bits_32" or route == "positive_gaps":
        assert st["path_bits"] == 32, st
    if route == "engine_1":
        assert st["engine"] == 1, st
    db.close()


def test_gapless_above_is_exact_and_never_pruned(swg, ctx, data, orc):
    flat, off = data["A"]
    q, sub = data["qA"], data["sub"]
    truth = gc.oracle_gapless(orc, q, flat, off, sub)
    ctx.set_scoring(sub, GO, GE)
    ctx.set_query(q)
    db = swg.Database(flat, off).upload(ctx)
    for opts in ({}, GEOMETRIES["four_passes_segments"](off)):
        for key, v in opts.items():
            ctx.set_option(key, v)
        _both_ways(ctx, db, truth, np.arange(N), ("gapless", opts), pruned=False, gapless=True)
    # ... and its answer is the gapless top-K's head
    T = int(np.sort(truth)[-10])
    hits, n_total, _ = ctx.search_above(db, T, gapless=True)
    assert hits == gc.expected_hits(truth, n_total) and hits == ctx.search_gapless(db, want_scores=False, k=n_total)[1]
    db.close()


def test_state(swg, ctx, data):
    """A pruned top-K search right after a search_above on the same context and database gives its usual hits, and the
    reverse; min_score below 1 is an argument error; a search in flight a state error, and it still ends well."""
    flat, off = data["A"]
    truth = data["truthA"]
    ctx.set_scoring(data["sub"], GO, GE)
    ctx.set_query(data["qA"])
    for key, v in GEOMETRIES["four_passes_segments"](off).items():
        ctx.set_option(key, v)
    ctx.set_option("prune", 2)
    db = swg.Database(flat, off).upload(ctx)
    T = int(np.sort(truth)[-10])
    want = _above(truth, np.arange(N), T)
    for k in (100, 10):
        hits, n_total, _ = ctx.search_above(db, T)
        assert hits == want and ctx.prune_last()["threshold"] == T
        _, top, _ = ctx.search(db, want_scores=False, k=k)
        info = ctx.prune_last()
        assert top == _expected(truth, np.arange(N), k) and info["pruned"], (k, info)
    hits, n_total, _ = ctx.search_above(db, T)
    assert hits == want and n_total == len(want) and ctx.prune_last()["pruned"]
    nh, nt = C.c_size_t(0), C.c_uint64(0)
    hit = (swg.Hit * 4)()
    for bad in (0, -1, -(1 << 31)):
        for fn in (swg.lib.swg_search_above, swg.lib.swg_search_gapless_above):
            assert fn(ctx.handle, db.handle, bad, C.cast(hit, C.c_void_p), 4, C.byref(nh), C.byref(nt), None) == swg.SWG_ERR_ARG, bad
            assert b"min_score" in swg.lib.swg_last_error(ctx.handle)
    with pytest.raises(swg.SwgError) as e:
        ctx.search_above(db, 0)
    assert e.value.code == swg.SWG_ERR_ARG
    t = ctx.search_begin(db, k=10)
    for gapless in (False, True):
        with pytest.raises(swg.SwgError) as e:
            ctx.search_above(db, T, gapless=gapless)
        assert e.value.code == swg.SWG_ERR_STATE
    _, top, _ = ctx.search_end(t)
    assert top == _expected(truth, np.arange(N), 10)
    assert ctx.search_above(db, T)[0] == want
    db.close()
