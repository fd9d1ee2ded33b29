"""GPU (-m gpu): the fifth level of the pruning bound (option prune_refine5) -- the fourth level's walk over
both tables of 5-residue blocks, the query columns jumped over between two blocks charged as a gap.

The device's second table must be the recurrence's entry for entry; after a search under the five levels every pair's
bound must be the least the mirrors give, level by level, each stage's list the pairs whose bound reaches its T and
pairs_skipped their count; the hits must be the oracle's, from a view, a shard and two searches in flight too; and with
the option left automatic on databases of this size the level is not taken."""
import contextlib

import numpy as np
import pytest

from test_gpu_parity import _reset_options
from test_gpu_prune_deep import PRUNE_KEYS, _geometry, _pair_mirrors, _sample_blocks, _set_query, data  # noqa: F401
from test_gpu_prune_kmer import _pair_sequences
from test_prune_adjacent_host import numpy_table5_spans

pytestmark = pytest.mark.gpu

GO, GE = -2, -1
KEYS = PRUNE_KEYS + ("prune_refine5",)


@pytest.fixture(autouse=True)
def _options(ctx):
    def reset():
        _reset_options(ctx)
        ctx.set_option("prune", 1)
        ctx.set_option("prune_head", 4)
        for key in KEYS:
            ctx.set_option(key, 0)

    reset()
    ctx.set_option("autotune", 0)
    yield
    reset()
    ctx.set_option("autotune", 1)


def _sub(swg, name):
    return np.asarray(swg.load_scoring(name).table(), dtype=np.int8).reshape(32, 32)


def _force_levels(ctx, swg, fifth=True, fourth=True):
    ctx.set_option("prune", 2)
    for key, v in (("prune_kmer", 4), ("prune_segments", 32), ("prune_refine", 128), ("prune_refine3", 256),
                   ("prune_refine4", swg.PRUNE_REFINE4_FORCED if fourth else 1), ("prune_refine5", swg.PRUNE_REFINE5_FORCED if fifth else 1)):
        ctx.set_option(key, v)


@pytest.mark.parametrize("lq, gaps", [(37, (-2, -1)), (300, (-11, -1)), (777, (-3, -2))])
def test_the_second_table_equals_the_recurrence(swg, ctx, lq, gaps):
    """lq = 37 leaves 219 of the 256 segments without columns, 300 and 777 are no multiples of 256; 777 is more than three
    of the kernel's chunks of 256 columns."""
    rng = np.random.default_rng(0x5EED0F01 + lq)
    q = swg.synth_query(0x5EED0E02, 777)[:lq].copy()
    sub = _sub(swg, "BLOSUM62")
    cls = _sample_blocks(rng)
    want = numpy_table5_spans(swg, sub, q, gaps, cls)
    flat, off = swg.synth_db(0x5EED0E03, 600, median=40, max_len=200)
    ctx.set_scoring(sub, gaps[0], gaps[1])
    ctx.set_query(q)
    db = swg.Database(flat, off).upload(ctx)
    _force_levels(ctx, swg)
    before = ctx.debug_prune_tables5()
    ctx.search(db, want_scores=False, k=10)
    info = ctx.debug_prune_tables5()
    assert ctx.prune_last()["pruned"] and not info["refused"]
    assert info["refine5"] == 256 and info["bits"] == 8 and info["refine5_builds"] == before["refine5_builds"] + 1
    ix = ((((cls[:, 0] * 22 + cls[:, 1]) * 22 + cls[:, 2]) * 22 + cls[:, 3]) * 22 + cls[:, 4]).astype(np.uint32)
    got = ctx.debug_prune_refine5_read(ix).astype(np.int64)
    assert np.array_equal(got, want), (lq, np.argwhere(got != want)[:3])
    W = -(-lq // 256)
    assert np.any(got[:, (lq - 1) // W]) and not np.any(got[:, (lq - 1) // W + 1:])
    # the fourth level's table stands beside it, and the same search again builds nothing
    assert ctx.debug_prune_tables4()["bits"] == 8
    ctx.search(db, want_scores=False, k=10)
    assert ctx.debug_prune_tables5()["refine5_builds"] == info["refine5_builds"]
    db.close()


def _five_mirrors(swg, data, label, rows, q, gaps, pflat, poff):
    four = _pair_mirrors(swg, data, label, rows, q, gaps, pflat, poff)
    key = label + "/5"
    if key not in data["mirrors"]:
        u = swg.debug_prune_kmer_refine5(rows, q, gaps[0], gaps[1], 256, pflat, poff)
        data["mirrors"][key] = np.maximum(u[0::2], u[1::2]).astype(np.int64)
    return four + [data["mirrors"][key]]


def _expected(stages, n_pairs, mirrors, fixed):
    """What a search leaves, by the rules of the other levels: in a cut stage a pair at or above T is walked again, level by
    level, and keeps the least bound.  -> (bounds, pairs cut by the fifth level alone)"""
    want = mirrors[0].copy()
    cut5 = 0
    for si, (begin, end, T, _) in enumerate(stages):
        p = np.arange(begin, min(end, n_pairs))
        b = mirrors[0][p].copy()
        if fixed and si == 0 and len(stages) > 1 and (int(np.sum(b < T)) + max(0, end - n_pairs)) * 8 < end - begin:
            continue
        for level in (1, 2, 3, 4):
            walk = b >= T
            if level == 4:
                cut5 += int(np.sum(walk & (mirrors[4][p] < T)))
            b[walk] = np.minimum(b[walk], mirrors[level][p][walk])
        want[p] = b
    return want, cut5


def _check(ctx, db, n, mirrors, fixed):
    got = ctx.debug_prune_refine_read(db)
    assert ctx.debug_prune_tables4()["refine4"] == 256 and ctx.debug_prune_tables5()["refine5"] == 256
    b = got["bounds"].astype(np.int64)
    want, cut5 = _expected(got["stages"], n, mirrors, fixed)
    assert np.array_equal(b[:n], want), np.flatnonzero(b[:n] != want)[:5]
    skipped = 0
    for begin, end, T, lst in got["stages"]:
        assert np.array_equal(lst.astype(np.int64), begin + np.flatnonzero(b[begin:end] >= T)), begin
        skipped += (end - begin) - int(np.sum(want[begin:min(end, n)] >= T))     # (an empty slot's pair is skipped too)
    assert ctx.prune_last()["pairs_skipped"] == skipped
    return got, cut5


def test_bounds_are_the_least_of_the_five_mirrors(swg, orc, ctx, data):  # noqa: F811
    """lq = 300 (W = 2) over several launch segments: T rises from stage to stage; then a caller's threshold."""
    flat, off, q = data["flat"], data["off"], data["q"]
    sub = _sub(swg, "BLOSUM62")
    _set_query(ctx, swg, sub, q, (GO, GE))
    db = swg.Database(flat, off).upload(ctx)
    pflat, poff = _pair_sequences(db, flat, off)
    mirrors = _five_mirrors(swg, data, "edges", sub, q, (GO, GE), pflat, poff)
    n = len(mirrors[0])
    assert np.all(mirrors[4] <= mirrors[3]) and np.sum(mirrors[4] < mirrors[3]) > n // 4     # (the charge is felt: W = 2, e = 1)
    _geometry(ctx, off)
    _force_levels(ctx, swg)
    _, hits, _ = ctx.search(db, want_scores=False, k=10)
    scores = orc.score_db(q, flat, off, sub, GO, GE)
    assert hits == orc.topk(scores, 10)
    assert ctx.prune_last()["pruned"] and ctx.prune_last()["threshold"] > 0
    got, _ = _check(ctx, db, n, mirrors, False)
    assert len(got["stages"]) >= 4
    hits, total, _ = ctx.search_above(db, 40)
    want = sorted(((int(s), i) for i, s in enumerate(scores) if s >= 40), key=lambda h: (-h[0], h[1]))
    assert total == len(want) and sorted(hits, key=lambda h: (-h[0], h[1])) == want
    got, _ = _check(ctx, db, n, mirrors, True)
    assert all(T == 40 for _, _, T, _ in got["stages"])
    # behind no fourth level's walk: the table of (5, 256) is built all the same, and the hits are the oracle's
    _force_levels(ctx, swg, fourth=False)
    _, hits, _ = ctx.search(db, want_scores=False, k=10)
    assert hits == orc.topk(scores, 10) and ctx.debug_prune_tables4()["refine4"] == 0 and ctx.debug_prune_tables5()["refine5"] == 256
    db.close()


def test_one_launch_segment_under_a_callers_threshold(swg, orc, ctx, data):  # noqa: F811
    """lq = 61: W = 1 and 195 segments without columns; one launch segment, cut at a caller's threshold from the start."""
    flat, off = data["long_short"]
    q = data["q"][100:161].copy()
    sub = _sub(swg, "PAM250")
    gaps = (-11, -1)
    _set_query(ctx, swg, sub, q, gaps)
    db = swg.Database(flat, off).upload(ctx)
    pflat, poff = _pair_sequences(db, flat, off)
    mirrors = _five_mirrors(swg, data, "long_short61", sub, q, gaps, pflat, poff)
    n = len(mirrors[0])
    for key, v in {"cols_per_wave": 4, "group_lanes": 16}.items():
        ctx.set_option(key, v)
    _force_levels(ctx, swg)
    scores = orc.score_db(q, flat, off, sub, gaps[0], gaps[1])
    T = int(np.sort(scores)[-30])
    hits, total, _ = ctx.search_above(db, T)
    want = sorted(((int(s), i) for i, s in enumerate(scores) if s >= T), key=lambda h: (-h[0], h[1]))
    assert ctx.prune_last()["pruned"] and total == len(want) and sorted(hits, key=lambda h: (-h[0], h[1])) == want
    got, _ = _check(ctx, db, n, mirrors, True)
    assert len(got["stages"]) == 1 and got["stages"][0][2] == T
    _, top, _ = ctx.search(db, want_scores=False, k=10)
    assert top == orc.topk(scores, 10)
    db.close()


@contextlib.contextmanager
def _own_context(swg, data):  # noqa: F811
    """A context of its own -- a refused table is refused for the rest of a context's life, and the session's holds both
    already -- with the module's query and database and all five levels forced -> (context, database, the unpruned hits)"""
    c = swg.Context(0)
    db = None
    try:
        c.set_option("autotune", 0)
        _set_query(c, swg, _sub(swg, "BLOSUM62"), data["q"], (GO, GE))
        _geometry(c, data["off"])
        db = swg.Database(data["flat"], data["off"]).upload(c)
        c.set_option("prune", 0)
        _, plain, _ = c.search(db, want_scores=False, k=10)
        _force_levels(c, swg)
        yield c, db, plain
    finally:
        swg.lib.swg_debug_fail_alloc(0)
        if db is not None:
            db.close()
        c.close()


def test_a_refused_fifth_table_leaves_the_fourth_level(swg, data):  # noqa: F811
    """swg_debug_fail_alloc site 6: the reservation of the fifth level's table finds no room (simulated on the host)."""
    with _own_context(swg, data) as (c, db, plain):
        swg.lib.swg_debug_fail_alloc(6)
        _, hits, _ = c.search(db, want_scores=False, k=10)
        assert hits == plain and c.prune_last()["pruned"]
        four, five = c.debug_prune_tables4(), c.debug_prune_tables5()
        assert four["refine4"] == 256 and four["bits"] == 8 and not four["refused"]
        assert five["refine5"] == 0 and five["refused"] is True and five["refine5_builds"] == 0


def test_a_refused_fourth_table_takes_the_fifth_level_with_it(swg, data):  # noqa: F811
    """Site 5: the fourth level's table, which the fifth reads too; and the context stays without both."""
    with _own_context(swg, data) as (c, db, plain):
        swg.lib.swg_debug_fail_alloc(5)
        for _ in range(2):
            _, hits, _ = c.search(db, want_scores=False, k=10)
            assert hits == plain and c.prune_last()["pruned"]
            four, five = c.debug_prune_tables4(), c.debug_prune_tables5()
            assert four["refine4"] == 0 and four["refused"] is True and four["refine4_builds"] == 0
            assert five["refine5"] == 0 and five["refine5_builds"] == 0
            assert c.debug_prune_tables()["refine3"] == 256     # (the levels in front stand)


def test_a_refusal_is_the_contexts_own(swg, data):  # noqa: F811
    with _own_context(swg, data) as (c, db, plain):
        swg.lib.swg_debug_fail_alloc(5)
        c.search(db, want_scores=False, k=10)
        assert c.debug_prune_tables4()["refused"] is True
        with _own_context(swg, data) as (c2, db2, plain2):
            _, hits, _ = c2.search(db2, want_scores=False, k=10)
            four, five = c2.debug_prune_tables4(), c2.debug_prune_tables5()
            assert hits == plain2 == plain
            assert four["refine4"] == 256 and not four["refused"] and five["refine5"] == 256 and not five["refused"]


def test_views_shards_searches_in_flight_and_the_automatic_choice(swg, ctx, data):  # noqa: F811
    flat, off, q = data["flat"], data["off"], data["q"]
    sub = _sub(swg, "BLOSUM62")
    _set_query(ctx, swg, sub, q, (GO, GE))
    _geometry(ctx, off)
    db = swg.Database(flat, off).upload(ctx)
    ctx.set_option("prune", 0)
    _, plain, _ = ctx.search(db, want_scores=False, k=10)
    _force_levels(ctx, swg)
    _, hits, _ = ctx.search(db, want_scores=False, k=10)
    builds = ctx.debug_prune_tables5()["refine5_builds"]
    assert hits == plain and ctx.debug_prune_tables5()["refine5"] == 256
    members = np.arange(0, len(off) - 1, 2, dtype=np.uint32)
    view = db.view(ctx, members)
    ctx.set_option("prune", 0)
    _, vplain, _ = ctx.search(view, want_scores=False, k=10)
    ctx.set_option("prune", 2)
    _, vhits, _ = ctx.search(view, want_scores=False, k=10)
    assert vhits == vplain and ctx.prune_last()["pruned"]
    assert ctx.debug_prune_tables5() == {"refine5": 256, "refine5_builds": builds, "bits": 8, "refused": False}
    view.close()
    shard = swg.Database(flat, off, shard_rank=1, shard_count=2).upload(ctx)
    ctx.set_option("prune", 0)
    _, splain, _ = ctx.search(shard, want_scores=False, k=10)
    ctx.set_option("prune", 2)
    _, shits, _ = ctx.search(shard, want_scores=False, k=10)
    assert shits == splain and ctx.debug_prune_tables5()["refine5_builds"] == builds
    s1 = ctx.search_begin(db, want_scores=False, k=10)
    s2 = ctx.search_begin(shard, want_scores=False, k=10)
    assert ctx.search_end(s1)[1] == plain and ctx.search_end(s2)[1] == splain
    assert ctx.debug_prune_tables5()["refine5_builds"] == builds
    # a gap whose further residues are free: the level is off, forced or not, and nothing is built
    ctx.set_scoring(sub, -3, 0)
    ctx.set_option("prune", 0)
    _, zplain, _ = ctx.search(db, want_scores=False, k=10)
    ctx.set_option("prune", 2)
    _, zhits, _ = ctx.search(db, want_scores=False, k=10)
    assert zhits == zplain and ctx.debug_prune_tables5()["refine5"] == 0 and ctx.debug_prune_tables5()["refine5_builds"] == builds
    assert ctx.debug_prune_tables4()["refine4"] == 256
    # left automatic on a database of this size: not taken, and the launches are those of the level switched off
    ctx.set_scoring(sub, GO, GE)
    logs = []
    for v in (0, 1):
        for key in KEYS:
            ctx.set_option(key, 0)
        ctx.set_option("prune_refine5", v)
        swg.debug_launch_log(True)
        _, ahits, _ = ctx.search(db, want_scores=False, k=10)
        logs.append(swg.debug_launch_log_read())
        swg.debug_launch_log(False)
        assert ahits == plain and ctx.debug_prune_tables5()["refine5"] == 0 and ctx.debug_prune_tables5()["refine5_builds"] == builds
    assert logs[0] == logs[1] and len(logs[0]) > 0
    with pytest.raises(Exception, match="prune_refine5"):
        ctx.set_option("prune_refine5", 256)
    shard.close()
    db.close()
