"""GPU (-m gpu): the pair-by-pair cut of a pruned search's stages and the second-level bound behind it (DESIGN 4.2.1;
options prune_cut and prune_refine), on database A of test_gpu_prune.py under prune = 2 in the four_passes_segments
geometry, the first level forced to k = 4 in 32 segments and the second to 64 and to 128.

The second table must be the host mirror's entry for entry; after a search every pair's bound must be the first level's,
or -- in a cut stage, where that reached the stage's T -- the lesser of it and the refined one; every stage's list must
be exactly the ids of its pairs whose bound reaches its T, ascending, and swg_prune_last must count the others; and the
hits must be the unpruned search's and the oracle's."""
import numpy as np
import pytest

from test_gpu_parity import _reset_options
from test_gpu_prune import FORMS, GE, GEOMETRIES, GO, N, _case, _expected, _segment_blocks
from test_gpu_prune import data  # noqa: F401  (the module's databases and oracle scores, as a fixture of this module)
from test_gpu_prune_kmer import _pair_sequences

pytestmark = pytest.mark.gpu

REFINES = (64, 128)


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


def _force(ctx, off, refine, extra=None):
    ctx.set_option("prune", 2)
    ctx.set_option("prune_kmer", 4)
    ctx.set_option("prune_segments", 32)
    ctx.set_option("prune_refine", refine)
    for key, v in {**GEOMETRIES["four_passes_segments"](off), **(extra or {})}.items():
        ctx.set_option(key, v)


def _mirror(swg, rows, q, gaps, S2, pflat, poff):
    """-> (first-level pair bounds, refined pair bounds, the second table) from the host mirrors"""
    _, u = swg.debug_prune_kmer_seg(rows, q, gaps[0], gaps[1], 4, 32, pflat, poff, table=False)
    t2, r = swg.debug_prune_kmer_refine(rows, q, gaps[0], gaps[1], S2, pflat, poff)
    return np.maximum(u[0::2], u[1::2]).astype(np.int64), np.maximum(r[0::2], r[1::2]).astype(np.int64), t2


def _pair_blocks(poff):
    rows = np.diff(poff.astype(np.int64))[0::2]
    return (2 + rows + 3) // 4


def _check_bounds_and_lists(ctx, db, first, refined, blocks, label):
    """The read-back of the search last ended against the mirrors.  -> (stages, pairs with a skipped one in front of a kept one)"""
    got = ctx.debug_prune_refine_read(db)
    info = ctx.prune_last()
    n = len(first)
    b = got["bounds"].astype(np.int64)
    assert got["pairs"] >= n and not np.any(b[n:]), label            # (pairs of empty slots: bound 0)
    both = np.minimum(first, refined)
    in_cut = np.zeros(got["pairs"], dtype=bool)
    skipped_pairs = skipped_blocks = 0
    holes = 0
    assert got["stages"], label
    last_T = 0
    for begin, end, T, lst in got["stages"]:
        assert 0 <= begin <= end <= got["pairs"] and not np.any(in_cut[begin:end]), (label, begin, end)
        in_cut[begin:end] = True
        assert T >= last_T and T <= info["threshold"], (label, T, last_T, info)
        last_T = T
        e = min(end, n)
        p = np.arange(begin, e)
        reach = first[p] >= T
        # below T at the first level: left alone
        assert np.array_equal(b[p][~reach], first[p][~reach]), (label, begin)
        # at or above: the lesser of the two
        done = b[p] == np.where(reach, both[p], first[p])
        assert np.all(done), (label, begin, p[~done][:5], b[p][~done][:5], both[p][~done][:5])
        want = begin + np.flatnonzero(b[begin:end] >= T)
        assert np.array_equal(lst.astype(np.int64), want), (label, begin, end, T, len(lst), len(want))
        skip = np.setdiff1d(np.arange(begin, end), want)
        skipped_pairs += len(skip)
        skipped_blocks += int(blocks[skip[skip < n]].sum())           # (an empty slot's pair has no blocks)
        if len(want):
            holes += int(np.sum(skip < want[-1]))
    # everywhere else: the first level's
    rest = np.flatnonzero(~in_cut[:n])
    assert np.array_equal(b[rest], first[rest]), label
    assert info["pairs_skipped"] == skipped_pairs and info["pair_rows_skipped"] == 4 * skipped_blocks, (label, info, skipped_pairs, skipped_blocks)
    return got["stages"], holes


@pytest.mark.parametrize("lq", [200, 100])
@pytest.mark.parametrize("S2", REFINES)
def test_table_bounds_and_lists_equal_the_mirror(swg, ctx, data, S2, lq):
    """Index query, then the PSSM of the same query under other gaps; k = 100, below which database A (40 relatives)
    keeps unrelated pairs and skips others among them: a prefix of the length order would not do."""
    flat, off = data["A"]
    sub = data["sub"]
    q = data["qA"][:lq].copy()
    _force(ctx, off, S2)
    db = swg.Database(flat, off).upload(ctx)
    pflat, poff = _pair_sequences(db, flat, off)
    blocks = _pair_blocks(poff)
    builds = ctx.debug_prune_refine_read(db, arrays=False)
    holes = 0
    for step, (kind, gaps) in enumerate((("index", (GO, GE)), ("pssm", (-11, -1)))):
        ctx.set_scoring(sub, gaps[0], gaps[1])
        rows, qq = (sub[q.astype(np.int64)].copy(), None) if kind == "pssm" else (sub, q)
        if kind == "pssm":
            ctx.set_query_pssm(rows)
        else:
            ctx.set_query(q)
        first, refined, t2 = _mirror(swg, rows, qq, gaps, S2, pflat, poff)
        ctx.search(db, want_scores=False, k=100)
        assert ctx.prune_last()["pruned"]
        got = ctx.debug_prune_refine_read(db, segments=S2)
        assert (got["k"], got["segments"], got["refine"]) == (4, 32, S2)
        assert got["builds"] == builds["builds"] + step + 1 and got["refine_builds"] == builds["refine_builds"] + step + 1
        assert np.array_equal(got["table"], t2), (kind, np.argwhere(got["table"] != t2)[0])
        stages, h = _check_bounds_and_lists(ctx, db, first, refined, blocks, (kind, S2, lq))
        assert len(stages) >= 4
        holes += h
    assert holes > 0
    db.close()


@pytest.mark.parametrize("form", ["f16", "int16", "wide"])
def test_hits_equal_unpruned_and_oracle(swg, ctx, data, form):
    flat, off, q, sub, truth = _case(data, "four_passes_segments", form)
    ctx.set_scoring(sub, GO, GE)
    ctx.set_query(q)
    db = swg.Database(flat, off).upload(ctx)
    pflat, poff = _pair_sequences(db, flat, off)
    blocks = _pair_blocks(poff)
    for S2 in REFINES:
        first, refined, _ = _mirror(swg, sub, q, (GO, GE), S2, pflat, poff)
        for k in (10, 100):
            _reset_options(ctx)
            ctx.set_option("autotune", 0)
            for key, v in {**GEOMETRIES["four_passes_segments"](off), **FORMS[form][0]}.items():
                ctx.set_option(key, v)
            ctx.set_option("prune", 0)
            _, plain, st0 = ctx.search(db, want_scores=False, k=k)
            assert plain == _expected(truth, np.arange(len(truth)), k), (form, k)
            _force(ctx, off, S2, FORMS[form][0])
            _, hits, st = ctx.search(db, want_scores=False, k=k)
            assert ctx.prune_last()["pruned"] and hits == plain, (form, S2, k, ctx.prune_last())
            assert st["cell_form"] == st0["cell_form"] and st["passes"] == st0["passes"] and st["cell_form"] in FORMS[form][1], (form, st)
            _check_bounds_and_lists(ctx, db, first, refined, blocks, (form, S2, k))
        # scores requested (diagnostic): the oracle's, or 0 where the pair's final bound is below the last T
        scores, hits, _ = ctx.search(db, want_scores=True, k=100)
        info = ctx.prune_last()
        assert info["pruned"] and hits == plain
        b = ctx.debug_prune_refine_read(db)["bounds"].astype(np.int64)
        order = np.array([int(v) for v in db.order()], dtype=np.int64)
        pair_of = np.empty(len(truth), dtype=np.int64)
        pair_of[order] = np.arange(len(order)) // 2
        zero = scores != truth
        assert not np.any(scores[zero]) and np.all(b[pair_of[zero]] < info["threshold"]), (form, S2, int(zero.sum()))
        assert info["pairs_skipped"] > 0 and zero.sum() > 0
    db.close()


def test_pairs_at_the_chunk_edges(swg, ctx, data):
    """A chunk of the refine kernel is 32 token blocks: pairs of 1, 31, 32, 33, 64 and 65 blocks, seeded among 400
    unrelated sequences.  No relatives and k = 3: T stays low, so the seeded pairs are all walked to their end."""
    sub = data["sub"]
    q = data["qA"]
    rng = np.random.default_rng(0x5EED0C01)
    flat, off = swg.synth_db(0x5EED0C02, 400, median=60, max_len=300)
    o = off.astype(np.int64)
    seqs = [flat[o[i]:o[i + 1]] for i in range(400)]
    for nb in (1, 1, 31, 31, 32, 32, 33, 33, 64, 64, 65, 65):            # 4 * nb - 2 rows: the longest sequence of nb blocks
        seqs.append(rng.integers(1, 21, size=4 * nb - 2).astype(np.int8))
    loff = np.zeros(len(seqs) + 1, dtype=np.uint64)
    loff[1:] = np.cumsum([len(s) for s in seqs])
    lflat = np.concatenate(seqs).astype(np.int8)
    ctx.set_scoring(sub, GO, GE)
    ctx.set_query(q)
    db = swg.Database(lflat, loff).upload(ctx)
    pflat, poff = _pair_sequences(db, lflat, loff)
    blocks = _pair_blocks(poff)
    assert {31, 32, 33, 64, 65} <= set(int(v) for v in blocks)
    for S2 in REFINES:
        first, refined, _ = _mirror(swg, sub, q, (GO, GE), S2, pflat, poff)
        _force(ctx, loff, S2, {"segment_blocks": _segment_blocks(loff, parts=12)})
        ctx.set_option("prune", 0)
        _, plain, _ = ctx.search(db, want_scores=False, k=3)
        ctx.set_option("prune", 2)
        _, hits, _ = ctx.search(db, want_scores=False, k=3)
        assert hits == plain and ctx.prune_last()["pruned"]
        stages, _ = _check_bounds_and_lists(ctx, db, first, refined, blocks, ("edges", S2))
        # every seeded length has a pair in a cut stage whose first-level bound reached that stage's T: walked
        walked = np.zeros(len(blocks), dtype=bool)
        for begin, end, T, _ in stages:
            e = min(end, len(blocks))
            walked[begin:e] = first[begin:e] >= T
        assert all(np.any(walked & (blocks == nb)) for nb in (31, 32, 33, 64, 65)), [(nb, walked[blocks == nb]) for nb in (31, 32, 33, 64, 65)]
        assert np.any(refined[walked] < first[walked])
    db.close()


@pytest.mark.parametrize("dbkind", ["view", "shard"])
def test_views_and_shards(swg, ctx, data, dbkind):
    flat, off = data["A"]
    ctx.set_scoring(data["sub"], GO, GE)
    ctx.set_query(data["qA"])
    parent = None
    if dbkind == "view":
        want = np.delete(np.arange(N), np.arange(0, N, 3))
        parent = swg.Database(flat, off).upload(ctx)
        db = parent.view(ctx, want)
    else:
        want = np.arange(1, N, 2)
        o64 = off.astype(np.int64)
        loc = np.concatenate([flat[o64[i]:o64[i + 1]] for i in want]).astype(np.int8)
        loff = np.zeros(len(want) + 1, dtype=np.uint64)
        loff[1:] = np.cumsum(np.diff(o64)[want])
        db = swg.Database(loc, loff, index=want.astype(np.uint32), n_total=N).upload(ctx)
    for S2 in REFINES:
        _force(ctx, off, S2, {"segment_blocks": _segment_blocks(off, members=want)})
        ctx.set_option("prune", 0)
        _, plain, _ = ctx.search(db, want_scores=False, k=100)
        assert plain == _expected(data["truthA"], want, 100)
        ctx.set_option("prune", 2)
        _, hits, _ = ctx.search(db, want_scores=False, k=100)
        info = ctx.prune_last()
        assert info["pruned"] and hits == plain and info["pairs_skipped"] > 0, (dbkind, S2, info)
        got = ctx.debug_prune_refine_read(db)
        assert got["refine"] == S2
        for begin, end, T, lst in got["stages"]:
            assert np.array_equal(lst.astype(np.int64), begin + np.flatnonzero(got["bounds"][begin:end] >= T)), (dbkind, S2, begin)
    db.close()
    if parent is not None:
        parent.close()


def test_searches_in_flight_share_both_tables_and_a_new_query_rebuilds_them(swg, ctx, data):
    flat, off = data["A"]
    sub = data["sub"]
    ctx.set_scoring(sub, GO, GE)
    _force(ctx, off, 128)
    db = swg.Database(flat, off).upload(ctx)
    qa = data["qA"]
    qb = np.ascontiguousarray(qa[::-1])
    ctx.set_query(qa)
    ctx.search(db, want_scores=False, k=10)
    before = ctx.debug_prune_refine_read(db)
    tickets = [(ctx.search_begin(db, k=k), k) for k in (3, 100, 10)]
    for t, k in tickets:
        _, hits, _ = ctx.search_end(t)
        assert hits == _expected(data["truthA"], np.arange(N), k), k
        assert ctx.prune_last()["pruned"], k
    got = ctx.debug_prune_refine_read(db)
    assert (got["builds"], got["refine_builds"]) == (before["builds"], before["refine_builds"])
    # a new query: both tables anew, B's
    ctx.set_query(qb)
    _, hits_b, _ = ctx.search(db, want_scores=False, k=10)
    got = ctx.debug_prune_refine_read(db, segments=128)
    assert (got["builds"], got["refine_builds"]) == (before["builds"] + 1, before["refine_builds"] + 1)
    one = np.array([0, 1], dtype=np.uint64)
    tb, _ = swg.debug_prune_kmer_refine(sub, qb, GO, GE, 128, flat[:1], one)
    ta, _ = swg.debug_prune_kmer_refine(sub, qa, GO, GE, 128, flat[:1], one)
    assert np.array_equal(got["table"], tb) and not np.array_equal(ta, tb)
    ctx.set_option("prune", 0)
    _, plain_b, _ = ctx.search(db, want_scores=False, k=10)
    assert hits_b == plain_b
    # the same query with the other S2 is another second table; the first stays
    ctx.set_option("prune", 2)
    ctx.set_option("prune_refine", 64)
    _, hits_b64, _ = ctx.search(db, want_scores=False, k=10)
    got = ctx.debug_prune_refine_read(db)
    assert hits_b64 == plain_b and (got["builds"], got["refine_builds"], got["refine"]) == (before["builds"] + 1, before["refine_builds"] + 2, 64)
    # off: nothing more is built, and the hook says so
    ctx.set_option("prune_refine", 1)
    _, hits_off, _ = ctx.search(db, want_scores=False, k=10)
    got = ctx.debug_prune_refine_read(db)
    assert hits_off == plain_b and (got["refine_builds"], got["refine"]) == (before["refine_builds"] + 2, 0)
    with pytest.raises(Exception, match="prune_refine"):
        ctx.set_option("prune_refine", 32)
    with pytest.raises(Exception, match="prune_cut"):
        ctx.set_option("prune_cut", 2)
    db.close()


def test_the_prefix_cut_is_still_there(swg, ctx, data):
    """prune_cut = 1: the stage takes the prefix up to its last pair that reaches T -- from the first-level bounds and
    each stage's T, which the pair-by-pair search of the same bound reads back, pairs_skipped is what lies behind them."""
    flat, off = data["A"]
    ctx.set_scoring(data["sub"], GO, GE)
    ctx.set_query(data["qA"])
    _force(ctx, off, 1)
    db = swg.Database(flat, off).upload(ctx)
    _, hits, _ = ctx.search(db, want_scores=False, k=100)
    by_pair = ctx.prune_last()
    got = ctx.debug_prune_refine_read(db)
    assert got["refine"] == 0 and got["stages"]
    behind = 0
    for begin, end, T, lst in got["stages"]:
        reach = np.flatnonzero(got["bounds"][begin:end] >= T)
        behind += (end - begin) - (int(reach[-1]) + 1 if len(reach) else 0)
    ctx.set_option("prune_cut", 1)
    _, hits1, _ = ctx.search(db, want_scores=False, k=100)
    prefix = ctx.prune_last()
    assert hits1 == hits == _expected(data["truthA"], np.arange(N), 100)
    # (T of a stage is the K-th best of the sequences filled so far: the prefix fills a superset, whose extra members
    # are below T -- the same T stage by stage)
    assert prefix["pruned"] and prefix["pairs_skipped"] == behind, (prefix, behind)
    assert by_pair["pairs_skipped"] > prefix["pairs_skipped"] and by_pair["threshold"] == prefix["threshold"]
    assert ctx.debug_prune_refine_read(db)["stages"] == []
    db.close()
