"""GPU (-m gpu): the segmented, ordered form of the k-mer pruning bound (options prune_kmer = 4 / 5 with
prune_segments = S), on the small databases of test_gpu_prune.py under prune = 2.

The device's table -- every class block's best cell within each of the S segments of the query's columns -- and its pair
bounds must be the host mirror's (swg_debug_prune_kmer_seg), entry for entry; the hits must be the unpruned search's and
the oracle's; and the ordered bound must cut at least what the unordered one cuts."""
import numpy as np
import pytest

from test_gpu_parity import _reset_options
from test_gpu_prune import FORMS, GE, GEOMETRIES, GO, N, _case, _expected, _segment_blocks
from test_gpu_prune import data  # noqa: F401  (the module's databases and oracle scores, as a fixture of this module)
from test_gpu_prune_kmer import _pair_sequences

pytestmark = pytest.mark.gpu

CASES = [(4, 3), (4, 16), (4, 32), (5, 8)]   # (k, S): every lane-group width of the bound kernel, S below and at the width


@pytest.fixture(autouse=True)
def _options(ctx):
    def reset():
        _reset_options(ctx)
        ctx.set_option("prune", 1)
        ctx.set_option("prune_head", 4)
        ctx.set_option("prune_kmer", 0)
        ctx.set_option("prune_segments", 0)

    reset()
    ctx.set_option("autotune", 0)
    yield
    reset()
    ctx.set_option("autotune", 1)


@pytest.mark.parametrize("k,S,lq", [(k, S, 200) for k, S in CASES] + [(4, 32, 100)])
def test_table_and_pair_bounds_equal_the_mirror(swg, ctx, data, k, S, lq):
    """Index query, then the PSSM of the same query under other gaps.  200 columns: four passes; 100 columns in 32
    segments of 4: the last seven hold nothing."""
    flat, off = data["A"]
    sub = data["sub"]
    q = data["qA"][:lq].copy()
    ctx.set_option("prune", 2)
    ctx.set_option("prune_kmer", k)
    ctx.set_option("prune_segments", S)
    for key, v in GEOMETRIES["four_passes_segments"](off).items():
        ctx.set_option(key, v)
    db = swg.Database(flat, off).upload(ctx)
    pflat, poff = _pair_sequences(db, flat, off)
    builds = ctx.debug_prune_kmer_seg_read(db)["builds"]
    for step, (kind, gaps) in enumerate((("index", (GO, GE)), ("pssm", (-11, -1)))):
        ctx.set_scoring(sub, gaps[0], gaps[1])
        if kind == "pssm":
            pssm = sub[q.astype(np.int64)]
            ctx.set_query_pssm(pssm)
            want_t, u = swg.debug_prune_kmer_seg(pssm, None, gaps[0], gaps[1], k, S, pflat, poff)
        else:
            ctx.set_query(q)
            want_t, u = swg.debug_prune_kmer_seg(sub, q, gaps[0], gaps[1], k, S, pflat, poff)
        ctx.search(db, want_scores=False, k=10)
        assert ctx.prune_last()["pruned"]
        got = ctx.debug_prune_kmer_seg_read(db, k=k, segments=S, bounds=True)
        assert (got["k"], got["segments"]) == (k, S) and got["builds"] == builds + step + 1, (kind, gaps, got["k"], got["segments"], got["builds"])
        assert np.array_equal(got["table"], want_t), (kind, gaps, np.argwhere(got["table"] != want_t)[0])
        want_b = np.maximum(u[0::2], u[1::2]).astype(np.int64)
        assert got["pairs"] >= len(want_b)
        assert np.array_equal(got["bounds"][:len(want_b)].astype(np.int64), want_b), (kind, gaps)
        assert not np.any(got["bounds"][len(want_b):])            # (pairs of empty slots)
        if lq == 100:
            assert not np.any(got["table"][:, 25:]) and np.any(got["table"][:, 24])
    db.close()


def _hits_under_every_bound(ctx, db, truth, members, label, ks=(10, 100)):
    """Hits under prune = 0 and under prune = 2 with every (k, S): the oracle's.  -> pairs and rows skipped per bound at ks[0]."""
    skipped = {}
    for k in ks:
        ctx.set_option("prune", 0)
        _, plain, st0 = ctx.search(db, want_scores=False, k=k)
        assert plain == _expected(truth, members, k), (label, k)
        ctx.set_option("prune", 2)
        for kmer, S in [(4, 1), (5, 1)] + CASES:
            ctx.set_option("prune_kmer", kmer)
            ctx.set_option("prune_segments", S)
            _, hits, st = ctx.search(db, want_scores=False, k=k)
            info = ctx.prune_last()
            got = ctx.debug_prune_kmer_seg_read(db)
            assert info["pruned"] and (got["k"], got["segments"]) == (kmer, S), (label, k, kmer, S, info)
            assert hits == plain, (label, k, kmer, S, info, st)
            assert st["cell_form"] == st0["cell_form"] and st["passes"] == st0["passes"], (label, k, kmer, S)
            if k == ks[0]:
                skipped[(kmer, S)] = (info["pairs_skipped"], info["pair_rows_skipped"])
    # the ordered bound is never above the unordered one of the same k: it cuts at least as much
    for kmer, S in CASES:
        assert skipped[(kmer, S)] >= skipped[(kmer, 1)], (label, skipped)
    return skipped, st


@pytest.mark.parametrize("form", ["f16", "int16", "wide"])
def test_hits_equal_unpruned_and_oracle(swg, ctx, data, form):
    flat, off, q, sub, truth = _case(data, "four_passes_segments", form)
    ctx.set_scoring(sub, GO, GE)
    ctx.set_query(q)
    for key, v in {**GEOMETRIES["four_passes_segments"](off), **FORMS[form][0]}.items():
        ctx.set_option(key, v)
    db = swg.Database(flat, off).upload(ctx)
    skipped, st = _hits_under_every_bound(ctx, db, truth, np.arange(len(truth)), form)
    assert st["cell_form"] in FORMS[form][1] and st["engine"] == 2 and st["work_queue"] == 1, st
    if form == "f16":
        assert st["passes"] == 4
        # swg_prune_last: at least as many pair rows skipped at (5, 8) as at (5, 1)
        assert skipped[(5, 8)][1] >= skipped[(5, 1)][1], skipped
    db.close()


@pytest.mark.parametrize("dbkind", ["view", "shard"])
def test_views_and_shards(swg, ctx, data, dbkind):
    flat, off = data["A"]
    ctx.set_scoring(data["sub"], GO, GE)
    ctx.set_query(data["qA"])
    for key, v in GEOMETRIES["four_passes_segments"](off).items():
        ctx.set_option(key, v)
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
    ctx.set_option("segment_blocks", _segment_blocks(off, members=want))
    skipped, _ = _hits_under_every_bound(ctx, db, data["truthA"], want, dbkind, ks=(10,))
    assert skipped[(4, 1)][0] > 0, skipped
    db.close()
    if parent is not None:
        parent.close()


def test_a_new_query_gets_a_new_table_and_searches_in_flight_share_one(swg, ctx, data):
    flat, off = data["A"]
    sub = data["sub"]
    ctx.set_scoring(sub, GO, GE)
    for key, v in GEOMETRIES["four_passes_segments"](off).items():
        ctx.set_option(key, v)
    ctx.set_option("prune", 2)
    ctx.set_option("prune_kmer", 4)
    ctx.set_option("prune_segments", 16)
    db = swg.Database(flat, off).upload(ctx)
    qa = data["qA"]
    qb = np.ascontiguousarray(qa[::-1])
    ctx.set_query(qa)
    ctx.search(db, want_scores=False, k=10)
    builds = ctx.debug_prune_kmer_seg_read(db)["builds"]
    # searches in flight share the table of the epoch
    tickets = [(ctx.search_begin(db, k=k), k) for k in (3, 100, 10)]
    for t, k in tickets:
        _, hits, _ = ctx.search_end(t)
        assert hits == _expected(data["truthA"], np.arange(N), k), k
        assert ctx.prune_last()["pruned"], k
    assert ctx.debug_prune_kmer_seg_read(db)["builds"] == builds
    # a new query: a new table, B's
    ctx.set_query(qb)
    _, hits_b, _ = ctx.search(db, want_scores=False, k=10)
    got = ctx.debug_prune_kmer_seg_read(db, k=4, segments=16)
    assert got["builds"] == builds + 1
    tb, _ = swg.debug_prune_kmer_seg(sub, qb, GO, GE, 4, 16, flat[:1], np.array([0, 1], dtype=np.uint64))
    ta, _ = swg.debug_prune_kmer_seg(sub, qa, GO, GE, 4, 16, flat[:1], np.array([0, 1], dtype=np.uint64))
    assert np.array_equal(got["table"], tb) and not np.array_equal(ta, tb)
    ctx.set_option("prune", 0)
    _, plain_b, _ = ctx.search(db, want_scores=False, k=10)
    assert hits_b == plain_b
    ctx.set_option("prune", 2)
    # the same k with other segments is another table: built again, and the unsegmented hook does not read it
    ctx.set_option("prune_segments", 32)
    _, hits_b32, _ = ctx.search(db, want_scores=False, k=10)
    assert hits_b32 == plain_b and ctx.debug_prune_kmer_seg_read(db)["builds"] == builds + 2
    with pytest.raises(Exception):
        ctx.debug_prune_kmer_read(db, k=4)
    # a table beyond the budget is refused
    ctx.set_option("prune_kmer", 5)
    with pytest.raises(Exception, match="budget"):
        ctx.search(db, want_scores=False, k=10)
    ctx.set_option("prune_segments", 8)
    _, hits_b58, _ = ctx.search(db, want_scores=False, k=10)
    assert hits_b58 == plain_b
    db.close()
