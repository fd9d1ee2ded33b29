"""GPU (-m gpu): the k-mer form of the pruning bound (option prune_kmer = 4 / 5), on the small databases of
test_gpu_prune.py under prune = 2.

The device's table -- every class block's local score against the query -- and its pair bounds must be the host mirror's
(swg_debug_prune_kmer), entry for entry; the hits under every bound must be the unpruned search's and the oracle's; and
the tighter bound must cut at least what the colmax bound cuts."""
import numpy as np
import pytest

from test_gpu_parity import _reset_options
from test_gpu_prune import FORMS, GE, GEOMETRIES, GO, N, _case, _expected, _segment_blocks
from test_gpu_prune import data  # noqa: F401  (the module's databases and oracle scores, as a fixture of this module)

pytestmark = pytest.mark.gpu

KMERS = (1, 4, 5)


@pytest.fixture(autouse=True)
def _options(ctx):
    def reset():
        _reset_options(ctx)
        ctx.set_option("prune", 1)
        ctx.set_option("prune_head", 4)
        ctx.set_option("prune_kmer", 0)

    reset()
    ctx.set_option("autotune", 0)
    yield
    reset()
    ctx.set_option("autotune", 1)


def _pair_sequences(db, flat, off):
    """The pairs of the token order as sequences for the mirror: x, then y filled up to x's length with padding rows."""
    order = np.array([int(v) for v in db.order()], dtype=np.int64)
    assert len(order) % 2 == 0 and np.all(order != 0xFFFFFFFF)
    o = off.astype(np.int64)
    parts, lens = [], []
    for x, y in zip(order[0::2], order[1::2]):
        sx, sy = flat[o[x]:o[x + 1]], flat[o[y]:o[y + 1]]
        assert len(sx) >= len(sy)
        parts += [sx, sy, np.zeros(len(sx) - len(sy), dtype=np.int8)]
        lens += [len(sx), len(sx)]
    poff = np.zeros(len(lens) + 1, dtype=np.uint64)
    poff[1:] = np.cumsum(lens)
    return np.concatenate(parts).astype(np.int8), poff


@pytest.mark.parametrize("k", [4, 5])
def test_table_and_pair_bounds_equal_the_mirror(swg, ctx, data, k):
    """Index query, the same after set_scoring with other gaps, and the PSSM of the same query under a third pair of
    gaps: the device's table is the mirror's.  The pair bounds of the first: max(U_x, U_y) of every pair."""
    flat, off = data["A"]
    sub = data["sub"]
    q = data["qA"][:75].copy()
    ctx.set_option("prune", 2)
    ctx.set_option("prune_kmer", k)
    for key, v in GEOMETRIES["four_passes_segments"](off).items():
        ctx.set_option(key, v)
    db = swg.Database(flat, off).upload(ctx)
    pflat, poff = _pair_sequences(db, flat, off)
    builds = ctx.debug_prune_kmer_read(db)["builds"]
    for step, (kind, gaps) in enumerate((("index", (GO, GE)), ("index", (-11, -1)), ("pssm", (0, 0)))):
        ctx.set_scoring(sub, gaps[0], gaps[1])
        if kind == "pssm":
            pssm = sub[q.astype(np.int64)]
            ctx.set_query_pssm(pssm)
            want_t, u = swg.debug_prune_kmer(pssm, None, gaps[0], gaps[1], k, pflat, poff)
        else:
            ctx.set_query(q)
            want_t, u = swg.debug_prune_kmer(sub, q, gaps[0], gaps[1], k, pflat, poff)
        ctx.search(db, want_scores=False, k=10)
        assert ctx.prune_last()["pruned"]
        got = ctx.debug_prune_kmer_read(db, k=k, bounds=True)
        assert got["k"] == k and got["builds"] == builds + step + 1, (kind, gaps, got["k"], got["builds"])
        assert np.array_equal(got["table"], want_t), (kind, gaps, int(np.flatnonzero(got["table"] != want_t)[0]))
        want_b = np.maximum(u[0::2], u[1::2]).astype(np.int64)
        assert got["pairs"] >= len(want_b)
        assert np.array_equal(got["bounds"][:len(want_b)].astype(np.int64), want_b), (kind, gaps)
        assert not np.any(got["bounds"][len(want_b):])            # (pairs of empty slots)
    db.close()


def _hits_under_every_bound(ctx, db, truth, members, label, ks=(10, 100)):
    """Hits under prune = 0 and under prune = 2 with every bound: the oracle's.  -> pairs skipped per bound at ks[0]."""
    skipped = {}
    for k in ks:
        ctx.set_option("prune", 0)
        _, plain, st0 = ctx.search(db, want_scores=False, k=k)
        assert plain == _expected(truth, members, k), (label, k)
        ctx.set_option("prune", 2)
        for kmer in KMERS:
            ctx.set_option("prune_kmer", kmer)
            _, hits, st = ctx.search(db, want_scores=False, k=k)
            info = ctx.prune_last()
            assert info["pruned"] and ctx.debug_prune_kmer_read(db)["k"] == kmer, (label, k, kmer, info)
            assert hits == plain, (label, k, kmer, info, st)
            assert st["cell_form"] == st0["cell_form"] and st["passes"] == st0["passes"], (label, k, kmer)
            if k == ks[0]:
                skipped[kmer] = (info["pairs_skipped"], info["pair_rows_skipped"])
    assert skipped[4] >= skipped[1] and skipped[5] >= skipped[1], (label, skipped)
    return skipped, st


@pytest.mark.parametrize("geometry,form", [("four_passes_segments", "f16"), ("four_passes_segments", "int16"), ("four_passes_segments", "wide"),
                                           ("last_pass_28", "f16"), ("one_pass", "f16")])
def test_hits_equal_unpruned_and_oracle(swg, ctx, data, geometry, form):
    flat, off, q, sub, truth = _case(data, geometry, form)
    ctx.set_scoring(sub, GO, GE)
    ctx.set_query(q)
    opts = {**GEOMETRIES[geometry](off), **FORMS[form][0]}
    if geometry == "last_pass_28":
        opts["segment_blocks"] = _segment_blocks(off)
    for key, v in opts.items():
        ctx.set_option(key, v)
    db = swg.Database(flat, off).upload(ctx)
    skipped, st = _hits_under_every_bound(ctx, db, truth, np.arange(len(truth)), (geometry, form))
    assert st["cell_form"] in FORMS[form][1] and st["engine"] == 2 and st["work_queue"] == 1, st
    if geometry == "last_pass_28":
        assert st["passes"] == 2 and st["last_pass_cols"] == 28, st
    if geometry == "four_passes_segments" and form == "f16":
        # database A, unrelated sequences but for 1 %: the tighter bounds cut strictly more
        assert st["passes"] == 4
        assert skipped[4] > skipped[1] and skipped[5] > skipped[1], skipped
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
    skipped, _ = _hits_under_every_bound(ctx, db, data["truthA"], want, dbkind)
    assert skipped[1][0] > 0, skipped
    db.close()
    if parent is not None:
        parent.close()


def test_a_new_query_gets_a_new_table(swg, ctx, orc, data):
    """Query A, then query B against a database that holds relatives of B which score low against A: half of them among
    the longest sequences (the first stage: they set T), half of them short.  Under A's table the short ones' bounds are
    below T; the hits must be B's, and the table on the device B's."""
    sub = data["sub"]
    rng = np.random.default_rng(0x5EED0C01)
    letters = np.array(sorted(set(int(v) for v in data["A"][0]) - {0}))
    qa = swg.synth_query(0x5EED0C02, 300)
    qb = swg.synth_query(0x5EED0C03, 300)
    seqs = [rng.choice(letters, size=int(n)).astype(np.int8) for n in rng.integers(100, 601, size=1988)]

    def relative(changed):
        r = qb.copy()
        at = rng.choice(300, size=changed, replace=False)
        r[at] = rng.choice(letters, size=changed)
        return r.astype(np.int8)

    for _ in range(6):   # (the long ones are the more distant: the short ones are the hits)
        seqs.append(np.concatenate([rng.choice(letters, size=140), relative(30), rng.choice(letters, size=150)]).astype(np.int8))
    for _ in range(6):
        seqs.append(relative(8))
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    flat = np.concatenate(seqs).astype(np.int8)
    truth_a = orc.score_db(qa, flat, off, sub, GO, GE)
    truth_b = orc.score_db(qb, flat, off, sub, GO, GE)
    n = len(seqs)
    ctx.set_scoring(sub, GO, GE)
    ctx.set_option("cols_per_wave", 4)
    ctx.set_option("group_lanes", 16)
    ctx.set_option("segment_blocks", _segment_blocks(off))
    ctx.set_option("prune", 2)
    ctx.set_option("prune_kmer", 4)
    db = swg.Database(flat, off).upload(ctx)
    ctx.set_query(qa)
    _, hits, _ = ctx.search(db, want_scores=False, k=5)
    assert hits == _expected(truth_a, np.arange(n), 5)
    ctx.set_query(qb)
    _, hits, _ = ctx.search(db, want_scores=False, k=5)
    info = ctx.prune_last()
    assert hits == _expected(truth_b, np.arange(n), 5), info
    assert set(i for _, i in hits) <= set(range(n - 6, n)), hits
    assert info["pairs_skipped"] > 0, info
    # what a stale table would have done: the short relatives' bounds under A's table are below the threshold they met
    ta, ua = swg.debug_prune_kmer(sub, qa, GO, GE, 4, flat, off)
    tb, ub = swg.debug_prune_kmer(sub, qb, GO, GE, 4, flat, off)
    fifth_long = int(np.sort(truth_b[n - 12:n - 6])[-5])          # (T once the first stage is filled)
    assert fifth_long <= info["threshold"] and np.all(ua[n - 6:] < fifth_long) and np.all(ub[n - 6:] >= truth_b[n - 6:]), (ua[n - 6:], fifth_long, info)
    assert np.array_equal(ctx.debug_prune_kmer_read(db, k=4)["table"], tb)
    db.close()


def test_searches_in_flight_share_one_table(swg, ctx, data):
    flat, off = data["A"]
    ctx.set_scoring(data["sub"], GO, GE)
    ctx.set_query(data["qA"])
    for key, v in GEOMETRIES["four_passes_segments"](off).items():
        ctx.set_option(key, v)
    ctx.set_option("prune", 2)
    db = swg.Database(flat, off).upload(ctx)
    ctx.set_option("prune_kmer", 1)
    ctx.search(db, want_scores=False, k=1)                            # (plans and buffers exist: the ones below only queue)
    builds = ctx.debug_prune_kmer_read(db)["builds"]
    ctx.set_option("prune_kmer", 5)
    tickets = [(ctx.search_begin(db, k=k), k) for k in (3, 100, 10)]
    for t, k in tickets:
        _, hits, _ = ctx.search_end(t)
        assert hits == _expected(data["truthA"], np.arange(N), k), k
        assert ctx.prune_last()["pruned"], k
    assert ctx.debug_prune_kmer_read(db)["builds"] == builds + 1
    # ... and searches that alternate between the two tables build each once
    tickets = []
    for kmer, k in ((4, 10), (5, 3), (4, 100), (5, 10)):
        ctx.set_option("prune_kmer", kmer)
        tickets.append((ctx.search_begin(db, k=k), k))
    for t, k in tickets:
        _, hits, _ = ctx.search_end(t)
        assert hits == _expected(data["truthA"], np.arange(N), k), k
    assert ctx.debug_prune_kmer_read(db)["builds"] == builds + 2
    db.close()


def test_flags_behind_a_cut_at_k5(swg, ctx, data):
    """Database B on the f16 cells under the table of 5: the planted copies score above 4096, are flagged in the head and
    run again on the int16 cells; the threshold (4095, the histogram's last bin) cuts nearly all the rest.  With scores
    asked for (diagnostic), a skipped sequence reports 0 and its true score is below T, flagged or not."""
    flat, off = data["B"]
    truth = data["truthB"]
    ctx.set_scoring(data["sub"], GO, GE)
    ctx.set_query(data["qB"])
    ctx.set_option("f16", 2)
    ctx.set_option("prune_kmer", 5)
    db = swg.Database(flat, off).upload(ctx)
    ctx.set_option("prune", 0)
    _, plain, _ = ctx.search(db, want_scores=False, k=10)
    ctx.set_option("prune", 2)
    _, hits, st = ctx.search(db, want_scores=False, k=10)
    info = ctx.prune_last()
    assert hits == plain == _expected(truth, np.arange(N), 10), info
    assert st["cell_form"] == 2 and st["n_rescored"] >= 10, st
    assert info["threshold"] == 4095 and info["pairs_skipped"] > N // 4, info
    ctx.set_option("prune_kmer", 1)
    ctx.search(db, want_scores=False, k=10)
    assert info["pairs_skipped"] >= ctx.prune_last()["pairs_skipped"]
    ctx.set_option("prune_kmer", 5)
    scores, hits, _ = ctx.search(db, want_scores=True, k=10)
    info = ctx.prune_last()
    T = info["threshold"]
    assert hits == _expected(truth, np.arange(N), 10) and T == 4095
    skipped = (scores == 0) & (truth != 0)
    assert skipped.sum() > 0 and np.array_equal(scores[~skipped], truth[~skipped])
    assert np.all(truth[skipped] < T)
    db.close()
