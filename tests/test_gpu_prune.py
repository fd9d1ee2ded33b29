"""GPU (-m gpu): hits-only pruning, run with option prune = 2 so that databases of a few thousand
sequences are staged and cut at all.

A pruned search skips the pairs whose score bound U = sum over residues of the residue's best score against any query
column is below the K-th best score found so far.  What it returns must be what the unpruned search returns -- the same
(score, index) pairs in the same order, which are the oracle's top-K -- through every geometry (one pass, several, several
segments, a last pass of its own), every 16-bit cell form, index and PSSM queries, plain databases, views and shards.
With scores requested (diagnostic) every sequence reports its oracle score or, skipped, 0 with U and the oracle score
both below the last threshold."""
import numpy as np
import pytest

from test_gpu_parity import _reset_options

pytestmark = pytest.mark.gpu

KS = (1, 10, 100)
GO, GE = -2, -1
N = 4000


@pytest.fixture(autouse=True)
def _options(ctx):
    _reset_options(ctx)
    ctx.set_option("autotune", 0)
    ctx.set_option("prune", 1)
    ctx.set_option("prune_head", 4)
    yield
    _reset_options(ctx)
    ctx.set_option("autotune", 1)
    ctx.set_option("prune", 1)
    ctx.set_option("prune_head", 4)


@pytest.fixture(scope="module")
def data(swg, orc):
    """The databases and every oracle score the module needs, computed once.
    A: 4000 short sequences, 1 % near-copies of a 200-column query (T ends high, most pairs fall below it).
    B: the same with a 1000-column query whose copies score above the f16 cells' ceiling of 4096; q952 = its first 952
    columns (two passes of 16 lanes x 32 columns, the last one 28 columns per lane); sub8 = the table times 8, under which
    the query can pass 32767 and the fill takes the wide form."""
    sub = np.asarray(swg.load_scoring("BLOSUM62").table(), dtype=np.int8).reshape(32, 32)
    d = {"sub": sub, "sub8": (sub.astype(np.int32) * 8).astype(np.int8)}
    d["qA"] = swg.synth_query(0x5EED0A01, 200)
    d["A"] = swg.synth_db(0x5EED0A02, N, median=60, max_len=600, query=d["qA"], fraction=0.01, subst=0.05)[:2]
    d["qB"] = swg.synth_query(0x5EED0B01, 1000)
    d["B"] = swg.synth_db(0x5EED0B02, N, median=60, max_len=1200, query=d["qB"], fraction=0.01, subst=0.05)[:2]
    d["q952"] = d["qB"][:952].copy()
    d["truthA"] = orc.score_db(d["qA"], d["A"][0], d["A"][1], sub, GO, GE)
    d["truthB"] = orc.score_db(d["qB"], d["B"][0], d["B"][1], sub, GO, GE)
    d["truthB952"] = orc.score_db(d["q952"], d["B"][0], d["B"][1], sub, GO, GE)
    d["truthB8"] = orc.score_db(d["qB"], d["B"][0], d["B"][1], d["sub8"], GO, GE)
    d["truthB8_952"] = orc.score_db(d["q952"], d["B"][0], d["B"][1], d["sub8"], GO, GE)
    assert np.sort(d["truthB"])[-10] > 4096 and np.sort(d["truthB952"])[-10] > 4096      # flags behind a cut
    assert np.sort(d["truthB8"])[-10] > 32767                                            # beyond the plain int16 cells
    return d


def _segment_blocks(off, parts=5, members=None):
    """segment_blocks that cuts the token order (pairs of consecutive sequences by length, two reset rows + the longer one,
    in 4-row blocks) of the sequences `members` (default: all) into at least `parts` segments."""
    lens = np.diff(off.astype(np.int64))
    lens = np.sort(lens if members is None else lens[members])[::-1]
    blocks = (lens[0::2] + 2 + 3) // 4
    return int(max(blocks.max() + 1, blocks.sum() // parts))


GEOMETRIES = {
    "one_pass": lambda off: {},
    "four_passes": lambda off: {"cols_per_wave": 4, "group_lanes": 16},
    "four_passes_segments": lambda off: {"cols_per_wave": 4, "group_lanes": 16, "segment_blocks": _segment_blocks(off)},
    "last_pass_28": lambda off: {"cols_per_wave": 32, "group_lanes": 16},
}
# (f16 = 2: the f16 cells even after a search of this database flagged more than 1/16 of its pair rows -- B's copies do)
FORMS = {"f16": ({"f16": 2}, (2,)), "int16": ({"f16": 0}, (0,)), "wide": ({"f16": 0}, (1,))}


def _case(data, geometry, form):
    """-> (flat, off, query, table, truth) of a (geometry, form) case: database A, except where the case needs a longer
    query (the 28-column last pass: B with 952 columns; the wide form: B under the table times 8)."""
    if form == "wide":
        q, truth = (data["q952"], data["truthB8_952"]) if geometry == "last_pass_28" else (data["qB"], data["truthB8"])
        return data["B"] + (q, data["sub8"], truth)
    if geometry == "last_pass_28":
        return data["B"] + (data["q952"], data["sub"], data["truthB952"])
    return data["A"] + (data["qA"], data["sub"], data["truthA"])


def _expected(truth, members, k):
    members = np.asarray(members, dtype=np.int64)
    return [(-s, i) for s, i in sorted((-int(truth[i]), int(i)) for i in members)[:k]]


def _hits_both_ways(ctx, db, truth, members, label, want_skips=None):
    """Hits for every k under prune = 0 and prune = 2: equal to each other and to the oracle's."""
    skipped = 0
    for k in KS:
        ctx.set_option("prune", 0)
        _, plain, st0 = ctx.search(db, want_scores=False, k=k)
        assert not ctx.prune_last()["pruned"], label
        ctx.set_option("prune", 2)
        _, pruned, st2 = ctx.search(db, want_scores=False, k=k)
        info = ctx.prune_last()
        assert info["pruned"], (label, k, st2)
        assert pruned == plain, (label, k, info, st2)
        assert pruned == _expected(truth, members, k), (label, k, info, st2)
        assert st2["cells"] == st0["cells"] and st2["cell_form"] == st0["cell_form"] and st2["passes"] == st0["passes"], (label, k)
        assert info["pair_rows_skipped"] <= info["pair_rows"] and (info["pairs_skipped"] > 0) == (info["pair_rows_skipped"] > 0), (label, info)
        skipped = max(skipped, info["pairs_skipped"])
    if want_skips:
        assert skipped > 0, label
    return st2


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_hits_equal_unpruned_and_oracle(swg, ctx, data, geometry, form):
    flat, off, q, sub, truth = _case(data, geometry, form)
    ctx.set_scoring(sub, GO, GE)
    ctx.set_query(q)
    for key, v in {**GEOMETRIES[geometry](off), **FORMS[form][0]}.items():
        ctx.set_option(key, v)
    db = swg.Database(flat, off).upload(ctx)
    st = _hits_both_ways(ctx, db, truth, np.arange(len(truth)), (geometry, form), want_skips=True)
    assert st["cell_form"] in FORMS[form][1], (geometry, form, st)
    assert st["engine"] == 2 and st["work_queue"] == 1, st
    if geometry == "one_pass":
        assert st["passes"] == 1 or len(q) > 200, st
    if geometry.startswith("four_passes") and len(q) == 200:
        assert st["passes"] == 4, st
    if geometry == "four_passes_segments":
        ctx.set_option("prune", 0)
        _, _, st0 = ctx.search(db, want_scores=False, k=10)
        assert st0["fill_launches"] >= 4 * st0["passes"], st0
    if geometry == "last_pass_28":
        assert st["passes"] == 2 and st["last_pass_cols"] == 28, st
    db.close()


def test_flags_behind_a_cut_are_rerun(swg, ctx, data):
    """Database B on the f16 cells: the planted copies score above 4096, are flagged in the head and run again on the int16
    cells by the list launch (never cut), while the threshold -- 4095, the histogram's last bin -- cuts nearly all the rest."""
    flat, off = data["B"]
    ctx.set_scoring(data["sub"], GO, GE)
    ctx.set_query(data["qB"])
    ctx.set_option("f16", 2)
    db = swg.Database(flat, off).upload(ctx)
    st = _hits_both_ways(ctx, db, data["truthB"], np.arange(N), "flags", want_skips=True)
    assert st["cell_form"] == 2 and st["n_rescored"] >= 10, st
    ctx.set_option("prune", 2)
    ctx.search(db, want_scores=False, k=10)
    info = ctx.prune_last()
    assert info["threshold"] == 4095 and info["pairs_skipped"] > N // 4, info
    db.close()


@pytest.mark.parametrize("geometry", ["four_passes_segments", "last_pass_28_segments"])
def test_flags_inside_a_cut_stage_are_rerun(swg, ctx, data, orc, geometry):
    """The f16 cells flag pairs INSIDE a cut stage (a list launch of the f16 form): database B behind 200 unrelated
    sequences that are longer than its planted copies, in segments, so that the copies -- above the ceiling of 4096 --
    lie in a segment behind the first.  They are flagged there, run again on the int16 cells and counted."""
    flat, off = data["B"]
    rng = np.random.default_rng(0x5EED0B03)
    lens = rng.integers(1300, 1500, size=200)
    extra = rng.choice(flat[flat > 0], size=int(lens.sum())).astype(np.int8)
    flat2 = np.concatenate([flat, extra]).astype(np.int8)
    off2 = np.concatenate([off, off[-1] + np.cumsum(lens).astype(np.uint64)]).astype(np.uint64)
    q = data["qB"] if geometry == "four_passes_segments" else data["q952"]
    truth = np.concatenate([data["truthB" if geometry == "four_passes_segments" else "truthB952"],
                            orc.score_db(q, extra, np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64), data["sub"], GO, GE)])
    n2 = len(truth)
    over = np.flatnonzero(truth > 4096)
    assert len(over) >= 10 and over.max() < N
    seg = _segment_blocks(off2)
    # the token order: pairs of consecutive sequences by length; every flagged sequence lies behind the first segment
    all_lens = np.diff(off2.astype(np.int64))
    by_len = np.sort(all_lens)[::-1]
    blocks_before = np.concatenate([[0], np.cumsum((by_len[0::2] + 2 + 3) // 4)])
    first_flagged_pair = int(np.searchsorted(-by_len, -all_lens[over].max(), side="left")) // 2
    assert blocks_before[first_flagged_pair] >= seg, (blocks_before[first_flagged_pair], seg)
    ctx.set_scoring(data["sub"], GO, GE)
    ctx.set_query(q)
    opts = {"cols_per_wave": 4, "group_lanes": 16} if geometry == "four_passes_segments" else {"cols_per_wave": 32, "group_lanes": 16}
    for key, v in {**opts, "segment_blocks": seg, "f16": 2}.items():
        ctx.set_option(key, v)
    db = swg.Database(flat2, off2).upload(ctx)
    st = _hits_both_ways(ctx, db, truth, np.arange(n2), ("flags in a cut stage", geometry), want_skips=True)
    assert st["cell_form"] == 2, st
    assert st["n_rescored"] >= (len(over) + 1) // 2, (st, len(over))   # (whether it counts pairs or sequences)
    if geometry == "last_pass_28_segments":
        assert st["passes"] == 2 and st["last_pass_cols"] == 28, st
    db.close()


def test_batch_gapless_and_list_searches_are_never_pruned(swg, ctx, data):
    """The routes pruning leaves alone, asked with prune = 2 through the searches themselves: the queries of a batch
    (swg_search_multi), the gapless prefilter and the list searches end with nothing pruned and the unpruned results."""
    flat, off = data["A"]
    ctx.set_scoring(data["sub"], GO, GE)
    ctx.set_query(data["qA"])
    db = swg.Database(flat, off).upload(ctx)
    queries = [data["qA"], data["qA"][:150].copy()]
    lists = [np.arange(0, N, 2, dtype=np.uint32), np.arange(1, N, 3, dtype=np.uint32)]
    for opts in ({}, GEOMETRIES["four_passes_segments"](off)):
        for key, v in opts.items():
            ctx.set_option(key, v)
        got = {}
        for mode in (0, 2):
            ctx.set_option("prune", mode)
            _, h_multi, _ = ctx.search_multi(db, queries, k=10, want_scores=False)
            assert not ctx.prune_last()["pruned"], ("multi", opts, mode)
            _, h_gapless, _ = ctx.search_gapless(db, want_scores=False, k=10)
            assert not ctx.prune_last()["pruned"], ("gapless", opts, mode)
            _, h_lists, _ = ctx.search_lists(db, queries, lists, k=10, want_scores=False)
            assert not ctx.prune_last()["pruned"], ("lists", opts, mode)
            got[mode] = ([list(h) for h in h_multi], list(h_gapless), [list(h) for h in h_lists])
        assert got[0] == got[2], opts
        assert got[2][0][0] == _expected(data["truthA"], np.arange(N), 10), opts
        # ... and the context prunes again right after them
        ctx.set_option("prune", 2)
        _, hits, _ = ctx.search(db, want_scores=False, k=10)
        assert ctx.prune_last()["pruned"] and hits == _expected(data["truthA"], np.arange(N), 10), opts
    db.close()


@pytest.mark.parametrize("dbkind", ["plain", "view", "shard"])
@pytest.mark.parametrize("kind", ["index", "pssm"])
def test_query_kinds_and_databases(swg, ctx, data, kind, dbkind):
    flat, off = data["A"]
    ctx.set_scoring(data["sub"], GO, GE)
    if kind == "pssm":
        ctx.set_query_pssm(data["sub"][data["qA"].astype(np.int64)])
    else:
        ctx.set_query(data["qA"])
    for key, v in GEOMETRIES["four_passes_segments"](off).items():
        ctx.set_option(key, v)
    parent = None
    if dbkind == "plain":
        want = np.arange(N)
        db = swg.Database(flat, off).upload(ctx)
    elif dbkind == "view":
        want = np.delete(np.arange(N), np.arange(0, N, 3))
        parent = swg.Database(flat, off).upload(ctx)
        db = parent.view(ctx, want)
    else:
        # a shard cut elsewhere: every other sequence, with its index in the whole database
        want = np.arange(1, N, 2)
        o64 = off.astype(np.int64)
        loc = np.concatenate([flat[o64[i]:o64[i + 1]] for i in want]).astype(np.int8)
        loff = np.zeros(len(want) + 1, dtype=np.uint64)
        loff[1:] = np.cumsum(np.diff(o64)[want])
        db = swg.Database(loc, loff, index=want.astype(np.uint32), n_total=N).upload(ctx)
    ctx.set_option("segment_blocks", _segment_blocks(off, members=want))
    members = np.array(sorted(int(v) for v in db.order() if int(v) != 0xFFFFFFFF))
    assert np.array_equal(members, want) and db.count == len(want) and db.total_count == N
    _hits_both_ways(ctx, db, data["truthA"], members, (kind, dbkind), want_skips=True)
    db.close()
    if parent is not None:
        parent.close()


def test_scores_under_prune_2_are_the_oracles_or_skipped(swg, ctx, data):
    flat, off = data["A"]
    truth = data["truthA"]
    ctx.set_scoring(data["sub"], GO, GE)
    ctx.set_query(data["qA"])
    _, u = swg.debug_prune_bound(data["sub"], data["qA"], flat, off)
    u = u.astype(np.int64)
    db = swg.Database(flat, off).upload(ctx)
    order = np.array([int(v) for v in db.order()], dtype=np.int64)
    assert len(order) == N
    for geometry in ("one_pass", "four_passes_segments"):
        _reset_options(ctx)
        ctx.set_option("autotune", 0)
        for key, v in GEOMETRIES[geometry](off).items():
            ctx.set_option(key, v)
        ctx.set_option("prune", 2)
        scores, hits, st = ctx.search(db, want_scores=True, k=10)
        info = ctx.prune_last()
        T = info["threshold"]
        assert info["pruned"] and T > 0, (geometry, info)
        assert hits == _expected(truth, np.arange(N), 10), geometry
        skipped = (scores == 0) & (truth != 0)
        assert np.array_equal(scores[~skipped], truth[~skipped]), geometry
        assert np.all(u[skipped] < T) and np.all(truth[skipped] < T), (geometry, T)
        # pairs = consecutive sequences of the sorted order; a skipped pair reports 0 for both of its sequences
        pair_skipped = skipped[order[0::2]] & skipped[order[1::2]]
        assert not np.any(skipped[order[0::2]] ^ skipped[order[1::2]]), geometry
        assert info["pairs_skipped"] == int(pair_skipped.sum()) and info["pairs_skipped"] > 0, (geometry, info)
        assert 0 < info["pair_rows_skipped"] < info["pair_rows"], info
    db.close()


def test_k_of_the_whole_database_skips_nothing(swg, ctx, data):
    flat, off = data["A"]
    ctx.set_scoring(data["sub"], GO, GE)
    ctx.set_query(data["qA"])
    db = swg.Database(flat, off).upload(ctx)
    for opts in ({}, GEOMETRIES["four_passes_segments"](off)):
        for key, v in opts.items():
            ctx.set_option(key, v)
        ctx.set_option("prune", 2)
        for k in (N, N + 7):
            _, hits, _ = ctx.search(db, want_scores=False, k=k)
            assert len(hits) == N and hits == _expected(data["truthA"], np.arange(N), k), (opts, k)
            assert ctx.prune_last()["pairs_skipped"] == 0, (opts, k)
    db.close()


def test_a_tie_at_the_kth_place_keeps_the_lower_index(swg, ctx, data):
    """The K-th and the (K+1)-th best are the same sequence twice: the hit is the one with the lower index."""
    flat, off = data["A"]
    truth = data["truthA"]
    K = 10
    kth = _expected(truth, np.arange(N), K)[-1][1]
    seq = flat[int(off[kth]):int(off[kth + 1])]
    flat2 = np.concatenate([flat, seq, seq]).astype(np.int8)           # (twice: the database keeps an even count)
    off2 = np.concatenate([off, [off[-1] + len(seq), off[-1] + 2 * len(seq)]]).astype(np.uint64)
    truth2 = np.concatenate([truth, [truth[kth], truth[kth]]])
    ctx.set_scoring(data["sub"], GO, GE)
    ctx.set_query(data["qA"])
    db = swg.Database(flat2, off2).upload(ctx)
    for opts in ({}, GEOMETRIES["four_passes_segments"](off2)):
        for key, v in opts.items():
            ctx.set_option(key, v)
        ctx.set_option("prune", 2)
        for k in (K, K + 1, K + 2):
            _, hits, _ = ctx.search(db, want_scores=False, k=k)
            assert ctx.prune_last()["pruned"]
            assert hits == _expected(truth2, np.arange(N + 2), k), (opts, k)
    ctx.set_option("prune", 2)
    _, hits, _ = ctx.search(db, want_scores=False, k=K)
    assert hits[-1] == (int(truth[kth]), kth) and all(i < N for _, i in hits)
    db.close()


def test_two_searches_in_flight_with_different_k(swg, ctx, data):
    flat, off = data["A"]
    ctx.set_scoring(data["sub"], GO, GE)
    ctx.set_query(data["qA"])
    for key, v in GEOMETRIES["four_passes_segments"](off).items():
        ctx.set_option(key, v)
    ctx.set_option("prune", 2)
    db = swg.Database(flat, off).upload(ctx)
    ctx.search(db, want_scores=False, k=1)                            # (plans and buffers exist: the two below only queue)
    t1 = ctx.search_begin(db, k=3)
    t2 = ctx.search_begin(db, k=100)
    t3 = ctx.search_begin(db, k=10)
    for t, k in ((t1, 3), (t2, 100), (t3, 10)):
        _, hits, _ = ctx.search_end(t)
        assert hits == _expected(data["truthA"], np.arange(N), k), k
        assert ctx.prune_last()["pruned"], k
    db.close()


def test_auto_leaves_small_databases_alone_and_default_scores_are_exact(swg, ctx, data):
    ctx.set_scoring(data["sub"], GO, GE)
    for name, q, truth in (("A", data["qA"], data["truthA"]), ("B", data["qB"], data["truthB"])):
        flat, off = data[name]
        ctx.set_query(q)
        db = swg.Database(flat, off).upload(ctx)
        for opts in ({}, GEOMETRIES["four_passes_segments"](off)):
            for key, v in opts.items():
                ctx.set_option(key, v)
            for k in KS:
                _, hits, _ = ctx.search(db, want_scores=False, k=k)                # prune = 1, the default
                info = ctx.prune_last()
                assert not info["pruned"] and info["pairs_skipped"] == 0 and info["pair_rows_skipped"] == 0, (name, opts, k, info)
                assert hits == _expected(truth, np.arange(N), k), (name, opts, k)
            scores, hits, _ = ctx.search(db, k=10)                                 # want_scores = True, the default
            assert np.array_equal(scores, truth) and hits == _expected(truth, np.arange(N), 10), (name, opts)
            assert ctx.prune_last()["pairs_skipped"] == 0
        _reset_options(ctx)
        ctx.set_option("autotune", 0)
        db.close()
