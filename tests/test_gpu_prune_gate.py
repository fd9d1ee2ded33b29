"""GPU (-m gpu): the gate in front of the first pruning level (option prune_gate = 2).

The first level's launch waits for a threshold -- the K-th best score behind the first stage, or a caller's -- and a pair
whose colmax bound U_1 is below it is not walked.  Every case: the hits are those of the same search with prune_gate = 1
and the oracle's; swg_prune_last is that search's field for field; the pair bounds follow the mirror rule of
prune_gate_cases.expected_bounds exactly; each stage's list is the pairs whose bound reaches its T."""
import numpy as np
import pytest

from prune_gate_cases import CASES, GE, GO, NOT_BOUNDED, expected_bounds, make_data, pair_sequences
from test_gpu_parity import _reset_options

pytestmark = pytest.mark.gpu

PRUNE_KEYS = ("prune_kmer", "prune_segments", "prune_refine", "prune_cut", "prune_refine3", "prune_refine4", "prune_table_bits", "prune_gate")


@pytest.fixture(autouse=True)
def _options(ctx):
    def reset():
        _reset_options(ctx)
        ctx.set_option("prune", 1)
        ctx.set_option("prune_head", 4)
        for key in PRUNE_KEYS:
            ctx.set_option(key, 0)

    reset()
    ctx.set_option("autotune", 0)
    yield
    reset()
    ctx.set_option("autotune", 1)


@pytest.fixture(scope="module")
def data(swg):
    return make_data(swg)


def _sub(swg):
    return np.asarray(swg.load_scoring("BLOSUM62").table(), dtype=np.int8).reshape(32, 32)


def _oracle_scores(orc, swg, data, name):
    """The oracle's scores of a database, computed once and left alone"""
    key = ("oracle", name)
    if key not in data["cache"]:
        flat, off = data[name]
        scores = orc.score_db(data["q"], flat, off, _sub(swg), GO, GE)
        scores.setflags(write=False)
        data["cache"][key] = scores
    return data["cache"][key]


def _open(swg, ctx, data, which):
    """-> (the database object to search, what to close, its sequences (flat, off), the oracle's name for them)"""
    if which == "view":
        flat, off = data["main"]
        whole = swg.Database(flat, off).upload(ctx)
        members = np.arange(0, len(off) - 1, 3, dtype=np.uint32)
        return whole.view(ctx, members), [whole], flat, off, "main"
    if which == "shard":
        flat, off = data["main"]
        return swg.Database(flat, off, shard_rank=1, shard_count=2).upload(ctx), [], flat, off, "main"
    flat, off = data[which]
    return swg.Database(flat, off).upload(ctx), [], flat, off, which


def _geometry(ctx, off):
    """Four passes, and launch segments of the first stage's size: the 30 longest pairs"""
    lens = np.sort(np.diff(off.astype(np.int64)))[::-1]
    blocks = (lens[0::2] + 2 + 3) // 4
    for key, v in {"cols_per_wave": 4, "group_lanes": 16, "segment_blocks": int(blocks[:30].sum())}.items():
        ctx.set_option(key, v)


def _search(ctx, db, route, T):
    if route[0] == "topk":
        return ctx.search(db, want_scores=False, k=route[1])[1]
    hits, total, _ = ctx.search_above(db, T)
    return hits, total


@pytest.mark.parametrize("label", sorted(CASES))
def test_gated_search_is_the_ungated_one(swg, orc, ctx, data, label):
    which, kind, options, route = CASES[label]
    sub, q = _sub(swg), data["q"]
    ctx.set_scoring(sub, GO, GE)
    if kind == "pssm":
        ctx.set_query_pssm(sub[q.astype(np.int64)].copy())   # (the same scores column by column: the oracle's hits hold)
    else:
        ctx.set_query(q)
    db, also, flat, off, oname = _open(swg, ctx, data, which)
    order = np.array([int(v) for v in db.order()], dtype=np.int64)
    members = order[order != NOT_BOUNDED]
    pflat, poff = pair_sequences(order, flat, off)
    u = swg.debug_prune_bound(sub, q, pflat, poff)[1].astype(np.int64)
    u1 = np.maximum(u[0::2], u[1::2])
    n = len(u1)
    scores = _oracle_scores(orc, swg, data, oname)
    mine = np.full(len(scores), -1, dtype=np.int32)
    mine[members] = scores[members]
    _geometry(ctx, off)
    ctx.set_option("prune", 2)
    for key, v in options.items():
        ctx.set_option(key, v)
    fixed = route[0] == "above"
    T = 0
    if fixed:
        # inside the range: the tenth best score; over every bound: one more than the largest first-level bound
        ctx.set_option("prune_gate", 1)
        ctx.search(db, want_scores=False, k=10)
        T = orc.topk(mine, 10)[-1][0] if route[1] == "inside" else int(ctx.debug_prune_refine_read(db)["bounds"][:n].max()) + 1
    got = {}
    for gate in (1, 2):
        ctx.set_option("prune_gate", gate)
        hits = _search(ctx, db, route, T)
        info = ctx.prune_last()
        assert info["pruned"] and ctx.debug_prune_gate() == (gate == 2), (label, gate)
        read = ctx.debug_prune_refine_read(db)
        assert (read["k"], read["segments"]) == (options["prune_kmer"], options["prune_segments"])
        got[gate] = (hits, info, read["bounds"].astype(np.int64), read["stages"])
    (hits1, info1, b1, st1), (hits2, info2, b2, st2) = got[1], got[2]
    print(label, "T of the gate", st2[0][2] if st2 else None, "pairs", n, "left at the gate",
          int(np.sum(u1[st2[0][0]:] < st2[0][2])) if st2 else 0, info2)
    # the hits
    assert hits2 == hits1, label
    if fixed:
        want = sorted(((int(mine[i]), int(i)) for i in np.flatnonzero(mine >= T)), key=lambda h: (-h[0], h[1]))
        assert hits2[1] == len(want) and sorted(((int(s), int(i)) for s, i in hits2[0]), key=lambda h: (-h[0], h[1])) == want, label
        assert (len(want) == 0) == (route[1] == "over")
    else:
        assert hits2 == orc.topk(mine, min(route[1], len(members))), label
    # what the search left out
    assert info2 == info1, (label, info1, info2)
    # the stages and their lists: the same stages under the same thresholds, the same pairs kept
    assert [(b, e, t) for b, e, t, _ in st2] == [(b, e, t) for b, e, t, _ in st1], label
    for (b, e, t, l1), (_, _, _, l2) in zip(st1, st2):
        assert np.array_equal(l1, l2), (label, b)
        assert np.array_equal(l2.astype(np.int64), b + np.flatnonzero(b2[b:e] >= t)), (label, b)
    # the bounds: the mirror rule
    want = expected_bounds(b1[:n], u1, st2, fixed)
    assert np.array_equal(b2[:n], want), (label, np.flatnonzero(b2[:n] != want)[:5])
    assert np.array_equal(b2[n:], b1[n:]) or not st2
    if label == "k_at_least_n":
        assert st2 and all(t == 0 for _, _, t, _ in st2) and np.array_equal(b2[st2[0][0]:n], b1[st2[0][0]:n])
    elif label == "above_over_every_bound":
        assert all(len(l) == 0 for _, _, _, l in st2) and hits2[1] == 0
    elif st2:
        begin, Tg = st2[0][0], st2[0][2]
        assert Tg > 0 and len(st2) >= (1 if label == "head_and_rest" else 3)
        if not fixed:
            assert begin > 0 and np.all(b2[:begin] == NOT_BOUNDED)
        # T falls inside the range: pairs that leave at the gate, and pairs that reach it and are cut by the walk
        assert np.any(u1[begin:] < Tg), label
        assert np.any((u1[begin:] >= Tg) & (b2[begin:n] < Tg)), label
    if label == "s32":
        # ... and the ungated search's are the first level's mirror
        m = swg.debug_prune_kmer_seg(sub, q, GO, GE, 4, 32, pflat, poff, table=False)[1].astype(np.int64)
        assert np.array_equal(b1[:n], np.maximum(m[0::2], m[1::2]))
    if which in ("long_short", "main"):
        # a pair shorter than one chunk of the walk and one longer, and a pair beside a much shorter partner
        lens = np.diff(poff.astype(np.int64))[0::2]
        ylens = np.array([np.count_nonzero(pflat[int(poff[2 * i + 1]):int(poff[2 * i + 2])]) for i in range(n)])
        assert np.any(lens < 100) and np.any(lens > 200)
        if which == "long_short":
            assert np.any((lens >= 200) & (ylens <= 80)) and np.any((lens >= 60) & (ylens <= 4))
    db.close()
    for d in also:
        d.close()
