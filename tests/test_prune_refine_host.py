"""CPU: the second level of the pruning bound and the pair-by-pair cut, through the host mirror
(swg_debug_prune_kmer_refine), the choice (swg_debug_prune_refine_choice) and the list rule restated in numpy.

The second level walks a sequence's blocks of 4 rows in order over a k = 4 table of S2 = 64 or 128 segments of the
query's columns: the same recurrence as the first level's, so its bound covers the oracle's score, never exceeds the
unordered sum, and at S2 = 32 is the first level's mirror entry for entry.  The database and queries are those of
test_gpu_prune.py's `data` fixture (database A and its 200-column query)."""
import ctypes as C_

import numpy as np
import pytest

from test_gpu_prune import GE, GO, N

C = 22


@pytest.fixture(scope="module")
def base(swg, orc):
    sub = np.asarray(swg.load_scoring("BLOSUM62").table(), dtype=np.int8).reshape(32, 32)
    qA = swg.synth_query(0x5EED0A01, 200)
    flat, off = swg.synth_db(0x5EED0A02, N, median=60, max_len=600, query=qA, fraction=0.01, subst=0.05)[:2]
    cache = {}

    def get(lq, kind):
        """-> (rows, query or None, gaps, oracle scores) of the index query's first lq columns, or of its PSSM under -11 / -1"""
        if (lq, kind) not in cache:
            q = qA[:lq].copy()
            gaps = (GO, GE) if kind == "index" else (-11, -1)
            scores = orc.score_db(q, flat, off, sub, gaps[0], gaps[1]).astype(np.int64)
            cache[(lq, kind)] = (sub, q, gaps, scores) if kind == "index" else (sub[q.astype(np.int64)].copy(), None, gaps, scores)
        return cache[(lq, kind)]

    return flat, off, get


@pytest.mark.parametrize("kind", ["index", "pssm"])
@pytest.mark.parametrize("lq", [200, 100])
def test_refine_mirror_is_a_bound(swg, base, lq, kind):
    flat, off, get = base
    rows, q, gaps, scores = get(lq, kind)
    _, u1 = swg.debug_prune_kmer_seg(rows, q, gaps[0], gaps[1], 4, 1, flat, off, table=False)
    u1 = u1.astype(np.int64)
    prev = u1
    for S2 in (64, 128):
        t, u = swg.debug_prune_kmer_refine(rows, q, gaps[0], gaps[1], S2, flat, off)
        u = u.astype(np.int64)
        assert t.shape == (C ** 4, S2)
        assert np.all(u >= scores), (lq, kind, S2, int((scores - u).max()))
        assert np.all(u <= u1), (lq, kind, S2)
        W = -(-lq // S2)
        empty = [s for s in range(S2) if s * W >= lq]
        assert not np.any(t[:, empty])
        if lq == 100 and S2 == 128:
            assert W == 1 and len(empty) == 28 and np.any(t[:, 99])
        if lq == 200 and S2 == 128:
            # 2-column segments refine the 4-column segments of S2 = 64 (200 = 50 x 4 = 100 x 2): never a larger bound
            assert np.all(u <= prev)
        prev = u
    if kind == "pssm":
        assert u.sum() < u1.sum()       # (dear gaps, unrelated sequences: the order is worth something)


def test_refine_mirror_at_32_segments_is_the_first_level(swg, base):
    flat, off, get = base
    rows, q, gaps, _ = get(200, "index")
    t, u = swg.debug_prune_kmer_refine(rows, q, gaps[0], gaps[1], 32, flat, off)
    t32, u32 = swg.debug_prune_kmer_seg(rows, q, gaps[0], gaps[1], 4, 32, flat, off)
    assert np.array_equal(t, t32) and np.array_equal(u, u32)


@pytest.mark.parametrize("S2", [129, 48, 0, 1, 16, 256])
def test_other_segment_counts_are_refused(swg, S2):
    sub = np.asarray(swg.load_scoring("BLOSUM62").table(), dtype=np.int8).reshape(32, 32)
    u = np.zeros(1, dtype=np.uint64)
    off = np.array([0, 1], dtype=np.uint64)
    one = np.array([1], dtype=np.int8)
    p = lambda a: a.ctypes.data_as(C_.c_void_p)  # noqa: E731
    f = swg.lib.swg_debug_prune_kmer_refine
    assert f(p(sub), p(one), 1, -2, -1, S2, p(one), p(off), 1, None, p(u)) == swg.SWG_ERR_ARG
    assert f(p(sub), p(one), 1, -2, -1, 128, p(one), p(off), 1, None, p(u)) == swg.SWG_OK and u[0] == sub[1, 1]
    assert f(p(sub), p(one), 1, 1, -1, 128, p(one), p(off), 1, None, p(u)) == swg.SWG_ERR_ARG
    assert f(None, p(one), 1, -2, -1, 128, p(one), p(off), 1, None, p(u)) == swg.SWG_ERR_ARG


def test_choice_of_refinement(swg):
    ch = swg.debug_prune_refine_choice
    # the headline: k = 4 in 32 segments, refined
    k, S, S2 = ch(lq=3000, pair_rows=1900000000)
    assert (k, S) == (4, 32) and S2 in (64, 128)
    # the first level is what debug_prune_kmer_choice_seg says, whatever the refinement
    for kw in (dict(), dict(forced=4), dict(forced=5, segments=8), dict(segments=32), dict(lq=200, pair_rows=300000)):
        for refine in (0, 1, 64, 128):
            assert ch(refine=refine, **kw)[:2] == swg.debug_prune_kmer_choice_seg(**kw)[:2]
    # a forced prune_kmer or prune_segments: off, unless forced itself
    for kw in (dict(forced=4), dict(forced=4, segments=32), dict(segments=32), dict(forced=1), dict(forced=5, segments=8)):
        assert ch(**kw)[2] == 0, kw
        assert ch(refine=64, **kw)[2] == 64 and ch(refine=128, **kw)[2] == 128 and ch(refine=1, **kw)[2] == 0, kw
    # off is off; an unpruned search builds nothing
    assert ch(refine=1, lq=3000, pair_rows=1900000000) == (4, 32, 0)
    assert ch(pruned=0) == (0, 0, 0) and ch(pruned=0, refine=128) == (0, 0, 0)
    # a few thousand pair rows: the colmax bound and no second level
    assert ch(lq=200, pair_rows=5000) == (1, 1, 0)
    # more rows never take a second level that saves less
    got = [ch(lq=3000, pair_rows=r)[2] for r in (10 ** 4, 10 ** 6, 10 ** 8, 10 ** 9, 10 ** 10, 10 ** 11)]
    assert got == sorted(got) and got[0] == 0 and got[-1] > 0, got
    # values that are no option
    a = np.array([0, 1, 3000, 10 ** 9, 0, 0, 0, 32], dtype=np.int64)
    out = np.zeros(3, dtype=np.int64)
    assert swg.lib.swg_debug_prune_refine_choice(a.ctypes.data_as(C_.c_void_p), out.ctypes.data_as(C_.c_void_p)) == swg.SWG_ERR_ARG


def test_the_list_of_a_stage(swg):
    """The compaction rule against a hand-made bound array: the ids with bound >= T, ascending, within the stage only."""
    b = np.array([9, 3, 7, 7, 0, 8, 2, 7, 1, 6], dtype=np.uint32)
    assert list(swg.prune_list(b, 0, 10, 7)) == [0, 2, 3, 5, 7]
    assert list(swg.prune_list(b, 2, 8, 7)) == [2, 3, 5, 7]                   # a stage of its own range
    assert list(swg.prune_list(b, 4, 5, 7)) == [] and list(swg.prune_list(b, 0, 10, 10)) == []   # all below
    assert list(swg.prune_list(b, 0, 10, 0)) == list(range(10))               # T = 0: all of them, a bound of 0 too
    assert list(swg.prune_list(b, 2, 4, 7)) == [2, 3]                         # all above
    assert list(swg.prune_list(b, 3, 3, 0)) == []                             # an empty stage
    # a skipped pair in front of a kept one: what the prefix of the length order would have filled
    kept = swg.prune_list(b, 0, 10, 7)
    assert 1 not in kept and kept[-1] == 7 and len(kept) < kept[-1] + 1
    assert swg.prune_list(b, 0, 10, 7).dtype == np.uint32
