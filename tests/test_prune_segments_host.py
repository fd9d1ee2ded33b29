"""CPU: the segmented, ordered form of the k-mer pruning bound, through its host mirror
(swg_debug_prune_kmer_seg) and the choice of (k, S) (swg_debug_prune_kmer_choice_seg).

The query's columns are cut into S segments of W = ceil(lq / S) columns.  The table holds, for every class block, its
best cell within each segment; a sequence's blocks are taken in order with H[s] = max_{s' <= s} H[s'] + min(T[block][s],
the block's colmax sum), and U_{k,S} = max_s H[s].  One segment is the unsegmented bound entry for entry; the maximum of
a block's S entries is its unsegmented entry; U_{k,S} covers the oracle's score; and a finer cut of the columns never
gives a larger bound.  That the recurrence runs the right way is checked on its own: validity would not notice."""
import numpy as np
import pytest

GAPS = [(-2, -1), (0, 0), (-11, -1)]
KS = [4, 5]
SEGMENTS = [1, 2, 3, 8, 32]
LQS = [1, 7, 75, 200]
C = 22


def _table(swg, name):
    return np.asarray(swg.load_scoring(name).table(), dtype=np.int8).reshape(32, 32)


def _database(rng, letters):
    """60 sequences of 1..140 residues: below k, around 4, 5 and 20, the longest; residues of class 21 among them."""
    lens = rng.integers(1, 141, size=60)
    lens[:16] = [1, 2, 3, 4, 5, 6, 7, 17, 18, 19, 20, 21, 22, 23, 139, 140]
    off = np.zeros(61, dtype=np.uint64)
    off[1:] = np.cumsum(lens)
    flat = rng.choice(letters, size=int(off[-1])).astype(np.int8)
    return flat, off


def _boundaries(lq, S):
    W = -(-lq // S)
    return set(range(W, lq, W))


@pytest.fixture(scope="module")
def base(swg, orc):
    """(matrix, gaps, lq) -> (table, query, database, oracle scores): shared by every k and S."""
    cache = {}

    def get(matrix, gaps, lq):
        key = (matrix, gaps, lq)
        if key not in cache:
            sub = _table(swg, matrix)
            rng = np.random.default_rng(len(matrix) * 1000 + lq * 10 - gaps[0])
            letters = np.array([i for i in range(1, 27)] + [31])
            cls = np.array(swg.KMER_CLASS)
            assert np.any(cls[letters] == 21)
            q = rng.choice(letters, size=lq).astype(np.int8)
            flat, off = _database(rng, letters)
            assert np.any(cls[flat.astype(np.int64)] == 21)
            scores = orc.score_db(q, flat, off, sub, gaps[0], gaps[1]).astype(np.int64)
            cache[key] = (sub, q, flat, off, scores)
        return cache[key]

    return get


@pytest.mark.parametrize("lq", LQS)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("gaps", GAPS)
@pytest.mark.parametrize("matrix", ["BLOSUM62", "PAM250"])
def test_segmented_table_and_bound(swg, base, matrix, gaps, k, lq):
    sub, q, flat, off, scores = base(matrix, gaps, lq)
    t1, u1 = swg.debug_prune_kmer(sub, q, gaps[0], gaps[1], k, flat, off)
    u1 = u1.astype(np.int64)
    us = {}
    for S in SEGMENTS:
        t, u = swg.debug_prune_kmer_seg(sub, q, gaps[0], gaps[1], k, S, flat, off)
        assert t.shape == (C ** k, S)
        u = u.astype(np.int64)
        if S == 1:
            # one segment: the unsegmented mirror, entry for entry
            assert np.array_equal(t[:, 0], t1) and np.array_equal(u, u1), (matrix, gaps, k, lq)
        # the best of a block's segments is its unsegmented entry
        assert np.array_equal(t.max(axis=1), t1), (matrix, gaps, k, lq, S)
        # a segment without columns holds 0
        W = -(-lq // S)
        empty = [s for s in range(S) if s * W >= lq]
        assert not np.any(t[:, empty]), (lq, S, empty)
        assert (lq >= S) or empty
        # the bound covers the oracle's score, and the unsegmented bound covers it
        assert np.all(u >= scores), (matrix, gaps, k, lq, S, int((scores - u).max()))
        assert np.all(u <= u1), (matrix, gaps, k, lq, S)
        us[S] = u
        del t
    # a finer cut never gives a larger bound
    refined = 0
    for S in SEGMENTS:
        for S2 in SEGMENTS:
            if S2 != S and _boundaries(lq, S2) <= _boundaries(lq, S):
                assert np.all(us[S] <= us[S2]), (matrix, gaps, k, lq, S, S2)
                refined += _boundaries(lq, S2) < _boundaries(lq, S)
    if lq == 200:
        assert _boundaries(200, 2) < _boundaries(200, 8) and refined >= 5
        # unrelated sequences under dear gaps: the order is worth something (free gaps carry a block's best cell into
        # every later segment: nothing to gain there)
        if gaps == (-11, -1):
            assert us[8].sum() < us[2].sum() < us[1].sum(), (matrix, gaps, k)
    if lq == 75:
        assert 75 % 8 and _boundaries(75, 8) == set(range(10, 75, 10))     # (S does not divide lq; the last segment is short)


@pytest.mark.parametrize("k", KS)
def test_the_order_of_the_blocks(swg, k):
    """A query of 20 W then 20 C, two segments; gaps and the W / C mismatch too dear for a cell of one half to reach the other.  Blocks of W
    score in the first segment only, blocks of C in the second only.  W..WC..C gets the sum of its blocks' entries --
    its true score --, C..CW..W strictly less: the better half.  Unsegmented, both get the sum.  A recurrence that runs
    the wrong way, or lets the segment decrease, gets these the other way round."""
    sub = _table(swg, "BLOSUM62").copy()
    Wr, Cr = ord("W") - 64, ord("C") - 64
    sub[Wr, Cr] = sub[Cr, Wr] = -128
    cls = swg.KMER_CLASS
    q = np.array([Wr] * 20 + [Cr] * 20, dtype=np.int8)
    n = 6 if k == 4 else 8           # token rows: two reset rows, n W, n C, padding -- whole blocks of k of one residue each
    pq = np.array([Wr] * n + [Cr] * n, dtype=np.int8)
    qp = pq[::-1].copy()
    flat = np.concatenate([pq, qp])
    off = np.array([0, 2 * n, 4 * n], dtype=np.uint64)
    go, ge = -100, -100
    sw, sc = int(sub[Wr, Wr]), int(sub[Cr, Cr])
    assert sw > 0 and sc > 0 and sub[Wr, Cr] < 0
    t, u = swg.debug_prune_kmer_seg(sub, q, go, ge, k, 2, flat, off)
    ix = lambda d: int(np.ravel_multi_index(d, (C,) * k))  # noqa: E731
    P, Q = ix([cls[Wr]] * k), ix([cls[Cr]] * k)
    assert list(t[P]) == [k * sw, 0] and list(t[Q]) == [0, k * sc]
    total = n * sw + n * sc
    assert int(u[0]) == total                                  # P.Q: every block in its own half, in order
    assert int(u[1]) == max(n * sw, n * sc) < total            # Q.P: one half or the other
    t1, u1 = swg.debug_prune_kmer_seg(sub, q, go, ge, k, 1, flat, off)
    assert int(u1[0]) == total and int(u1[1]) == total
    # the blocks of P.Q, entry by entry: reset rows and padding take their place in the first and last block
    if k == 4:
        blocks = [([0, 0] + [cls[Wr]] * 2, 0), ([cls[Wr]] * 4, 0), ([cls[Cr]] * 4, 1), ([cls[Cr]] * 2 + [0, 0], 1)]
    else:
        blocks = [([0, 0] + [cls[Wr]] * 3, 0), ([cls[Wr]] * 5, 0), ([cls[Cr]] * 5, 1), ([cls[Cr]] * 3 + [0, 0], 1)]
    assert sum(int(t[ix(b), s]) for b, s in blocks) == total
    # three segments of 14 columns: W holds the first and part of the second, C part of the second and the third
    _, u3 = swg.debug_prune_kmer_seg(sub, q, go, ge, k, 3, flat, off, table=False)
    assert int(u3[0]) == total and int(u3[1]) == total         # (both kinds of block score in the middle segment)


def test_choice_of_k_and_segments(swg):
    ch = swg.debug_prune_kmer_choice_seg
    # an unpruned search builds nothing, whatever is forced
    for forced in (0, 1, 4, 5):
        for S in (0, 1, 8, 32):
            assert ch(forced=forced, segments=S, pruned=0)[:3] == (0, 0, 0)
    # a forced k with the segments left automatic is the unsegmented bound, on any range
    for forced in (1, 4, 5):
        for rows in (1, 10 ** 4, 10 ** 10):
            k, S, size, ok = ch(forced=forced, segments=0, lq=100, pair_rows=rows)
            assert (k, S, ok) == (forced, 1, True) and size == (0 if forced == 1 else 2 * C ** forced)
            assert swg.debug_prune_kmer_choice(forced=forced, lq=100, pair_rows=rows) == forced
    # both forced: as they are; the colmax bound has no table to segment
    assert ch(forced=4, segments=32)[:2] == (4, 32) and ch(forced=5, segments=8)[:2] == (5, 8) and ch(forced=1, segments=8)[:2] == (1, 1)
    # the budget: (5, 8) is within it, (5, 10) and (5, 32) are refused, every S of k = 4 is admitted
    assert swg.KMER_TABLE_BUDGET == 96 << 20
    assert ch(forced=5, segments=8)[2:] == (2 * 8 * C ** 5, True) and 2 * 8 * C ** 5 <= swg.KMER_TABLE_BUDGET
    for S in (10, 16, 32):
        k, S_, size, ok = ch(forced=5, segments=S)
        assert (k, S_) == (5, S) and size > swg.KMER_TABLE_BUDGET and not ok
    assert all(ch(forced=4, segments=S)[3] for S in range(1, 33))
    # forced segments with k automatic: the k of the unsegmented rule, stepped down where (5, S) is beyond the budget
    assert ch(segments=8)[:2] == (5, 8) and ch(segments=32) == (4, 32, 2 * 32 * C ** 4, True) and ch(segments=1)[:2] == (5, 1)
    assert ch(segments=8, lq=200, pair_rows=300000)[:2] == (1, 1)
    # both automatic: a candidate of the fixed list, within the budget; small ranges take the colmax bound as before
    cands = {(1, 1), (4, 1), (5, 1), (4, 16), (4, 32), (5, 8)}
    for lq in (50, 300, 3000, 30000):
        for rows in (0, 10 ** 5, 10 ** 7, 10 ** 9, 10 ** 10):
            k, S, _, ok = ch(lq=lq, pair_rows=rows)
            assert (k, S) in cands and ok, (lq, rows, k, S)
            # the hook without segments keeps its unsegmented meaning: prune_segments = 1
            assert swg.debug_prune_kmer_choice(lq=lq, pair_rows=rows) == ch(segments=1, lq=lq, pair_rows=rows)[0]
    assert ch(lq=200, pair_rows=300000)[:2] == (1, 1) and ch(lq=3000, pair_rows=0)[:2] == (1, 1)
    # the flagship: k = 4 in 32 segments, which measured best both with the table resident and behind a new query
    assert ch(lq=3000, pair_rows=1900000000) == (4, 32, 2 * 32 * C ** 4, True)
    # ... and more rows or fewer columns never take a candidate that saves less
    gains = {(1, 1): 0, (4, 1): 1, (5, 1): 2, (4, 16): 3, (4, 32): 4, (5, 8): 5}
    got = [gains[ch(lq=1000, pair_rows=r)[:2]] for r in (10 ** 4, 10 ** 5, 10 ** 6, 10 ** 7, 10 ** 8, 10 ** 9, 10 ** 10, 10 ** 11)]
    assert got == sorted(got) and got[0] == 0 and got[-1] >= 4, got
    rates = dict(table_rate=10 ** 12, fill_rate=10 ** 9, pair_rows=2 * 10 ** 8)   # (fixed rates: only the tables grow with lq)
    got = [gains[ch(lq=lq, **rates)[:2]] for lq in (50, 100, 400, 1000, 3000, 100000, 10 ** 7)]
    assert got == sorted(got, reverse=True) and got[0] >= 4 and got[-1] == 0, got


def test_argument_errors(swg):
    import ctypes as C_
    sub = _table(swg, "BLOSUM62")
    u = np.zeros(1, dtype=np.uint64)
    off = np.array([0, 1], dtype=np.uint64)
    one = np.array([1], dtype=np.int8)
    p = lambda a: a.ctypes.data_as(C_.c_void_p)  # noqa: E731
    f = swg.lib.swg_debug_prune_kmer_seg
    assert f(None, p(one), 1, -2, -1, 4, 2, p(one), p(off), 1, None, p(u)) == swg.SWG_ERR_ARG
    assert f(p(sub), p(one), 0, -2, -1, 4, 2, p(one), p(off), 1, None, p(u)) == swg.SWG_ERR_ARG
    assert f(p(sub), p(one), 1, -2, -1, 3, 2, p(one), p(off), 1, None, p(u)) == swg.SWG_ERR_ARG
    assert f(p(sub), p(one), 1, -2, -1, 4, 0, p(one), p(off), 1, None, p(u)) == swg.SWG_ERR_ARG
    assert f(p(sub), p(one), 1, -2, -1, 4, 33, p(one), p(off), 1, None, p(u)) == swg.SWG_ERR_ARG
    assert f(p(sub), p(one), 1, 1, -1, 4, 2, p(one), p(off), 1, None, p(u)) == swg.SWG_ERR_ARG
    assert f(p(sub), p(one), 1, -2, -1, 4, 2, p(one), p(off), 1, None, None) == swg.SWG_ERR_ARG
    # one column, 32 segments: the one residue scores in the first segment, the others hold 0
    assert f(p(sub), p(one), 1, -2, -1, 4, 32, p(one), p(off), 1, None, p(u)) == swg.SWG_OK and u[0] == sub[1, 1]
