"""CPU: the k-mer form of the pruning bound, through its host mirror (swg_debug_prune_kmer) and the
choice of k (swg_debug_prune_kmer_choice).

A sequence's token rows -- two reset rows, then its residues -- are cut into blocks of k rows, and U_k is the sum of the
blocks' own local scores against the whole query, read from a table over residue CLASSES (0 padding, 1..20 the standard
amino acids, 21 every other index under the best of their scores).  With non-positive gap scores U_k >= the local
score, and U_k <= U_1, the colmax bound.  The table's entries are checked against the oracle block by block, the bound
against the oracle sequence by sequence."""
import numpy as np
import pytest

GAPS = [(-2, -1), (0, 0), (-11, -1)]
KS = [4, 5]
C = 22
OTHER = 24   # X stands for class 21 in the oracle's table (its column there: the best of the merged residues)


def _table(swg, name):
    return np.asarray(swg.load_scoring(name).table(), dtype=np.int8).reshape(32, 32)


def _random_db(rng, n, lo, hi, residues):
    lens = rng.integers(lo, hi + 1, size=n)
    lens[:min(n, 8)] = [1, 2, 3, 4, 5, 7, hi - 1, hi][:min(n, 8)]   # (below k, around the block sizes, the longest)
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens)
    flat = rng.choice(residues, size=int(off[-1])).astype(np.int8)
    return flat, off


def _classes(swg):
    cls = np.array(swg.KMER_CLASS, dtype=np.int64)
    std = [int(np.flatnonzero(cls == c)[0]) for c in range(1, 21)]
    merged = [int(r) for r in np.flatnonzero(cls == 21)]
    assert cls[0] == 0 and len(std) == 20 and sorted(std + merged) == list(range(1, 32))
    assert "".join(chr(ord("A") + r - 1) for r in std) == "ACDEFGHIKLMNPQRSTVWY"
    return cls, std, merged


def _merged_table(sub, merged):
    """The table whose column OTHER is, row by row, the best of the merged residues' columns: class 21 as a residue."""
    m = sub.copy()
    m[:, OTHER] = sub[:, merged].max(axis=1)
    return m


def _digits(ix, k):
    out = []
    for _ in range(k):
        out.append(ix % C)
        ix //= C
    return out[::-1]


def _index(digits):
    ix = 0
    for d in digits:
        ix = ix * C + int(d)
    return ix


def _u_restated(swg, t, cm, seq, k):
    """U_k of one sequence (a 0 in it: a padding row) from the table and colmax: its token rows -- two reset rows first,
    padded to whole blocks of 4 -- in blocks of 4, or of 5 over every whole 20 rows and of 4 over the rest; a block adds
    the lesser of its entry and its rows' colmax entries."""
    cls = np.array(swg.KMER_CLASS, dtype=np.int64)
    rows = np.concatenate([[0, 0], np.asarray(seq, dtype=np.int64)])
    rows = np.concatenate([rows, np.zeros(-len(rows) % 4, dtype=np.int64)])
    cm = np.asarray(cm, dtype=np.int64)
    n5 = 20 * (len(rows) // 20) if k == 5 else 0
    cuts = list(range(0, n5, 5)) + list(range(n5, len(rows) + 1, 4))
    u = 0
    for a, b in zip(cuts[:-1], cuts[1:]):
        u += min(int(t[_index(list(cls[rows[a:b]]) + [0] * (k - (b - a)))]), int(cm[rows[a:b]].sum()))
    return u


@pytest.fixture(scope="module")
def mirror(swg):
    """(matrix, gaps, k) -> (query, table, database, U_k): every case's table is built once."""
    cache = {}

    def get(matrix, gaps, k):
        key = (matrix, gaps, k)
        if key not in cache:
            sub = _table(swg, matrix)
            rng = np.random.default_rng(len(matrix) * 100 - gaps[0])
            letters = np.array([i for i in range(1, 27)] + [31])
            q = rng.choice(letters, size=75).astype(np.int8)
            flat, off = _random_db(rng, 60, 1, 140, letters)
            t, u = swg.debug_prune_kmer(sub, q, gaps[0], gaps[1], k, flat, off)
            cache[key] = (sub, q, t, flat, off, u.astype(np.int64))
        return cache[key]

    return get


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("gaps", GAPS)
@pytest.mark.parametrize("matrix", ["BLOSUM62", "PAM250"])
def test_table_entries_are_the_blocks_oracle_scores(swg, orc, mirror, matrix, gaps, k):
    sub, q, t, _, _, _ = mirror(matrix, gaps, k)
    cls, std, merged = _classes(swg)
    assert t.size == C ** k
    rng = np.random.default_rng(k * 1000 + len(matrix) - gaps[0])
    # whole blocks of classes 1..21 (class 21 in a good share of them), and blocks with a padding tail
    blocks = [list(rng.integers(1, C, size=k)) for _ in range(150)]
    blocks += [list(rng.choice([1, 5, 21], size=k)) for _ in range(30)]
    tails = [b[:int(rng.integers(1, k))] for b in blocks[:60]]
    rep = np.array([0] + std + [OTHER], dtype=np.int8)           # class -> the residue that stands for it
    seqs = blocks + tails
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    flat = np.concatenate([rep[np.asarray(s, dtype=np.int64)] for s in seqs]).astype(np.int8)
    want = orc.score_db(q, flat, off, _merged_table(sub, merged), gaps[0], gaps[1]).astype(np.int64)
    got = np.array([int(t[_index(s + [0] * (k - len(s)))]) for s in seqs], dtype=np.int64)
    assert np.array_equal(got, want), (matrix, gaps, k, int(np.abs(got - want).max()))
    assert want.max() > 0
    # a block with a padding tail is its prefix: the entry of the shorter table index, whatever follows the first padding row
    for s in tails:
        assert t[_index(s + [0] * (k - len(s)))] == got[seqs.index(s)]
    assert t[0] == 0
    if k == 5:
        # ... and in the table of 5 a block of 4 rows is the table of 4's entry
        t4 = mirror(matrix, gaps, 4)[2]
        assert np.array_equal(t.reshape(-1, C)[:, 0], t4)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("gaps", GAPS)
@pytest.mark.parametrize("matrix", ["BLOSUM62", "PAM250"])
def test_bound_covers_the_oracle_score_and_is_below_colmax(swg, orc, mirror, matrix, gaps, k):
    sub, q, t, flat, off, u = mirror(matrix, gaps, k)
    lens = np.diff(off.astype(np.int64))
    assert lens.min() < k and np.any(lens % 4 != 0) and np.any(lens % 5 != 0) and lens.max() > 100
    scores = orc.score_db(q, flat, off, sub, gaps[0], gaps[1]).astype(np.int64)
    assert np.all(u >= scores), (matrix, gaps, k, int((scores - u).max()))
    assert scores.max() > 0
    cm, u1 = swg.debug_prune_bound(sub, q, flat, off)
    assert np.all(u <= u1.astype(np.int64)), (matrix, gaps, k)
    assert u.sum() < u1.astype(np.int64).sum()
    for i in range(len(lens)):
        assert _u_restated(swg, t, cm, flat[int(off[i]):int(off[i + 1])], k) == u[i], (i, int(lens[i]))


@pytest.mark.parametrize("k", KS)
def test_residues_outside_the_table(swg, orc, k):
    """Indices 27..30 have no letter: random scores, some positive, in both the query and the database.  They are class 21."""
    rng = np.random.default_rng(7)
    sub = _table(swg, "BLOSUM62").copy()
    sub[27:31, 1:] = rng.integers(-6, 7, size=(4, 31))
    sub[1:, 27:31] = rng.integers(-6, 7, size=(31, 4))
    every = np.arange(1, 32)
    q = rng.choice(every, size=60).astype(np.int8)
    flat, off = _random_db(rng, 50, 1, 120, every)
    _, u1 = swg.debug_prune_bound(sub, q, flat, off)
    for go, ge in GAPS:
        _, u = swg.debug_prune_kmer(sub, q, go, ge, k, flat, off, table=False)
        assert np.all(u.astype(np.int64) >= orc.score_db(q, flat, off, sub, go, ge)), (go, ge)
        assert np.all(u <= u1)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("gaps", GAPS)
def test_pssm_with_an_all_negative_column(swg, orc, gaps, k):
    rng = np.random.default_rng(11 - gaps[0])
    subp = np.zeros((32, 32), dtype=np.int8)
    subp[1:, 1:] = rng.integers(-9, 8, size=(31, 31))
    subp[1:, 5] = rng.integers(-9, 0, size=31)
    subp[1:, 9] = -128
    qp = rng.integers(1, 32, size=90).astype(np.int8)
    pssm = subp[qp.astype(np.int64)]
    flat, off = _random_db(rng, 50, 1, 150, np.arange(1, 32))
    t, u = swg.debug_prune_kmer(pssm, None, gaps[0], gaps[1], k, flat, off)
    scores = orc.score_db(qp, flat, off, subp, gaps[0], gaps[1])
    assert np.all(u.astype(np.int64) >= scores)
    _, u1 = swg.debug_prune_bound(pssm, None, flat, off)
    assert np.all(u <= u1)
    # residues 5 (E) and 9 (I) score below zero at every position: a block of them scores nothing
    cls = swg.KMER_CLASS
    assert t[_index([cls[5], cls[9]] * 2 + [cls[5]] * (k - 4))] == 0
    # the index query over the same table has the same table and bound
    t2, u2 = swg.debug_prune_kmer(subp, qp, gaps[0], gaps[1], k, flat, off)
    assert np.array_equal(t2, t) and np.array_equal(u2, u)


@pytest.mark.parametrize("k", KS)
def test_exact_copy_of_a_query_stretch_scores_the_bound(swg, orc, k):
    """Under BLOSUM62 a standard residue's best partner is itself: a copy of a stretch of the query scores exactly U_k,
    at every length around the block sizes -- a dropped block or row would show."""
    sub = _table(swg, "BLOSUM62")
    rng = np.random.default_rng(3)
    cls = np.array(swg.KMER_CLASS)
    letters = np.array([i for i in range(1, 27) if cls[i] < 21 and sub[i, i] > 0 and sub[i, i] == sub[1:27, i].max()])
    assert len(letters) == 20
    q = rng.choice(letters, size=200).astype(np.int8)
    cuts = [(0, 1), (10, 13), (20, 24), (30, 35), (40, 47), (50, 163), (0, 200), (199, 200), (17, 35), (60, 82)]
    assert [b - a for a, b in cuts][:6] == [1, 3, 4, 5, 7, 113]
    off = np.zeros(len(cuts) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([b - a for a, b in cuts])
    flat = np.concatenate([q[a:b] for a, b in cuts]).astype(np.int8)
    _, u = swg.debug_prune_kmer(sub, q, -2, -1, k, flat, off, table=False)
    scores = orc.score_db(q, flat, off, sub, -2, -1)
    assert np.array_equal(u.astype(np.int64), scores.astype(np.int64))
    assert [int(v) for v in u] == [int(sub[q[a:b].astype(np.int64), q[a:b].astype(np.int64)].sum()) for a, b in cuts]


def test_a_padded_sequence_is_the_shorter_one_of_a_pair(swg):
    """Residue 0 inside a sequence is a padding row: y filled up to x's length sums over x's blocks, and a sequence of
    padding rows alone adds nothing."""
    sub = _table(swg, "BLOSUM62")
    rng = np.random.default_rng(5)
    letters = np.arange(1, 26)
    q = rng.choice(letters, size=40).astype(np.int8)
    y = rng.choice(letters, size=17).astype(np.int8)
    cm, u1 = swg.debug_prune_bound(sub, q, y, np.array([0, 17], dtype=np.uint64))
    for k in KS:
        for lx in (17, 18, 19, 23, 38, 39, 57, 78, 79):
            flat = np.concatenate([y, np.zeros(lx - 17, dtype=np.int8), np.zeros(lx, dtype=np.int8)]).astype(np.int8)
            t, u = swg.debug_prune_kmer(sub, q, -2, -1, k, flat, np.array([0, lx, 2 * lx], dtype=np.uint64))
            assert u[1] == 0
            assert u[0] == _u_restated(swg, t, cm, flat[:lx], k), (k, lx)
            assert u[0] <= u1[0]


def test_choice_of_k(swg):
    ch = swg.debug_prune_kmer_choice
    # an unpruned search builds nothing, whatever is forced
    for forced in (0, 1, 4, 5):
        assert ch(forced=forced, pruned=0) == 0
    # forced values are honoured wherever the search is pruned, on any range
    for forced in (1, 4, 5):
        for rows in (1, 10 ** 4, 10 ** 10):
            assert ch(forced=forced, pruned=1, lq=100, pair_rows=rows) == forced
    # automatic, the library's own rates: the flagship (3000 columns against 1.9e9 pair rows) takes the larger table, a
    # database of a few thousand sequences none
    assert ch(lq=3000, pair_rows=1900000000) == 5
    assert ch(lq=200, pair_rows=300000) == 1
    assert ch(lq=3000, pair_rows=0) == 1
    # ... and steps down as lq grows against a small range at fixed rates: the tables' cells grow with lq, what the
    # range's rows can save does not
    rates = dict(table_rate=10 ** 12, fill_rate=10 ** 9, pair_rows=2 * 10 ** 8)
    got = [ch(lq=lq, **rates) for lq in (50, 100, 400, 1000, 3000, 100000)]
    assert got == sorted(got, reverse=True) and got[0] == 5 and got[-1] == 1 and 4 in got, got
    # more rows never choose a smaller k
    got = [ch(lq=1000, table_rate=10 ** 12, fill_rate=10 ** 9, pair_rows=r) for r in (10 ** 5, 10 ** 6, 10 ** 7, 10 ** 8, 10 ** 9)]
    assert got == sorted(got) and got[0] == 1 and got[-1] == 5, got


def test_argument_errors(swg):
    import ctypes as C_
    sub = _table(swg, "BLOSUM62")
    u = np.zeros(1, dtype=np.uint64)
    off = np.array([0, 1], dtype=np.uint64)
    one = np.array([1], dtype=np.int8)
    p = lambda a: a.ctypes.data_as(C_.c_void_p)  # noqa: E731
    f = swg.lib.swg_debug_prune_kmer
    assert f(None, p(one), 1, -2, -1, 4, p(one), p(off), 1, None, p(u)) == swg.SWG_ERR_ARG
    assert f(p(sub), p(one), 0, -2, -1, 4, p(one), p(off), 1, None, p(u)) == swg.SWG_ERR_ARG
    assert f(p(sub), p(one), 1, -2, -1, 3, p(one), p(off), 1, None, p(u)) == swg.SWG_ERR_ARG
    assert f(p(sub), p(one), 1, 1, -1, 4, p(one), p(off), 1, None, p(u)) == swg.SWG_ERR_ARG
    assert f(p(sub), p(one), 1, -2, -1, 4, p(one), p(off), 1, None, None) == swg.SWG_ERR_ARG
    assert f(p(sub), p(one), 1, -2, -1, 4, p(one), p(off), 1, None, p(u)) == swg.SWG_OK and u[0] == sub[1, 1]
