"""CPU: the score bound a pruned search cuts by, through its host mirror (swg_debug_prune_bound).

colmax[r] = max(0, best score of database residue r against any query column) and U(d) = sum of colmax over d's
residues.  With non-positive gap scores U >= the local alignment score, whatever the table: every case below checks that
against the oracle, pair by pair.  An exact copy of a stretch of the query under BLOSUM62 (every residue's best partner is
itself) scores exactly U, which catches a residue dropped from the sum."""
import numpy as np
import pytest

GAPS = [(-2, -1), (0, 0), (-11, -1)]


def _table(swg, name):
    return np.asarray(swg.load_scoring(name).table(), dtype=np.int8).reshape(32, 32)


def _random_db(rng, n, lo, hi, residues):
    lens = rng.integers(lo, hi + 1, size=n)
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens)
    flat = rng.choice(residues, size=int(off[-1])).astype(np.int8)
    return flat, off


def _colmax_numpy(rows, query):
    rows = np.asarray(rows, dtype=np.int64)
    cols = rows[np.unique(np.asarray(query, dtype=np.int64))] if query is not None else rows
    cm = np.maximum(cols.max(axis=0), 0)
    cm[0] = 0
    return cm


def _u_numpy(cm, flat, off):
    return np.array([int(cm[flat[int(off[i]):int(off[i + 1])].astype(np.int64)].sum()) for i in range(len(off) - 1)], dtype=np.int64)


@pytest.mark.parametrize("gaps", GAPS)
@pytest.mark.parametrize("matrix", ["BLOSUM62", "PAM250"])
def test_bound_covers_the_oracle_score(swg, orc, matrix, gaps):
    sub = _table(swg, matrix)
    rng = np.random.default_rng(len(matrix) * 100 - gaps[0])
    letters = np.array([i for i in range(1, 27)] + [31])
    q = rng.choice(letters, size=75).astype(np.int8)
    flat, off = _random_db(rng, 60, 1, 140, letters)
    cm, u = swg.debug_prune_bound(sub, q, flat, off)
    want_cm = _colmax_numpy(sub, q)
    assert np.array_equal(cm.astype(np.int64), want_cm)
    assert np.array_equal(u.astype(np.int64), _u_numpy(want_cm, flat, off))
    scores = orc.score_db(q, flat, off, sub, gaps[0], gaps[1])
    assert np.all(u.astype(np.int64) >= scores), (matrix, gaps, int((scores - u.astype(np.int64)).max()))
    assert scores.max() > 0


def test_residues_outside_the_table(swg, orc):
    """Indices 27..30 have no letter: the table's rows and columns for them are whatever the caller put there (here
    random, some positive), and database and query may both hold them."""
    rng = np.random.default_rng(7)
    sub = _table(swg, "BLOSUM62").copy()
    sub[27:31, 1:] = rng.integers(-6, 7, size=(4, 31))
    sub[1:, 27:31] = rng.integers(-6, 7, size=(31, 4))
    every = np.arange(1, 32)
    q = rng.choice(every, size=60).astype(np.int8)
    flat, off = _random_db(rng, 50, 1, 120, every)
    cm, u = swg.debug_prune_bound(sub, q, flat, off)
    assert np.array_equal(cm.astype(np.int64), _colmax_numpy(sub, q))
    for go, ge in GAPS:
        assert np.all(u.astype(np.int64) >= orc.score_db(q, flat, off, sub, go, ge))


@pytest.mark.parametrize("gaps", GAPS)
def test_pssm_with_an_all_negative_column(swg, orc, gaps):
    """A PSSM of at most 31 distinct positions is an index query over its own table (q'[i] = the id of position i's row),
    which is what the oracle takes.  Residues 5 and 9 score below zero at every position: their entries are 0, not the
    (negative) best."""
    rng = np.random.default_rng(11 - gaps[0])
    subp = np.zeros((32, 32), dtype=np.int8)
    subp[1:, 1:] = rng.integers(-9, 8, size=(31, 31))
    subp[1:, 5] = rng.integers(-9, 0, size=31)
    subp[1:, 9] = -128
    qp = rng.integers(1, 32, size=90).astype(np.int8)
    pssm = subp[qp.astype(np.int64)]
    flat, off = _random_db(rng, 50, 1, 150, np.arange(1, 32))
    cm, u = swg.debug_prune_bound(pssm, None, flat, off)
    assert cm[5] == 0 and cm[9] == 0 and cm[0] == 0
    assert np.array_equal(cm.astype(np.int64), _colmax_numpy(pssm, None))
    scores = orc.score_db(qp, flat, off, subp, gaps[0], gaps[1])
    assert np.all(u.astype(np.int64) >= scores)
    # the index query over the same table has the same bound when it uses the same rows
    cm2, u2 = swg.debug_prune_bound(subp, qp, flat, off)
    assert np.array_equal(cm2, cm) and np.array_equal(u2, u)


def test_exact_copy_of_a_query_stretch_scores_the_bound(swg, orc):
    sub = _table(swg, "BLOSUM62")
    rng = np.random.default_rng(3)
    letters = np.array([i for i in range(1, 27) if sub[i, i] > 0 and sub[i, i] == sub[1:27, i].max()])   # (a residue's best partner is itself)
    q = rng.choice(letters, size=200).astype(np.int8)
    # (the bound's table ranges over the residues the QUERY holds: all of `letters` at this length)
    assert set(int(v) for v in q) == set(int(v) for v in letters)
    cuts = [(0, 200), (0, 1), (199, 200), (17, 130), (60, 61), (3, 7)]
    off = np.zeros(len(cuts) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([b - a for a, b in cuts])
    flat = np.concatenate([q[a:b] for a, b in cuts]).astype(np.int8)
    _, u = swg.debug_prune_bound(sub, q, flat, off)
    scores = orc.score_db(q, flat, off, sub, -2, -1)
    assert np.array_equal(u.astype(np.int64), scores.astype(np.int64))
    assert [int(v) for v in u] == [int(sub[q[a:b].astype(np.int64), q[a:b].astype(np.int64)].sum()) for a, b in cuts]


def test_argument_errors(swg):
    import ctypes as C
    sub = _table(swg, "BLOSUM62")
    u = np.zeros(1, dtype=np.uint64)
    off = np.array([0, 1], dtype=np.uint64)
    one = np.array([1], dtype=np.int8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert swg.lib.swg_debug_prune_bound(None, p(one), 1, p(one), p(off), 1, None, p(u)) == swg.SWG_ERR_ARG
    assert swg.lib.swg_debug_prune_bound(p(sub), p(one), 0, p(one), p(off), 1, None, p(u)) == swg.SWG_ERR_ARG
    assert swg.lib.swg_debug_prune_bound(p(sub), p(one), 1, p(one), p(off), 1, None, None) == swg.SWG_ERR_ARG
