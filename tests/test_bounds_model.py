"""CPU: the forward rule of swg_align_bounds, restated in Python, against the int32 oracle's traceback.

The bounds kernel (csrc/swg_bounds.hip) finds an alignment's coordinates and its number of steps without
a traceback: every state value carries a tag (q_origin, d_origin, steps), and the predecessor is chosen by the tie rule
the walk of swg_trace_kernel applies (0 if the maximum is 0, else H, A, B in that order).  `forward_bounds` below is
the specification the kernel is written from; it is written the way the kernel computes, with the three reductions
(diagonal, vertical, left) taken at the SOURCE cell, so that a cell's H, A and B are what its neighbours handed over."""
import numpy as np
import pytest

from conftest import load_golden

GAPS = [(-11, -1), (-2, -1), (0, -1), (0, 0), (-1, 0), (1, -3), (-3, 1), (2, 1), (0, 1)]


def _reduce(states, adds, here):
    """max-with-pick over one cell's (value, tag) states H, A, B plus `adds`: the value and tag a neighbour starts from.
    A zero maximum starts the alignment at the source cell `here`; either way the step into the neighbour is counted."""
    vals = [v + a for (v, _), a in zip(states, adds)]
    m = max(max(vals), 0)
    if m == 0:
        return 0, (here[0], here[1], 1)
    for v, (_, t) in zip(vals, states):
        if v == m:
            return m, (t[0], t[1], t[2] + 1)


def forward_bounds(q, d, sub, gap_open, gap_extend):
    """-> (score, (q_begin, q_end, d_begin, d_end), n_ops) by the forward rule alone."""
    sub = np.asarray(sub).reshape(32, 32)
    lq, ld = len(q), len(d)
    go, ge = gap_open + gap_extend, gap_extend
    # per cell (j, i), j = database row, i = query column, both from 0 = border: the three reductions of its states
    D, V, L = {}, {}, {}

    def border(j, i):
        st = [(0, (i, j, 0))] * 3
        return st

    def hand_over(j, i, st):
        D[j, i] = _reduce(st, (0, 0, 0), (i, j))
        V[j, i] = _reduce(st, (go, ge, go), (i, j))
        L[j, i] = _reduce(st, (go, go, ge), (i, j))

    for i in range(lq + 1):
        hand_over(0, i, border(0, i))
    best, bj, bi, btag = 0, 0, 0, None
    for j in range(1, ld + 1):
        hand_over(j, 0, border(j, 0))
        for i in range(1, lq + 1):
            m, tag = D[j - 1, i - 1]
            h = (m + int(sub[int(q[i - 1]), int(d[j - 1])]), tag)
            st = [h, V[j - 1, i], L[j, i - 1]]
            hand_over(j, i, st)
            if h[0] > best:                      # rows, then columns, ascending: the first cell of the highest score
                best, bj, bi, btag = h[0], j, i, tag
    if best == 0:
        return 0, (0, 0, 0, 0), 0
    return best, (btag[0], bi, btag[1], bj), btag[2]


def _same(orc, q, d, sub, go, ge):
    sc, co, ops = orc.pair_trace(q, d, sub, go, ge)
    assert forward_bounds(q, d, sub, go, ge) == (sc, co, len(ops)), (list(q), list(d), go, ge)


@pytest.mark.parametrize("letters", [1, 2, 4, 20])
def test_forward_rule_equals_the_walk_on_random_pairs(orc, letters):
    rng = np.random.default_rng(0xB0D5 + letters)
    sub = rng.integers(-4, 8, size=(32, 32)).astype(np.int8)
    for n in range(90):
        go, ge = GAPS[n % len(GAPS)]
        q = rng.integers(1, letters + 1, size=int(rng.integers(1, 18))).astype(np.int8)
        d = rng.integers(1, letters + 1, size=int(rng.integers(1, 18))).astype(np.int8)
        _same(orc, q, d, sub, go, ge)


@pytest.mark.parametrize("gaps", GAPS)
def test_forward_rule_on_ties(orc, gaps):
    """One letter, every score equal: every maximum is tied, so the H, A, B order and the best-cell rule decide."""
    sub = np.full((32, 32), 3, dtype=np.int8)
    for lq, ld in ((1, 1), (5, 5), (7, 3), (3, 7), (17, 16)):
        _same(orc, np.ones(lq, dtype=np.int8), np.ones(ld, dtype=np.int8), sub, *gaps)
    sub = np.full((32, 32), -1, dtype=np.int8)       # nothing scores: all zeros
    _same(orc, np.ones(4, dtype=np.int8), np.ones(6, dtype=np.int8), sub, *gaps)


@pytest.mark.parametrize("name", ["blosum62_tiny_db", "blosum62_gap_pos1_m3", "blosum62_gap_0_pos1"])
def test_forward_rule_on_golden_top_hits(orc, name):
    g = load_golden(name)
    go, ge = int(g["gaps"][0]), int(g["gaps"][1])
    off = g["offsets"].astype(np.int64)
    lens = np.diff(off)
    top = np.argsort(-g["oracle32"].astype(np.int64), kind="stable")
    top = [int(i) for i in top if lens[i] * len(g["query"]) <= 40000][:4]     # (the restatement is a Python double loop)
    assert top
    for i in top:
        _same(orc, g["query"], g["flat"][off[i]:off[i + 1]], g["sub"], go, ge)
