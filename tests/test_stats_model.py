"""CPU: the forward rule of swg_align_stats, restated in Python, against the int32 oracle's traceback.

The stats kernel (csrc/swg_bounds.hip) is the bounds kernel with two counts more in every tag: the tag is
(q_origin, d_origin, steps, ident, opens).  `forward_stats` below is `forward_bounds` of test_bounds_model.py with the
two counts; like it, it is written the way the kernel computes, the three reductions taken at the SOURCE cell.
  * forming H(j, i) from the diagonal reduction: ident += (q_i == d_j)
  * diagonal reduction: the counts are copied; a start gives (0, 0)
  * vertical reduction (the next A): opens + 1 when the pick is H or B, unchanged when it is A; a start gives ident 0,
    opens 1 (the path then begins with a gap)
  * left reduction (the next B): the same with A and B exchanged
  * a border cell's vertical and left hand-overs carry opens = 1 whatever they pick (with a positive gap_extend a path
    may run in from the border: the pick is then the border's own A or B, and it is still an opening); its diagonal
    hand-over carries 0
The truth is the ops string of orc.pair_trace with the counts taken from it: n_gap_open = matches of I+|D+."""
import re

import numpy as np
import pytest

from conftest import load_golden

GAPS = [(-11, -1), (-2, -1), (0, -1), (0, 0), (-1, 0), (1, -3), (-3, 1), (2, 1), (0, 1)]   # test_bounds_model.py's


def _reduce(states, adds, here, own, border):
    """max-with-pick over one cell's (value, tag) states H, A, B plus `adds`.  own: the index of the direction's own
    state (None diagonal, 1 = A downwards, 2 = B to the right); continuing any other state opens a gap run."""
    gap = own is not None
    vals = [v + a for (v, _), a in zip(states, adds)]
    m = max(max(vals), 0)
    if m == 0:
        return 0, (here[0], here[1], 1, 0, 1 if gap else 0)
    for n, (v, (_, t)) in enumerate(zip(vals, states)):
        if v == m:
            opens = t[4] + (1 if gap and n != own else 0)
            if border:
                opens = 1 if gap else 0
            return m, (t[0], t[1], t[2] + 1, t[3], opens)


def forward_stats(q, d, sub, gap_open, gap_extend):
    """-> (score, (q_begin, q_end, d_begin, d_end), n_ops, n_ident, n_gap_open) by the forward rule alone."""
    sub = np.asarray(sub).reshape(32, 32)
    lq, ld = len(q), len(d)
    go, ge = gap_open + gap_extend, gap_extend
    D, V, L = {}, {}, {}

    def hand_over(j, i, st, border=False):
        D[j, i] = _reduce(st, (0, 0, 0), (i, j), None, border)
        V[j, i] = _reduce(st, (go, ge, go), (i, j), 1, border)
        L[j, i] = _reduce(st, (go, go, ge), (i, j), 2, border)

    for i in range(lq + 1):
        hand_over(0, i, [(0, (i, 0, 0, 0, 0))] * 3, border=True)
    best, bj, bi, btag = 0, 0, 0, None
    for j in range(1, ld + 1):
        hand_over(j, 0, [(0, (0, j, 0, 0, 0))] * 3, border=True)
        for i in range(1, lq + 1):
            m, t = D[j - 1, i - 1]
            tag = (t[0], t[1], t[2], t[3] + int(q[i - 1] == d[j - 1]), t[4])
            h = (m + int(sub[int(q[i - 1]), int(d[j - 1])]), tag)
            hand_over(j, i, [h, V[j - 1, i], L[j, i - 1]])
            if h[0] > best:                      # rows, then columns, ascending: the first cell of the highest score
                best, bj, bi, btag = h[0], j, i, tag
    if best == 0:
        return 0, (0, 0, 0, 0), 0, 0, 0
    return best, (btag[0], bi, btag[1], bj), btag[2], btag[3], btag[4]


def counts_of(q, d, co, ops):
    """(n_ident, n_match, n_gap_open, n_gap) of a spelled path."""
    qi, di, ident = co[0], co[2], 0
    for o in ops:
        if o == "M":
            ident += int(q[qi] == d[di])
            qi, di = qi + 1, di + 1
        elif o == "I":
            di += 1
        else:
            qi += 1
    assert (qi, di) == (co[1], co[3])
    return ident, ops.count("M"), len(re.findall("I+|D+", ops)), len(ops) - ops.count("M")


def _same(orc, q, d, sub, go, ge):
    sc, co, ops = orc.pair_trace(q, d, sub, go, ge)
    ident, match, opens, gap = counts_of(q, d, co, ops)
    got = forward_stats(q, d, sub, go, ge)
    assert got == (sc, co, len(ops), ident, opens), (list(q), list(d), go, ge, ops)
    # the two counts the host derives (swg.h)
    assert match == (co[1] - co[0]) + (co[3] - co[2]) - len(ops) and gap == len(ops) - match
    return ops, ident, match, opens


@pytest.mark.parametrize("letters", [1, 2, 4, 20])
def test_stats_rule_equals_the_walk_on_random_pairs(orc, letters):
    rng = np.random.default_rng(0xB0D5 + letters)                    # the pairs of test_bounds_model.py
    sub = rng.integers(-4, 8, size=(32, 32)).astype(np.int8)
    seen = []
    for n in range(90):
        go, ge = GAPS[n % len(GAPS)]
        q = rng.integers(1, letters + 1, size=int(rng.integers(1, 18))).astype(np.int8)
        d = rng.integers(1, letters + 1, size=int(rng.integers(1, 18))).astype(np.int8)
        seen.append(_same(orc, q, d, sub, go, ge))
    if letters == 1:
        return                                                       # one letter: every column is identical
    # the set cannot go soft: a path that starts with a gap, one with two openings, one with a mismatch
    assert any(ops[:1] in ("I", "D") for ops, _, _, _ in seen)
    assert any(opens >= 2 for _, _, _, opens in seen)
    assert any(ident < match for _, ident, match, _ in seen)


@pytest.mark.parametrize("gaps", GAPS)
def test_stats_rule_on_ties(orc, gaps):
    """One letter, every score equal: every maximum is tied, so the H, A, B order and the best-cell rule decide."""
    sub = np.full((32, 32), 3, dtype=np.int8)
    for lq, ld in ((1, 1), (5, 5), (7, 3), (3, 7), (17, 16)):
        _same(orc, np.ones(lq, dtype=np.int8), np.ones(ld, dtype=np.int8), sub, *gaps)
    sub = np.full((32, 32), -1, dtype=np.int8)       # nothing scores: all zeros
    _same(orc, np.ones(4, dtype=np.int8), np.ones(6, dtype=np.int8), sub, *gaps)


@pytest.mark.parametrize("name", ["blosum62_tiny_db", "blosum62_gap_pos1_m3", "blosum62_gap_0_pos1"])
def test_stats_rule_on_golden_top_hits(orc, name):
    g = load_golden(name)
    go, ge = int(g["gaps"][0]), int(g["gaps"][1])
    off = g["offsets"].astype(np.int64)
    lens = np.diff(off)
    top = np.argsort(-g["oracle32"].astype(np.int64), kind="stable")
    top = [int(i) for i in top if lens[i] * len(g["query"]) <= 40000][:4]     # (the restatement is a Python double loop)
    assert top
    for i in top:
        _same(orc, g["query"], g["flat"][off[i]:off[i + 1]], g["sub"], go, ge)


def test_stats_rule_alternating_gaps(orc):
    """The widest count the kernel's tag must hold, in small: a column costs 20, a gap step pays 3 and a longer run pays
    less per step (1), so the path alternates I and D up to the one M it must end in -- every gap step is an opening."""
    sub = np.full((32, 32), -20, dtype=np.int8)
    q = d = np.ones(12, dtype=np.int8)
    ops, ident, match, opens = _same(orc, q, d, sub, 2, 1)
    assert opens == len(ops) - match and opens >= 2 and "II" not in ops and "DD" not in ops
