"""CPU: the arithmetic of the gapless cells (seq-align-gpu_amd/csrc/swg_kernels.hip, CellsGapless), re-done in numpy
float16 in the manner of test_f16_cells_model.py -- the same operations in the same order, one rounding each, as
v_pk_add_f16 and the maxima perform them -- against the oracle with the gaps priced out.  What the kernel's correctness
rests on, checked without a GPU: a pair whose computed best stays below +2048.0 (score 4096) has the oracle's score
exactly; a pair is flagged exactly when its true score is 4096 or more, however far beyond (to +inf); and one row of the
padding residue's profile value, -65504, floors every M the wipe does not take care of, raises no best and makes no NaN."""
import numpy as np
import pytest

import gapless_cases as gc
import scoring_edges as se
from conftest import ROOT  # noqa: F401  (path set-up)

F = np.float16
FLOOR = F(-2048.0)
PAD = F(-65504.0)


def gapless_row(M, s):
    """One database row: M[i] <- max(M[i-1] + s[i], floor), column 0 (left of the query) held at the floor."""
    with np.errstate(over="ignore"):
        t = (M[:-1] + s).astype(F)
    Mn = np.empty_like(M)
    Mn[0] = FLOOR
    Mn[1:] = np.maximum(t, FLOOR)
    return Mn


def gapless_cells_best(q, d, sub):
    M = np.full(len(q) + 1, FLOOR, dtype=F)
    best = FLOOR
    for r in range(len(d)):
        M = gapless_row(M, sub[q, d[r]].astype(F))
        best = max(best, M.max())
    return best


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_gapless_cells_are_exact_below_their_ceiling_and_flag_everything_else(seed):
    import swg_loader
    orc = swg_loader.oracle()
    rng = np.random.default_rng(seed)
    n_flagged = n_exact = n_upper = n_inf = 0
    for case in range(30):
        kind = case % 3
        if kind == 0:                         # every entry anywhere in int8, rows and columns 0 included
            sub = se.full_range(rng)
        elif kind == 1:                       # a diagonal that decides how fast scores grow, the rest negative
            sub = rng.integers(-128, 4, size=(32, 32)).astype(np.int8)
            sub[np.arange(32), np.arange(32)] = int(rng.choice([6, 17, 60, 100, 127, 127]))
        else:
            sub = se.diag127(rng)
        far = case % 10 == 0                  # a whole copy of 600 residues at 127 each: 76 200, +inf in the making
        if far:
            sub = se.diag127(rng)
        lq = 600 if far else int(rng.integers(20, 110))
        q = rng.integers(1, 32, size=lq).astype(np.int8)
        a = 0 if far else int(rng.integers(0, lq // 2))
        b = lq if far else int(rng.integers(a + 1, lq + 1))
        d = np.concatenate([rng.integers(1, 32, size=int(rng.integers(0, 6))), q[a:b], rng.integers(1, 32, size=int(rng.integers(0, 6)))]).astype(np.int8)
        hit = rng.random(len(d)) < (0.0 if far else rng.choice([0.0, 0.0, 0.05, 0.3]))
        d[hit] = rng.integers(1, 32, size=int(hit.sum()))
        flat, off = gc.pack([d])
        truth = int(gc.oracle_gapless(orc, q, flat, off, sub)[0])
        best = gapless_cells_best(q.astype(np.int64), d.astype(np.int64), sub.astype(np.int32))
        assert not np.isnan(best), case
        flagged = bool(best >= F(2048.0))
        assert flagged == (truth >= 4096), (case, truth, float(best))
        if flagged:
            n_flagged += 1
            n_inf += bool(np.isinf(best))
        else:
            assert int(best) + 2048 == truth, (case, truth, float(best))
            n_exact += 1
            n_upper += truth > 2048
    assert n_flagged >= 5 and n_exact >= 8 and n_upper >= 1 and n_inf >= 1, (n_flagged, n_exact, n_upper, n_inf)


def test_one_padding_row_floors_every_state():
    """A reset row (and every row that pads the shorter sequence of a pair) reads the padding residue's profile row,
    -65504 in every column.  Whatever a pair left behind below 63456 = 65504 - 2048 -- the kernel wipes a lane whose best
    reached 32768 by hand -- is floored in ONE such row; the transient sum may be -inf, never NaN; and the row's values
    never exceed the floor, so a running best is not raised."""
    left = np.concatenate([np.arange(-2048, 2049, 7), [2048, 4096, 32767, 32768, 63455]]).astype(F)
    M = np.concatenate([[FLOOR], left]).astype(F)
    Mn = gapless_row(M, np.full(len(M) - 1, PAD, dtype=F))
    assert not np.isnan(Mn).any() and (Mn == FLOOR).all()
    with np.errstate(over="ignore"):
        assert F(FLOOR + PAD) == -np.inf and max(F(FLOOR + PAD), FLOOR) == FLOOR     # the transient of a clean state
        # what the explicit wipe is for: +inf survives the row (inf - 65504 = inf, still no NaN) and 65504 nearly does
        assert F(F(np.inf) + PAD) == np.inf and F(F(65504.0) + PAD) == F(0.0)
    # the kernel's test for "32768 or more" on the bit pattern: exponent field >= 30 (32752 is the float16 just below)
    for v, huge in ((32752.0, False), (32768.0, True), (65504.0, True), (np.inf, True), (-2048.0, False), (2048.0, False)):
        bits = int(np.array([v], dtype=F).view(np.uint16)[0])
        assert ((((bits & 0x7800) + 0x0800) & 0x8000) != 0) == huge, v


# ---- the lane group's stream: pairs back to back, reset rows, padding rows, the explicit wipe -----------------------
def _stream_scores(q, pairs, sub, G, K, f16_wipe):
    """The work-queue kernel's row loop for one lane group, restated: lane g holds columns [g K, (g + 1) K) of both
    sequences of a pair and works one row behind lane g - 1; a pair's token stream is two reset rows (padding residue,
    reset flag), one row per residue of the longer sequence X (Y padded with the padding residue), the last flagged
    LAST, then padding rows to a whole 4-row block; pairs follow each other without a gap.  State per lane: M[K] of both
    sequences, mdl (the diagonal into the strip's first column = the left lane's last M of the row before), best, and bc
    (the pair's best travelling along its last row).  Returns the biased f16 bests (X, Y) of every pair."""
    lq = len(q)
    prof = np.full((32, G * K), PAD, dtype=F)                  # [residue][column]; residue 0 and columns >= lq: padding
    prof[1:, :lq] = sub[q][:, 1:].T.astype(F)
    toks = []                                                  # (x residue, y residue, reset, last)
    for x, y in pairs:
        rows = [(0, 0, True, False), (0, 0, True, len(x) == 0)]    # (an empty pair ends on its second reset row)
        for r in range(len(x)):
            rows.append((int(x[r]), int(y[r]) if r < len(y) else 0, False, r == len(x) - 1))
        while len(rows) % 4:
            rows.append((0, 0, False, False))
        toks += rows
    toks += [(0, 0, False, False)] * (G + 12)                  # the drain: idle rows until the last row reaches the tail
    M = np.full((2, G, K), FLOOR, dtype=F)
    mdl = np.full((2, G), FLOOR, dtype=F)
    best = np.full((2, G), FLOOR, dtype=F)
    bc = np.full((2, G), FLOOR, dtype=F)
    m_out = np.full((2, G), FLOOR, dtype=F)
    out = []
    lanes = np.arange(G)
    with np.errstate(over="ignore", invalid="raise"):
        for t in range(len(toks) + G):
            row = t - lanes                                    # the row each lane is on
            live = (row >= 0) & (row < len(toks))
            tk = [toks[r] if ok else (0, 0, False, False) for r, ok in zip(row, live)]
            res = np.array([[a[0] for a in tk], [a[1] for a in tk]])
            reset = np.array([a[2] for a in tk])
            last = np.array([a[3] for a in tk])
            em = np.concatenate([np.full((2, 1), FLOOR, dtype=F), m_out[:, :-1]], axis=1)   # the left lane's edge of the step before
            cin = np.concatenate([np.full((2, 1), FLOOR, dtype=F), bc[:, :-1]], axis=1)
            if f16_wipe:
                huge = reset & ((best >= F(32768.0)).any(axis=0))          # either half: the test is on the packed word
                M[:, huge, :] = FLOOR
                mdl[:, huge] = FLOOR
                best[:, huge] = FLOOR
            best[:, reset] = FLOOR
            s = np.stack([prof[res[h]].reshape(G, G, K)[lanes, lanes] for h in range(2)])    # [2][lane][its K columns]
            prev = np.concatenate([mdl[:, :, None], M[:, :, :-1]], axis=2)
            M = np.maximum((prev + s).astype(F), FLOOR)
            assert not np.isnan(M).any()
            best = np.maximum(best, M.max(axis=2))
            mdl = em
            m_out = M[:, :, -1].copy()
            special = reset | last
            bc = np.where(special[None, :], np.maximum(cin, best), bc)
            if last[G - 1]:
                out.append((bc[0, G - 1], bc[1, G - 1]))
    return out


@pytest.mark.parametrize("G,K,lq", [(16, 6, 90), (16, 13, 200), (32, 2, 64), (32, 17, 540)])   # (540 x 127 = 68 580: +inf)
def test_lane_group_stream_leaks_nothing_from_pair_to_pair(G, K, lq):
    """Pairs of every kind back to back through one lane group: whole copies far beyond the ceiling (600 rows x 127:
    +inf in the making -- the explicit wipe's case), copies just above and just below the flag, random sequences, an
    empty Y, Y much shorter than X.  Every unflagged sequence has the oracle's score, whatever ran before it."""
    import swg_loader
    orc = swg_loader.oracle()
    rng = np.random.default_rng(G * 100 + K)
    sub = se.diag127(rng, zero0=True)
    q = rng.integers(1, 32, size=lq).astype(np.int8)
    rnd = lambda n: rng.integers(1, 32, size=n).astype(np.int8)
    long_copy = np.tile(q, 600 // lq + 1)[:600]                # 600 rows, every diagonal a run of copies: huge values
    pairs = [(long_copy, rnd(600)), (rnd(40), rnd(7)), (q[:33].copy(), q[:32].copy()), (rnd(35), np.zeros(0, dtype=np.int8)),
             (long_copy, long_copy[:500]), (q[5:37].copy(), rnd(30)), (rnd(50), rnd(50)), (q.copy(), rnd(3)), (rnd(9), rnd(9))]
    if lq >= 530:
        # a copy that ENDS on the pair's last row with +inf still in the strip (530 x 127; 2 + 530 rows are whole 4-row
        # blocks, so only the two reset rows follow): what a padding row cannot clear, before a short random pair
        pairs += [(q[:530].copy(), rnd(100)), (rnd(40), rnd(7)), (rnd(9), rnd(9))]
        leaked = _stream_scores(q.astype(np.int64), pairs[-3:], sub.astype(np.int32), G, K, f16_wipe=False)
        assert np.isinf(leaked[1][0]), "without the explicit wipe the +inf reaches the next pair: the case is live"
    got = _stream_scores(q.astype(np.int64), pairs, sub.astype(np.int32), G, K, f16_wipe=True)
    assert len(got) == len(pairs)
    n_flag = n_exact = 0
    for (x, y), bests in zip(pairs, got):
        for d, b in zip((x, y), bests):
            flat, off = gc.pack([d])
            truth = int(gc.oracle_gapless(orc, q, flat, off, sub)[0]) if len(d) else 0
            assert bool(b >= F(2048.0)) == (truth >= 4096), (len(d), truth, float(b))
            if truth < 4096:
                assert int(b) + 2048 == truth, (len(d), truth, float(b))
                n_exact += 1
            else:
                n_flag += 1
    assert n_flag >= 4 and n_exact >= 10, (n_flag, n_exact)
