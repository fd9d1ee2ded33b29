"""CPU: the arithmetic of the packed int16 cells and of their wide form (seq-align-gpu_amd/csrc/swg_kernels.hip,
CellsDiag FORM 0 and 1), re-done in numpy int16 with explicit saturation -- the same operations in the same
order as the kernel's row(): v_pk_add_i16 clamp (M_diag + s), v_pk_sub_u16 clamp (plain form: floors at 0 for free) or
v_pk_sub_i16 clamp (wide form: values held as v - 32768, floor -32768 = score 0), v_pk_max_i16 -- against the int32
oracle, for gap magnitudes g, e from 0 to 32767.  What the kernels' correctness rests on, checked without a GPU: a pair
is flagged (best stuck at 32767, resp. 65535) exactly when the oracle's score is 32767 (65535) or more, and every
unflagged score is the oracle's.  Sibling of test_f16_cells_model.py; the sequences come from tests/scoring_edges.py, so
the large magnitudes are visible in the scores."""
import numpy as np
import pytest

import scoring_edges as se
from conftest import ROOT  # noqa: F401  (path set-up)

I16, U16, I32 = np.int16, np.uint16, np.int32


def add_i16_sat(a, b):
    return np.clip(a.astype(I32) + b.astype(I32), -32768, 32767).astype(I16)


def sub_i16_sat(a, b):
    return np.clip(a.astype(I32) - b.astype(I32), -32768, 32767).astype(I16)


def sub_u16_sat(a, b):
    """Unsigned saturating subtract on the same 16 bits (the operands are bit patterns, as in the register)."""
    d = np.clip(a.view(U16).astype(I32) - b.view(U16).astype(I32), 0, 65535)
    return d.astype(U16).view(I16)


def i16_cells_best(q, d, sub, g, e, wide):
    """Best cell of one pair as CellsDiag<K, 0 / 1>::row computes it, cell by cell in anti-diagonal order (the cells of
    an anti-diagonal do not depend on each other).  Returns the register's int16 value: the score itself (plain), the
    score - 32768 (wide)."""
    lq, ld = len(q), len(d)
    zero = I16(-32768) if wide else I16(0)
    sat_sub = sub_i16_sat if wide else sub_u16_sat
    go = np.array([g], dtype=U16).view(I16)       # magnitudes up to 32767: the same bits either way
    ge = np.array([e], dtype=U16).view(I16)
    S = np.asarray(sub)[np.asarray(q, dtype=np.int64)][:, np.asarray(d, dtype=np.int64)].astype(I16)   # [lq, ld]
    g0 = sat_sub(np.array([zero]), go)[0]         # column 0: M = score 0, so G = max(0 - g, 0)
    new = lambda: np.full(lq + 1, zero, dtype=I16)
    M2, M1, G1, A1, B1 = new(), new(), new(), new(), new()
    G1[0] = g0
    best = zero
    i = np.arange(1, lq + 1)
    for k in range(1, lq + ld):
        r = k - i
        valid = (r >= 0) & (r < ld)
        s = np.where(valid, S[i - 1, np.clip(r, 0, ld - 1)], I16(0)).astype(I16)
        t = add_i16_sat(M2[i - 1], s)                                   # M_diag + s, sticks at 32767
        a = np.maximum(G1[i], sat_sub(A1[i], ge))
        b = np.maximum(G1[i - 1], sat_sub(B1[i - 1], ge))
        m = np.maximum(np.maximum(t, a), b)
        G = sat_sub(m, go)
        M, A, B, Gn = new(), new(), new(), new()
        Gn[0] = g0
        M[1:] = np.where(valid, m, zero)                                # (rows before the first: the reset state)
        A[1:] = np.where(valid, a, zero)
        B[1:] = np.where(valid, b, zero)
        Gn[1:] = np.where(valid, G, zero)
        if valid.any():
            best = max(best, m[valid].max())
        M2, M1, G1, A1, B1 = M1, M, Gn, A, B
    return int(best)


def _check_pairs(orc, q, seqs, sub, go, ge):
    g, e = -(go + ge), -ge
    assert 0 <= e <= g <= 32767
    tally = {"plain_exact": 0, "plain_flagged": 0, "wide_exact": 0, "wide_flagged": 0, "gapped": 0}
    for d in seqs:
        truth, _, ops = orc.pair_trace(q, d, sub, go, ge)
        tally["gapped"] += "I" in ops or "D" in ops
        plain = i16_cells_best(q, d, sub, g, e, wide=False)
        assert (plain == 32767) == (truth >= 32767), (go, ge, len(d), truth, plain)
        if plain != 32767:
            assert plain == truth, (go, ge, len(d), truth, plain)
        tally["plain_flagged" if plain == 32767 else "plain_exact"] += 1
        wide = i16_cells_best(q, d, sub, g, e, wide=True) + 32768
        assert (wide == 65535) == (truth >= 65535), (go, ge, len(d), truth, wide)
        if wide != 65535:
            assert wide == truth, (go, ge, len(d), truth, wide)
        tally["wide_flagged" if wide == 65535 else "wide_exact"] += 1
    return tally


GAPS = [(-2, -1), (0, 0), (-3, 0), (-2047, -1), (0, -2049), (-15999, -1), (0, -16000), (-16383, -16384),
        (-32766, -1), (0, -32767), (-32767, 0)]


@pytest.mark.parametrize("gaps", GAPS, ids=["go%d_ge%d" % x for x in GAPS])
def test_i16_cells_are_exact_below_their_ceilings_and_flag_everything_else(orc, gaps):
    """Relatives with indels between two flanks that each score more than g (so the gap shows), at this magnitude's
    own flank length and at flanks of 262 (copies score 66548, gapped relatives 66548 - g: for small g beyond both
    ceilings, for g = 32767 between them)."""
    go, ge = gaps
    g = -(go + ge)
    sub = se.diag127()
    total = {}
    for F in sorted({se.flank_len(g), 262}):
        rng = np.random.default_rng([g, -ge, F])
        q = rng.integers(1, 32, size=2 * F).astype(np.int8)
        _, flat, off, kinds = se.split_db(g, 13, rng, query=q)
        seqs = se.seqs_of(flat, off)
        # (one of each kind, a short decoy, and a single insertion and a single deletion, which pay at any e)
        seqs = seqs[:6] + [seqs[10], np.concatenate([q[:F], q[:1], q[F:]]), np.concatenate([q[:F - 1], q[F:]])]
        for k_, v in _check_pairs(orc, q, seqs, sub, go, ge).items():
            total[k_] = total.get(k_, 0) + v
    assert total["plain_exact"] >= 2 and total["plain_flagged"] >= 2 and total["wide_exact"] >= 4, total
    assert total["wide_flagged"] >= 1 and total["gapped"] >= 2, total


@pytest.mark.parametrize("gaps", [(-2, -1), (-2048, -1), (0, -32767)], ids=["go-2_ge-1", "go-2048_ge-1", "go0_ge-32767"])
def test_i16_ceilings_to_the_unit(orc, gaps):
    """Prefixes of one query that score 32766, 32767, 65533 and 65535 exactly: the plain cells flag from 32767 on
    (32767 itself included -- a stuck value and a true one cannot be told apart), the wide form from 65535 on."""
    go, ge = gaps
    rng = np.random.default_rng(5)
    sub = se.diag127()
    sub[31, 31], sub[30, 30] = 1, 2
    r = lambda n: rng.integers(1, 30, size=n).astype(np.int8)
    q = np.concatenate([r(258), [31], r(258), [30], r(6)]).astype(np.int8)
    cuts = {258: 32766, 259: 32767, 517: 65533, 518: 65535, 524: 65535 + 6 * 127}
    seqs = [q[:n].copy() for n in cuts]
    for d, want in zip(seqs, cuts.values()):
        assert orc.pair(q, d, sub, go, ge) == want
    tally = _check_pairs(orc, q, seqs, sub, go, ge)
    assert (tally["plain_exact"], tally["plain_flagged"], tally["wide_exact"], tally["wide_flagged"]) == (1, 4, 3, 2)


def test_saturating_operations_are_what_the_instructions_do():
    """The three clamped operations on the values the cells meet: the unsigned subtract floors at 0 with a subtrahend up
    to 32767 (and clears anything with the reset rows' all-ones operand), the signed one floors at -32768 on values
    biased by -32768, the add sticks at both ends."""
    a = np.array([0, 1, 127, 32766, 32767], dtype=I16)
    big = np.array([32767], dtype=I16)
    assert sub_u16_sat(a, big).tolist() == [0, 0, 0, 0, 0] and sub_u16_sat(a, np.array([126], dtype=I16)).tolist() == [0, 0, 1, 32640, 32641]
    assert sub_u16_sat(a, np.array([-1], dtype=I16)).tolist() == [0] * 5                 # 0xFFFF: the reset rows' gap operand
    w = np.array([-32768, -32767, 0, 32767], dtype=I16)
    assert sub_i16_sat(w, big).tolist() == [-32768, -32768, -32767, 0]
    assert add_i16_sat(w, np.array([127], dtype=I16)).tolist() == [-32641, -32640, 127, 32767]
    assert add_i16_sat(w, np.array([-128], dtype=I16)).tolist() == [-32768, -32768, -128, 32639]
