"""CPU: the mirror of a fifth level of the pruning bound (swg_debug_prune_kmer_refine5) -- the fourth
level's blocks of 5 in 256 segments, with the query columns jumped over between two blocks charged as a gap.  Against the
int32 oracle from below (the bound must never fall under a score: gapped relatives of the query are the cases where a
wrong charge would put it there), against the fourth level's mirror from above, and against a numpy restatement of the
second table and of the walk in its exact form."""
import numpy as np
import pytest

from test_prune_deep_host import _blocks5, numpy_table5

C = 22
S = 256
NONE = -(1 << 28)


def _sub(swg, name):
    return np.asarray(swg.load_scoring(name).table(), dtype=np.int8).reshape(32, 32)


def numpy_table5_spans(swg, rows, q, gaps, cls):
    """-> the second entries [n][S] of the class blocks cls [n][5]: the best of score + e x span over a block's chains whose
    last match lies in the segment, all blocks at once along the query"""
    lq = len(q) if q is not None else rows.shape[0]
    prof = (rows[q.astype(np.int64)] if q is not None else rows).astype(np.int64)
    klass = np.asarray(swg.KMER_CLASS, dtype=np.int64)
    cprof = np.full((lq, C), -128, dtype=np.int64)
    for r in range(1, 32):
        cprof[:, klass[r]] = np.maximum(cprof[:, klass[r]], prof[:, r])
    g, e = -(gaps[0] + gaps[1]), -gaps[1]
    W = -(-lq // S)
    n = len(cls)
    M = np.full((5, n), NONE, dtype=np.int64)   # a row's cell of the previous column: best chain ending there, in any state
    A = np.full((5, n), NONE, dtype=np.int64)   # ... in a gap along the query
    best = np.zeros(n, dtype=np.int64)
    table = np.zeros((n, S), dtype=np.int64)
    for i in range(lq):
        diag = np.full(n, NONE, dtype=np.int64)
        above = np.full(n, NONE, dtype=np.int64)
        B = np.full(n, NONE, dtype=np.int64)
        for j in range(5):
            a = np.maximum(np.maximum(M[j] - (g - e), A[j]), NONE)
            b = np.maximum(np.maximum(above - g, B - e), NONE)
            h = cprof[i, cls[:, j]] + np.maximum(0, diag + e)
            m = np.maximum(np.maximum(h, a), b)
            diag = M[j].copy()
            M[j], A[j], B, above = m, a, b, m
            best = np.maximum(best, h)
        if (i + 1) % W == 0 or i + 1 == lq:
            table[:, i // W] = best
            best = np.zeros(n, dtype=np.int64)
    return table


def numpy_bound5_exact(swg, rows, q, gaps, flat, off):
    """The exact form, restated: a block ending in segment s behind one that ended in s'' adds
    min(T, colmax sum, T2 - e W max(0, s - s'' - 1)); a block may be left out."""
    klass = np.asarray(swg.KMER_CLASS, dtype=np.int64)
    lq = len(q) if q is not None else rows.shape[0]
    o = off.astype(np.int64)
    seq_blocks = [_blocks5(flat[o[i]:o[i + 1]].astype(np.int64) & 31) for i in range(len(o) - 1)]
    allb = np.unique(np.concatenate(seq_blocks), axis=0)
    t, colmax = numpy_table5(swg, rows, q, gaps, S, klass[allb])
    t2 = numpy_table5_spans(swg, rows, q, gaps, klass[allb])
    key = {tuple(b): i for i, b in enumerate(allb.tolist())}
    c = -gaps[1] * -(-lq // S)
    s = np.arange(S)
    between = np.maximum(0, s[None, :] - s[:, None] - 1)          # [s''][s]
    reach = s[:, None] <= s[None, :]
    out = np.zeros(len(seq_blocks), dtype=np.int64)
    for i, blocks in enumerate(seq_blocks):
        H = np.zeros(S, dtype=np.int64)
        for b in blocks:
            k = key[tuple(b.tolist())]
            tm = np.minimum(t[k], colmax[b].sum())
            add = np.minimum(tm[None, :], t2[k][None, :] - c * between)
            H = np.maximum(H, np.where(reach, H[:, None] + add, NONE).max(axis=0))
        out[i] = H.max()
    return out


def _families(swg, q, rng):
    """-> (the sequences as the oracle scores them, as the mirrors walk them): unrelated ones, gapped relatives of the
    query, the short and the padded ones, and residues of class 21"""
    lq = len(q)
    W = -(-lq // S)
    cut = min(3 * W + 1, lq // 3)
    a = lq // 3
    klass = np.asarray(swg.KMER_CLASS)
    merged = np.nonzero(klass == C - 1)[0]
    merged = merged[merged > 0]
    ins = rng.integers(1, 21, size=40).astype(np.int8)
    deleted = np.concatenate([q[:a], q[a + cut:]])
    inserted = np.concatenate([q[:2 * lq // 3], ins, q[2 * lq // 3:]])
    both = np.concatenate([q[:a], q[a + cut:2 * lq // 3], ins, q[2 * lq // 3:]])
    real = [rng.integers(1, 21, size=int(n)).astype(np.int8) for n in (lq, lq // 2 + 3, 2 * lq)] + [
        deleted, inserted, both, q.copy(),
        q[:3].copy(),                                    # shorter than 5 rows
        q[5:5 + 13].copy(),                              # 2 + 13 rows: four token blocks, no block of 5
        np.concatenate([q[:20], rng.choice(merged, size=9).astype(np.int8), q[29:min(lq, 70)]]),
    ]
    walked = [r.copy() for r in real]
    # the shorter sequence of a pair of very different lengths, filled up to the longer one's
    real.append(q[10:40].copy())
    walked.append(np.concatenate([q[10:40], np.zeros(2 * lq - 30, dtype=np.int8)]))
    return real, walked


def _flat(parts):
    off = np.zeros(len(parts) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in parts])
    return np.concatenate(parts).astype(np.int8), off


@pytest.mark.parametrize("gaps", [(-2, -1), (-11, -1)])
@pytest.mark.parametrize("table", ["BLOSUM62", "PAM250"])
@pytest.mark.parametrize("lq", [61, 300, 3000])
def test_between_the_score_and_the_fourth_level(swg, orc, lq, table, gaps):
    rng = np.random.default_rng(0x5EED0E01 + lq)
    sub = _sub(swg, table)
    q = swg.synth_query(0x5EED0E02, lq)
    real, walked = _families(swg, q, rng)
    rflat, roff = _flat(real)
    flat, off = _flat(walked)
    scores = orc.score_db(q, rflat, roff, sub, gaps[0], gaps[1]).astype(np.int64)
    u4 = swg.debug_prune_kmer_refine4(sub, q, gaps[0], gaps[1], S, flat, off).astype(np.int64)
    assert swg.debug_prune_table_bits(sub, q, 5) == 8
    for N in (0, 1, 3, S):
        u5 = swg.debug_prune_kmer_refine5(sub, q, gaps[0], gaps[1], S, flat, off, explicit=N)
        assert u5 is not None
        u5 = u5.astype(np.int64)
        assert np.all(u5 >= scores), (lq, table, gaps, N, (u5 - scores).tolist())
        assert np.all(u5 <= u4), (lq, table, gaps, N)
        if N == S:
            exact = u5
    for N in (0, 1, 3):     # a relaxed form is never below the exact one
        assert np.all(swg.debug_prune_kmer_refine5(sub, q, gaps[0], gaps[1], S, flat, off, explicit=N).astype(np.int64) >= exact)
    # the relatives score high: the charge is real there, and the bound still holds
    assert scores[3] > 2 * lq and scores[4] > 2 * lq and scores[5] > 2 * lq


@pytest.mark.parametrize("lq, table, gaps", [(61, "BLOSUM62", (-2, -1)), (300, "PAM250", (-11, -1)), (300, "BLOSUM62", (-3, -2))])
def test_the_exact_form_against_numpy(swg, lq, table, gaps):
    rng = np.random.default_rng(0x5EED0E03)
    sub = _sub(swg, table)
    q = swg.synth_query(0x5EED0E02, lq)
    _, walked = _families(swg, q, rng)
    keep = [w for w in walked if len(w) <= 2 * lq][:9] + [walked[-1][:lq]]
    flat, off = _flat(keep)
    u5 = swg.debug_prune_kmer_refine5(sub, q, gaps[0], gaps[1], S, flat, off, explicit=S).astype(np.int64)
    assert np.array_equal(u5, numpy_bound5_exact(swg, sub, q, gaps, flat, off))
    # one sequence at a time (no block shares a prefix with another sequence's): the same bounds
    for i in (0, 3, len(keep) - 1):
        one = np.array([0, off[i + 1] - off[i]], dtype=np.uint64)
        ui = swg.debug_prune_kmer_refine5(sub, q, gaps[0], gaps[1], S, flat[int(off[i]):int(off[i + 1])], one, explicit=S)
        assert int(ui[0]) == u5[i], i


def test_the_explicit_segments_reach_the_exact_form(swg):
    """Beyond the n at which e W n exceeds every second entry the cap no longer binds: N that large is the exact form."""
    sub = _sub(swg, "BLOSUM62")
    q = swg.synth_query(0x5EED0E02, 3000)
    rng = np.random.default_rng(0x5EED0E04)
    _, walked = _families(swg, q, rng)
    flat, off = _flat(walked)
    N = -(-5 * (int(sub.max()) + 1) // 12)      # W = 12, e = 1: no second entry is above 12 N
    exact = swg.debug_prune_kmer_refine5(sub, q, -2, -1, S, flat, off, explicit=S)
    assert np.array_equal(swg.debug_prune_kmer_refine5(sub, q, -2, -1, S, flat, off, explicit=N), exact)
    # the device's N: never below the exact form
    assert swg.REFINE5_EXPLICIT < N and np.all(swg.debug_prune_kmer_refine5(sub, q, -2, -1, S, flat, off) >= exact)


def test_where_the_level_is_off(swg):
    sub = _sub(swg, "BLOSUM62")
    q = swg.synth_query(0x5EED0E02, 90)
    flat, off = _flat([q[:50].copy(), q[20:33].copy()])
    # a gap whose further residues are free: the fourth level, so no fifth
    assert swg.debug_prune_kmer_refine5(sub, q, -3, 0, S, flat, off) is None
    assert swg.debug_prune_kmer_refine5(sub, q, -3, -1, S, flat, off) is not None
    # a PSSM with an entry of 52: the k = 5 tables need 16 bits; the fourth level's mirror is what it was
    pssm = sub[q.astype(np.int64)].copy()
    pssm[40, 12] = 52
    assert swg.debug_prune_table_bits(pssm, None, 5) == 16
    assert swg.debug_prune_kmer_refine5(pssm, None, -11, -1, S, flat, off) is None
    t, colmax = numpy_table5(swg, pssm, None, (-11, -1), S, np.asarray(swg.KMER_CLASS, dtype=np.int64)[_blocks5(q[:50].astype(np.int64))])
    H = np.zeros(S, dtype=np.int64)
    for b, e in zip(_blocks5(q[:50].astype(np.int64)), t):
        H = np.maximum.accumulate(H) + np.minimum(e, colmax[b].sum())
    assert int(swg.debug_prune_kmer_refine4(pssm, None, -11, -1, S, flat, off)[0]) == H.max()
    # ... and one whose second entries alone are no bytes: 5 x 51 fits, 5 x (51 + 1) does not
    pssm[40, 12] = 51
    assert swg.debug_prune_table_bits(pssm, None, 5) == 8
    assert swg.debug_prune_kmer_refine5(pssm, None, -11, -1, S, flat, off) is None
    # other segment counts are no option
    u = np.zeros(2, dtype=np.uint64)
    on = np.zeros(1, dtype=np.int32)
    p = lambda a: a.ctypes.data  # noqa: E731
    for bad in (0, 128, 255, 512):
        assert swg.lib.swg_debug_prune_kmer_refine5(p(sub), p(q), 90, -2, -1, bad, 0, p(flat), p(off), 2, p(u), p(on)) == swg.SWG_ERR_ARG


HEADLINE_ROWS = 1938193684


def test_choice_of_the_fifth_level(swg):
    ch = swg.debug_prune_refine5_choice
    F = swg.PRUNE_REFINE5_FORCED
    # the levels in front of it are what debug_prune_refine4_choice says, whatever the fifth
    for kw in (dict(), dict(forced=4), dict(segments=32), dict(refine=64), dict(refine3=1), dict(refine4=1), dict(refine4=5256),
               dict(lq=200, pair_rows=300000), dict(table_bits=16), dict(table_bits5=16)):
        for r5 in (0, 1, F):
            for ok in (True, False):
                assert ch(refine5=r5, admitted=ok, **kw)[:5] == swg.debug_prune_refine4_choice(**kw), (kw, r5, ok)
    # automatic: more rows never lose it, the rule is the other levels'; every test-sized database is far below it
    got = [ch(lq=3000, pair_rows=r)[5] for r in (10 ** 4, 10 ** 6, 10 ** 7, 10 ** 8, 10 ** 9, HEADLINE_ROWS, 10 ** 10, 10 ** 11)]
    assert got == sorted(got) and got[:3] == [0, 0, 0] and got[-1] == 256, got
    for lq in (50, 200, 367, 1000, 3000):
        for rows in (5000, 300000, 3000000):
            assert ch(lq=lq, pair_rows=rows)[5] == 0, (lq, rows)
    # only behind a fourth level that was itself chosen automatically: every forced earlier level stays without it
    for kw in (dict(forced=4), dict(forced=4, segments=32), dict(segments=32), dict(forced=1), dict(refine=128), dict(refine=1), dict(refine3=256),
               dict(refine3=1), dict(refine4=5256), dict(refine4=1)):
        assert ch(lq=3000, pair_rows=10 ** 11, **kw)[5] == 0, kw
        assert ch(lq=3000, pair_rows=10 ** 11, refine5=F, **kw)[5] == 256, kw
        assert ch(lq=3000, pair_rows=10 ** 11, refine5=1, **kw)[5] == 0, kw
    # a caller's threshold: forced or off
    assert ch(lq=3000, pair_rows=10 ** 11, fixed=True)[4:] == (256, 0) and ch(lq=3000, pair_rows=10 ** 11, fixed=True, refine5=F)[5] == 256
    # e = 0, or entries that are no bytes: off whoever asks
    assert ch(lq=3000, pair_rows=10 ** 11, admitted=False)[4:] == (256, 0)
    assert ch(lq=3000, pair_rows=10 ** 11, admitted=False, refine5=F)[5] == 0
    assert ch(lq=3000, pair_rows=10 ** 11, table_bits5=16, refine5=F)[4:] == (0, 0)
    # forced on a small range; an unpruned search builds nothing; values that are no option
    assert ch(lq=200, pair_rows=5000, refine5=F) == (1, 1, 0, 0, 0, 256)
    assert ch(pruned=0, refine5=F) == (0, 0, 0, 0, 0, 0)
    for bad in ([0, 1, 3000, 10 ** 9, 0, 0, 0, 0, 0, 8, 0, 8, 256, 1, 0], [0, 1, 3000, 10 ** 9, 0, 0, 0, 0, 0, 8, 0, 8, 0, 2, 0],
                [0, 1, 3000, 10 ** 9, 0, 0, 0, 0, 0, 8, 0, 8, 0, 1, 2]):
        a = np.array(bad, dtype=np.int64)
        out = np.zeros(6, dtype=np.int64)
        assert swg.lib.swg_debug_prune_refine5_choice(a.ctypes.data, out.ctypes.data) == swg.SWG_ERR_ARG, bad


def test_the_stages_queue_the_fifth_level_behind_the_fourth(swg):
    segs = [(0, 10), (10, 25), (25, 31)]
    fourth = swg.debug_prune_stages(segs, refine=128, refine3=256, refine4=256)
    fifth = swg.debug_prune_stages(segs, refine=128, refine3=256, refine4=256, refine5=256)
    assert [s[:3] for s in fifth] == [s[:3] for s in fourth] and fifth[0][3] == ()
    assert all(s[3] == ("threshold", "refine", "refine3", "refine4", "refine5", "list") for s in fifth[1:])
    fixed = swg.debug_prune_stages(segs, fixed=True, refine=128, refine3=256, refine4=256, refine5=256)
    assert fixed[0][3] == ("gate", "refine", "refine3", "refine4", "refine5", "list")
    assert all(s[3] == ("refine", "refine3", "refine4", "refine5", "list") for s in fixed[1:])
    gated = swg.debug_prune_stages(segs, refine=128, refine3=256, refine4=256, refine5=256, gate=True)
    assert gated[1][3] == ("threshold", "bound", "refine", "refine3", "refine4", "refine5", "list") and "bound" not in gated[2][3]
    # behind no fourth level's walk; never with the prefix cut
    assert swg.debug_prune_stages(segs, refine5=256)[1][3] == ("threshold", "refine5", "list")
    assert swg.debug_prune_stages(segs, refine=128, refine4=256, refine5=256, prefix_cut=True)[1][3] == ("threshold", "prefix_cut")
    # the hooks without the level are what they were
    assert swg.debug_prune_stages(segs, refine=128, refine3=256, refine4=256, gate=True)[1][3] == ("threshold", "bound", "refine", "refine3", "refine4", "list")
