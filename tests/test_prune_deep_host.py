"""CPU: the fourth level of the pruning bound -- blocks of 5 residues over 256 segments -- through the host
hooks: its mirror (swg_debug_prune_kmer_refine4), which holds no table, against a numpy restatement, the table-holding
mirror of k = 5 and the oracle; its choice (swg_debug_prune_refine4_choice) at its size edge, under every forced earlier
level and under both entry widths; and the stage list with its flag."""
import ctypes as C_

import numpy as np
import pytest

GO, GE = -2, -1
C = 22
HEADLINE_ROWS = 1938193684


def _sub(swg, name):
    return np.asarray(swg.load_scoring(name).table(), dtype=np.int8).reshape(32, 32)


def _blocks5(seq):
    """A sequence's token rows in the blocks the k = 5 bound takes: of 5 over every whole 20 rows, of 4 (a fifth, padding,
    row behind them) over the rest"""
    n_blocks = (2 + len(seq) + 3) // 4
    r = np.zeros(4 * n_blocks, dtype=np.int64)
    r[2:2 + len(seq)] = seq
    rows5 = 20 * (n_blocks // 5)
    out = [r[i:i + 5] for i in range(0, rows5, 5)]
    out += [np.concatenate([r[i:i + 4], [0]]) for i in range(rows5, len(r), 4)]
    return np.array(out, dtype=np.int64).reshape(-1, 5)


def numpy_table5(swg, rows, q, gaps, S, cls):
    """-> (the entries [n][S] of the class blocks cls [n][5] -- the recurrence of the table kernel, all blocks at once along
    the query --, colmax [32])"""
    lq = len(q) if q is not None else rows.shape[0]
    prof = (rows[q.astype(np.int64)] if q is not None else rows).astype(np.int64)
    klass = np.asarray(swg.KMER_CLASS, dtype=np.int64)
    cprof = np.full((lq, C), -128, dtype=np.int64)
    for r in range(1, 32):
        cprof[:, klass[r]] = np.maximum(cprof[:, klass[r]], prof[:, r])
    colmax = np.zeros(32, dtype=np.int64)
    colmax[1:] = np.maximum(prof[:, 1:].max(axis=0), 0)
    g, e = -(gaps[0] + gaps[1]), -gaps[1]
    W = -(-lq // S)
    n = len(cls)
    M = np.zeros((5, n), dtype=np.int64)
    A = np.zeros((5, n), dtype=np.int64)
    best = np.zeros(n, dtype=np.int64)
    table = np.zeros((n, S), dtype=np.int64)
    for i in range(lq):
        diag = np.zeros(n, dtype=np.int64)
        left = np.zeros(n, dtype=np.int64)
        B = np.zeros(n, dtype=np.int64)
        for j in range(5):
            s = cprof[i, cls[:, j]]
            a = np.maximum(np.maximum(M[j] - g, A[j] - e), 0)
            b = np.maximum(np.maximum(left - g, B - e), 0) if j else np.zeros(n, dtype=np.int64)
            m = np.maximum(np.maximum(diag + s, a), b)
            diag = M[j].copy()
            M[j], A[j], B, left = m, a, b, m
            best = np.maximum(best, m)
        if (i + 1) % W == 0 or i + 1 == lq:
            table[:, i // W] = best
            best = np.zeros(n, dtype=np.int64)
    return table, colmax


def _numpy_bound5(swg, rows, q, gaps, S, flat, off):
    """The ordered k = 5 bound over S segments, restated: the entries of the blocks that occur, then each sequence's walk."""
    klass = np.asarray(swg.KMER_CLASS, dtype=np.int64)
    o = off.astype(np.int64)
    seq_blocks = [_blocks5(flat[o[i]:o[i + 1]].astype(np.int64) & 31) for i in range(len(o) - 1)]
    allb = np.unique(np.concatenate(seq_blocks), axis=0)
    table, colmax = numpy_table5(swg, rows, q, gaps, S, klass[allb])
    key = {tuple(b): t for b, t in zip(allb.tolist(), table)}
    out = np.zeros(len(seq_blocks), dtype=np.int64)
    for i, blocks in enumerate(seq_blocks):
        H = np.zeros(S, dtype=np.int64)
        for b in blocks:
            H = np.maximum.accumulate(H) + np.minimum(key[tuple(b.tolist())], colmax[b].sum())
        out[i] = H.max()
    return out


@pytest.fixture(scope="module")
def seqs(swg):
    """Random sequences of 0..60 residues (token blocks 1..16: whole fives, tails of 1 to 4), every index 1..31 and padding
    rows (0) inside some, and three that copy a stretch of the query"""
    rng = np.random.default_rng(0x5EED0D01)
    q = swg.synth_query(0x5EED0D02, 777)
    parts = [rng.integers(1, 32, size=int(n)).astype(np.int8) for n in rng.integers(0, 61, size=117)]
    for p in parts[::7]:
        p[len(p) // 2:] = 0      # (the shorter sequence of a pair, filled up)
    parts += [q[100:160].copy(), q[767:777].copy(), q[0:7].copy()]
    off = np.zeros(len(parts) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in parts])
    return q, np.concatenate(parts).astype(np.int8), off


@pytest.mark.parametrize("lq, S", [(37, 256), (300, 256), (777, 256), (300, 128)])
def test_the_fourth_mirror(swg, orc, seqs, lq, S):
    q777, flat, off = seqs
    sub = _sub(swg, "BLOSUM62")
    q = q777[:lq].copy()
    u = swg.debug_prune_kmer_refine4(sub, q, GO, GE, S, flat, off).astype(np.int64)
    assert np.array_equal(u, _numpy_bound5(swg, sub, q, (GO, GE), S, flat, off)), (lq, S)
    real = np.array([not np.any(flat[int(off[i]):int(off[i + 1])] == 0) for i in range(len(off) - 1)])
    scores = orc.score_db(q, flat, off, sub, GO, GE).astype(np.int64)
    assert np.all(u[real] >= scores[real]), (lq, S)
    # one sequence at a time (no block shares a prefix with another sequence's): the same bounds
    for i in (0, 5, 60, len(off) - 4):
        one = np.array([0, off[i + 1] - off[i]], dtype=np.uint64)
        part = flat[int(off[i]):int(off[i + 1])]
        ui = swg.debug_prune_kmer_refine4(sub, q, GO, GE, S, part if len(part) else np.zeros(1, np.int8), one)
        assert int(ui[0]) == u[i], (lq, S, i)


def test_the_fourth_mirror_against_the_table_of_5(swg, seqs):
    """lq = 32 in 256 segments is one column per segment and 224 empty ones; in 32 segments the table-holding mirror of
    k = 5 walks the same columns one to a segment: the same bounds.  And a PSSM under dear gaps against numpy."""
    q777, flat, off = seqs
    sub = _sub(swg, "PAM250")
    q = q777[200:232].copy()
    u = swg.debug_prune_kmer_refine4(sub, q, GO, GE, 256, flat, off)
    _, u32 = swg.debug_prune_kmer_seg(sub, q, GO, GE, 5, 32, flat, off, table=False)
    assert np.array_equal(u, u32)
    pssm = _sub(swg, "BLOSUM62")[q777[:90].astype(np.int64)].copy()
    pssm[40, 12] = 51
    assert swg.debug_prune_table_bits(pssm, None, 5) == 8
    u = swg.debug_prune_kmer_refine4(pssm, None, -11, -1, 256, flat, off).astype(np.int64)
    assert np.array_equal(u, _numpy_bound5(swg, pssm, None, (-11, -1), 256, flat, off))


@pytest.mark.parametrize("S4", [0, 1, 32, 64, 255, 257, 512, -1])
def test_the_fourth_mirror_takes_128_and_256_only(swg, S4):
    sub = _sub(swg, "BLOSUM62")
    u = np.zeros(1, dtype=np.uint64)
    off = np.array([0, 1], dtype=np.uint64)
    one = np.array([1], dtype=np.int8)
    p = lambda a: a.ctypes.data_as(C_.c_void_p)  # noqa: E731
    f = swg.lib.swg_debug_prune_kmer_refine4
    assert f(p(sub), p(one), 1, -2, -1, S4, p(one), p(off), 1, p(u)) == swg.SWG_ERR_ARG
    assert f(p(sub), p(one), 1, -2, -1, 256, p(one), p(off), 1, p(u)) == swg.SWG_OK and u[0] == sub[1, 1]
    assert f(p(sub), p(one), 1, 1, -1, 256, p(one), p(off), 1, p(u)) == swg.SWG_ERR_ARG


def test_choice_of_the_fourth_level(swg):
    ch = swg.debug_prune_refine4_choice
    F = swg.PRUNE_REFINE4_FORCED
    # the headline's ask: k = 4 in 32 segments, 128, 256, and blocks of 5 in 256
    assert ch(lq=3000, pair_rows=HEADLINE_ROWS) == (4, 32, 128, 256, 256)
    # the other levels are what debug_prune_refine3_choice says, whatever the fourth
    for kw in (dict(), dict(forced=4), dict(forced=5, segments=8), dict(segments=32), dict(refine=64), dict(refine3=1), dict(refine3=256),
               dict(lq=200, pair_rows=300000), dict(table_bits=16)):
        for r4 in (0, 1, F):
            for bits5 in (8, 16):
                assert ch(refine4=r4, table_bits5=bits5, **kw)[:4] == swg.debug_prune_refine3_choice(**kw), (kw, r4, bits5)
    # its size edge: more rows never lose it, and the rule is the other levels' -- the build of 22^4 x 26 x lq cells and the
    # walk may cost at most half of what the cut saves; every test-sized database is far below it
    got = [ch(lq=3000, pair_rows=r)[4] for r in (10 ** 4, 10 ** 6, 10 ** 7, 10 ** 8, 10 ** 9, HEADLINE_ROWS, 10 ** 10, 10 ** 11)]
    assert got == sorted(got) and got[:3] == [0, 0, 0] and got[-3:] == [256, 256, 256], got
    edge = [r for r in range(10 ** 7, 2 * 10 ** 9, 10 ** 7) if ch(lq=3000, pair_rows=r)[4]][0]
    assert all(ch(lq=3000, pair_rows=r)[3:] == (256, 256) for r in (edge, 2 * edge)) and ch(lq=3000, pair_rows=edge - 10 ** 7)[4] == 0
    for lq in (50, 200, 367, 1000, 3000):
        for rows in (5000, 300000, 3000000):
            assert ch(lq=lq, pair_rows=rows)[4] == 0, (lq, rows)
    # every forced earlier level: off, unless forced itself
    for kw in (dict(forced=4), dict(forced=4, segments=32), dict(segments=32), dict(forced=1), dict(forced=5, segments=8), dict(refine=128),
               dict(refine=64), dict(refine=1), dict(refine3=256), dict(refine3=1), dict(forced=4, segments=32, refine=128, refine3=256)):
        assert ch(lq=3000, pair_rows=HEADLINE_ROWS, **kw)[4] == 0, kw
        assert ch(lq=3000, pair_rows=HEADLINE_ROWS, refine4=F, **kw)[4] == 256, kw
        assert ch(lq=3000, pair_rows=HEADLINE_ROWS, refine4=1, **kw)[4] == 0, kw
    # widths: 16-bit tables of k = 4 leave the third level off and the fourth with it; a k = 5 table of 16 bits is refused
    # at this size, forced or not (5 x 52 > 255 while 4 x 52 fits a byte)
    assert ch(lq=3000, pair_rows=HEADLINE_ROWS, table_bits=16)[3:] == (0, 0)
    assert ch(lq=3000, pair_rows=HEADLINE_ROWS, table_bits5=16) == (4, 32, 128, 256, 0)
    assert ch(lq=3000, pair_rows=HEADLINE_ROWS, table_bits5=16, refine4=F)[4] == 0
    assert ch(lq=3000, pair_rows=HEADLINE_ROWS, table_bits=16, refine4=F)[4] == 256
    # off is off; forced is taken as given on a small range too; an unpruned search builds nothing
    assert ch(lq=3000, pair_rows=HEADLINE_ROWS, refine4=1) == (4, 32, 128, 256, 0)
    assert ch(lq=200, pair_rows=5000, refine4=F) == (1, 1, 0, 0, 256)
    assert ch(pruned=0) == (0, 0, 0, 0, 0) and ch(pruned=0, refine4=F) == (0, 0, 0, 0, 0)
    # values that are no option
    for bad in ([0, 1, 3000, 10 ** 9, 0, 0, 0, 0, 0, 8, 256, 8], [0, 1, 3000, 10 ** 9, 0, 0, 0, 0, 0, 8, 5128, 8], [0, 1, 3000, 10 ** 9, 0, 0, 0, 0, 0, 8, 0, 4],
                [0, 1, 3000, 10 ** 9, 0, 0, 0, 0, 512, 8, 0, 8]):
        a = np.array(bad, dtype=np.int64)
        out = np.zeros(5, dtype=np.int64)
        assert swg.lib.swg_debug_prune_refine4_choice(a.ctypes.data_as(C_.c_void_p), out.ctypes.data_as(C_.c_void_p)) == swg.SWG_ERR_ARG, bad


def test_the_stages_queue_the_fourth_level_behind_the_third(swg):
    segs = [(0, 10), (10, 25), (25, 31)]
    third = swg.debug_prune_stages(segs, refine=128, refine3=256)
    fourth = swg.debug_prune_stages(segs, refine=128, refine3=256, refine4=256)
    assert [s[:3] for s in fourth] == [s[:3] for s in third]
    assert fourth[0][3] == () and third[1][3] == ("threshold", "refine", "refine3", "list")
    assert all(s[3] == ("threshold", "refine", "refine3", "refine4", "list") for s in fourth[1:])
    # a caller's threshold: the first of several stages is gated, and all three walks read the gate's word
    fixed = swg.debug_prune_stages(segs, fixed=True, refine=128, refine3=256, refine4=256)
    assert fixed[0][3] == ("gate", "refine", "refine3", "refine4", "list") and all(s[3] == ("refine", "refine3", "refine4", "list") for s in fixed[1:])
    # behind no other level; never with the prefix cut; a head and a rest
    assert swg.debug_prune_stages(segs, refine4=256)[1][3] == ("threshold", "refine4", "list")
    assert swg.debug_prune_stages(segs, refine=128, refine4=256)[1][3] == ("threshold", "refine", "refine4", "list")
    assert swg.debug_prune_stages(segs, refine=128, refine3=256, refine4=256, prefix_cut=True)[1][3] == ("threshold", "prefix_cut")
    head = swg.debug_prune_stages([(0, 40)], head_pairs=8, refine=128, refine3=256, refine4=256)
    assert [s[:2] for s in head] == [(0, 8), (8, 40)] and head[1][3] == ("threshold", "refine", "refine3", "refine4", "list")
    # the hook without the fourth level is what it was
    a = np.array([0, 0, 128, 0, 256, 3, 0, 10, 10, 25, 25, 31], dtype=np.int64)
    out = np.zeros((7, 4), dtype=np.int64)
    n = C_.c_size_t(0)
    assert swg.lib.swg_debug_prune_stages3(a.ctypes.data_as(C_.c_void_p), out.ctypes.data_as(C_.c_void_p), 7, C_.byref(n)) == swg.SWG_OK
    assert n.value == 3 and [int(v) for v in out[:3, 3]] == [0, 1 | 8 | 32 | 16, 1 | 8 | 32 | 16]
