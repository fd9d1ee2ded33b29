"""CPU: the byte-wide k-mer tables and the third level of the pruning bound, through the host hooks: the
width rule (swg_debug_prune_table_bits), the 256-segment mirror (swg_debug_prune_kmer_refine3) against a numpy
restatement and the oracle, the third choice (swg_debug_prune_refine3_choice) and the stage list with its flag."""
import ctypes as C_

import numpy as np
import pytest

GO, GE = -2, -1
C = 22


def _sub(swg, name):
    return np.asarray(swg.load_scoring(name).table(), dtype=np.int8).reshape(32, 32)


# ---------------------------------------------------------------------------------------------------------------------
# the width rule

@pytest.mark.parametrize("k, top, bits", [(4, 63, 8), (4, 64, 16), (5, 51, 8), (5, 52, 16), (4, 127, 16), (5, 127, 16), (4, 1, 8)])
def test_width_rule_at_its_edges(swg, k, top, bits):
    """k x the largest score <= 255 gives bytes: 4 x 63 = 252, 4 x 64 = 256; 5 x 51 = 255, 5 x 52 = 260.  A PSSM of 7
    columns of small scores with `top` once, at a standard residue, at class 21's and at the last index."""
    for r in (5, 27, 31):
        pssm = np.full((7, 32), -3, dtype=np.int8)
        pssm[:, 1:] = np.arange(31, dtype=np.int8) % 5 - 2
        pssm[3, r] = top
        assert swg.debug_prune_table_bits(pssm, None, k) == bits, (k, top, r)


def test_width_of_the_shipped_matrices(swg):
    q = np.arange(1, 32, dtype=np.int8)       # every residue: the largest diagonal entry is among the columns
    for name, top in (("BLOSUM62", 11), ("PAM250", 17)):
        sub = _sub(swg, name)
        assert int(sub[1:, 1:].max()) == top
        assert swg.debug_prune_table_bits(sub, q, 4) == 8 and swg.debug_prune_table_bits(sub, q, 5) == 8, name
    pssm = _sub(swg, "BLOSUM62")[q.astype(np.int64)].copy()
    pssm[2, 9] = 127
    assert swg.debug_prune_table_bits(pssm, None, 4) == 16 and swg.debug_prune_table_bits(pssm, None, 5) == 16
    # no k-mer table at other k, no query
    assert swg.lib.swg_debug_prune_table_bits(pssm.ctypes.data_as(C_.c_void_p), None, 31, 3) == swg.SWG_ERR_ARG
    assert swg.lib.swg_debug_prune_table_bits(pssm.ctypes.data_as(C_.c_void_p), None, 0, 4) == swg.SWG_ERR_ARG


def test_no_entry_of_a_byte_table_reaches_255(swg):
    """The rule's premise on a PSSM at its edge (largest score 63, k = 4): every entry of the mirror's table, which is
    what the device stores, is at most 4 x 63 -- a byte table drops nothing."""
    rng = np.random.default_rng(0x5EED0B01)
    pssm = rng.integers(-8, 64, size=(9, 32)).astype(np.int8)
    pssm[4, 7] = 63
    one = np.array([0, 1], dtype=np.uint64)
    t, _ = swg.debug_prune_kmer_refine(pssm, None, 0, 0, 256, np.array([1], dtype=np.int8), one)   # (free gaps: the largest entries)
    assert swg.debug_prune_table_bits(pssm, None, 4) == 8 and int(t.max()) <= 252 and int(t.max()) > 200


# ---------------------------------------------------------------------------------------------------------------------
# the 256-segment mirror

def _numpy_bound(swg, rows, q, gaps, S, flat, off):
    """The ordered k = 4 bound over S segments, restated: the table entries of the blocks that occur only (the recurrence of
    swg_kmer_table_kernel, all blocks at once along the query), then each sequence's walk."""
    lq = len(q) if q is not None else rows.shape[0]
    prof = rows[q.astype(np.int64)] if q is not None else rows                      # [lq][32]
    klass = np.asarray(swg.KMER_CLASS, dtype=np.int64)
    cprof = np.full((lq, C), -128, dtype=np.int64)
    for r in range(1, 32):
        cprof[:, klass[r]] = np.maximum(cprof[:, klass[r]], prof[:, r])
    colmax = np.zeros(32, dtype=np.int64)
    colmax[1:] = np.maximum(prof[:, 1:].max(axis=0), 0)
    o = off.astype(np.int64)
    seq_blocks = []
    for i in range(len(o) - 1):
        s = flat[o[i]:o[i + 1]].astype(np.int64) & 31
        n_blocks = (2 + len(s) + 3) // 4
        r = np.zeros(4 * n_blocks, dtype=np.int64)
        r[2:2 + len(s)] = s
        seq_blocks.append(r.reshape(n_blocks, 4))
    allb = np.unique(np.concatenate(seq_blocks), axis=0)
    cls = klass[allb]                                                              # [n][4]
    g, e = -(gaps[0] + gaps[1]), -gaps[1]
    W = -(-lq // S)
    n = len(allb)
    M = np.zeros((4, n), dtype=np.int64)
    A = np.zeros((4, n), dtype=np.int64)
    best = np.zeros(n, dtype=np.int64)
    table = np.zeros((n, S), dtype=np.int64)
    for i in range(lq):
        diag = np.zeros(n, dtype=np.int64)
        left = np.zeros(n, dtype=np.int64)
        B = np.zeros(n, dtype=np.int64)
        for j in range(4):
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
    """300 random sequences of 0..40 residues, the odd indices and residue 31 among them, and three that copy a stretch of the query"""
    rng = np.random.default_rng(0x5EED0B02)
    q = swg.synth_query(0x5EED0B03, 3000)
    parts = [rng.integers(1, 32, size=int(n)).astype(np.int8) for n in rng.integers(0, 41, size=297)]
    parts += [q[100:140].copy(), q[2990:3000].copy(), q[0:7].copy()]
    off = np.zeros(len(parts) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in parts])
    return q, np.concatenate(parts).astype(np.int8), off


@pytest.mark.parametrize("lq", [1, 256, 300, 3000])
def test_mirror_at_256_segments(swg, orc, seqs, lq):
    q3000, flat, off = seqs
    sub = _sub(swg, "BLOSUM62")
    q = q3000[:lq].copy() if lq > 256 else q3000[100:100 + lq].copy()
    t, u = swg.debug_prune_kmer_refine(sub, q, GO, GE, 256, flat, off)
    u = u.astype(np.int64)
    assert t.shape == (C ** 4, 256) and t.dtype == np.uint16
    W = -(-lq // 256)
    empty = [s for s in range(256) if s * W >= lq]
    assert len(empty) == {1: 255, 256: 0, 300: 106, 3000: 6}[lq] and not np.any(t[:, empty])
    assert np.any(t[:, (lq - 1) // W])
    assert np.array_equal(u, _numpy_bound(swg, sub, q, (GO, GE), 256, flat, off)), lq
    scores = orc.score_db(q, flat, off, sub, GO, GE).astype(np.int64)
    assert np.all(u >= scores), (lq, int((scores - u).max()))
    if lq in (256, 3000):
        # 256 = 256 x 1 = 128 x 2 and 3000 = 250 x 12 = 125 x 24: each of the 128 segments is two whole ones of the 256
        _, u128 = swg.debug_prune_kmer_refine(sub, q, GO, GE, 128, flat, off, table=False)
        assert np.all(u <= u128.astype(np.int64)), lq
        if lq == 3000:
            assert u.sum() < u128.sum()
    # the row maxima are the unsegmented table
    t1, _ = swg.debug_prune_kmer(sub, q, GO, GE, 4, flat[:1], np.array([0, 1], dtype=np.uint64))
    assert np.array_equal(t.max(axis=1), t1)


def test_mirror_of_a_pssm_at_256_segments(swg, orc, seqs):
    """A PSSM holding 127 (the 16-bit tables' case) under dear gaps"""
    q3000, flat, off = seqs
    sub = _sub(swg, "BLOSUM62")
    q = q3000[:300]
    pssm = sub[q.astype(np.int64)].copy()
    pssm[150, 12] = 127
    assert swg.debug_prune_table_bits(pssm, None, 4) == 16
    _, u = swg.debug_prune_kmer_refine(pssm, None, -11, -1, 256, flat, off, table=False)
    assert np.array_equal(u.astype(np.int64), _numpy_bound(swg, pssm, None, (-11, -1), 256, flat, off))


@pytest.mark.parametrize("S3", [0, 1, 32, 64, 128, 255, 257, 512, -1])
def test_the_third_mirror_takes_256_only(swg, S3):
    sub = _sub(swg, "BLOSUM62")
    u = np.zeros(1, dtype=np.uint64)
    off = np.array([0, 1], dtype=np.uint64)
    one = np.array([1], dtype=np.int8)
    p = lambda a: a.ctypes.data_as(C_.c_void_p)  # noqa: E731
    f = swg.lib.swg_debug_prune_kmer_refine3
    assert f(p(sub), p(one), 1, -2, -1, S3, p(one), p(off), 1, None, p(u)) == swg.SWG_ERR_ARG
    assert f(p(sub), p(one), 1, -2, -1, 256, p(one), p(off), 1, None, p(u)) == swg.SWG_OK and u[0] == sub[1, 1]


# ---------------------------------------------------------------------------------------------------------------------
# the third choice and the stages

def test_choice_of_the_third_level(swg):
    ch = swg.debug_prune_refine3_choice
    # the headline's ask: k = 4 in 32 segments, 128, 256
    assert ch(lq=3000, pair_rows=1900000000) == (4, 32, 128, 256)
    # the other levels are what debug_prune_refine_choice says, whatever the third
    for kw in (dict(), dict(forced=4), dict(forced=5, segments=8), dict(segments=32), dict(refine=64), dict(lq=200, pair_rows=300000)):
        for r3 in (0, 1, 256):
            for bits in (8, 16):
                assert ch(refine3=r3, table_bits=bits, **kw)[:3] == swg.debug_prune_refine_choice(**kw), (kw, r3, bits)
    # more rows never lose it; a few thousand and a few million pair rows (the tests' databases) never have it
    got = [ch(lq=3000, pair_rows=r)[3] for r in (10 ** 4, 10 ** 6, 10 ** 7, 10 ** 8, 10 ** 9, 1900000000, 10 ** 10, 10 ** 11)]
    assert got == sorted(got) and got[:3] == [0, 0, 0] and got[-3:] == [256, 256, 256], got
    for lq in (50, 200, 367, 1000, 3000):
        for rows in (5000, 300000, 3000000):
            assert ch(lq=lq, pair_rows=rows)[3] == 0, (lq, rows)
    # 16-bit tables: the 256-segment table would be twice the second level's bytes -- off
    assert ch(lq=3000, pair_rows=1900000000, table_bits=16) == (4, 32, 128, 0)
    # any forced prune_kmer, prune_segments or prune_refine: off, unless forced itself
    for kw in (dict(forced=4), dict(forced=4, segments=32), dict(segments=32), dict(forced=1), dict(forced=5, segments=8),
               dict(refine=128), dict(refine=64), dict(refine=1), dict(forced=4, segments=32, refine=128)):
        assert ch(lq=3000, pair_rows=1900000000, **kw)[3] == 0, kw
        assert ch(lq=3000, pair_rows=1900000000, refine3=256, **kw)[3] == 256, kw
        assert ch(lq=3000, pair_rows=1900000000, refine3=256, table_bits=16, **kw)[3] == 256, kw
        assert ch(lq=3000, pair_rows=1900000000, refine3=1, **kw)[3] == 0, kw
    # off is off; forced is taken as given on a small range too; an unpruned search builds nothing
    assert ch(lq=3000, pair_rows=1900000000, refine3=1) == (4, 32, 128, 0)
    assert ch(lq=200, pair_rows=5000, refine3=256) == (1, 1, 0, 256)
    assert ch(pruned=0) == (0, 0, 0, 0) and ch(pruned=0, refine3=256) == (0, 0, 0, 0)
    # values that are no option
    for bad in ([0, 1, 3000, 10 ** 9, 0, 0, 0, 0, 128, 8], [0, 1, 3000, 10 ** 9, 0, 0, 0, 0, 512, 8], [0, 1, 3000, 10 ** 9, 0, 0, 0, 0, 0, 4],
                [0, 1, 3000, 10 ** 9, 0, 0, 0, 32, 0, 8]):
        a = np.array(bad, dtype=np.int64)
        out = np.zeros(4, dtype=np.int64)
        assert swg.lib.swg_debug_prune_refine3_choice(a.ctypes.data_as(C_.c_void_p), out.ctypes.data_as(C_.c_void_p)) == swg.SWG_ERR_ARG, bad


def test_the_stages_queue_the_third_level_behind_the_second(swg):
    segs = [(0, 10), (10, 25), (25, 31)]
    plain = swg.debug_prune_stages(segs, refine=128)
    third = swg.debug_prune_stages(segs, refine=128, refine3=256)
    assert [s[:3] for s in third] == [s[:3] for s in plain]
    assert third[0][3] == () and plain[1][3] == ("threshold", "refine", "list")
    assert all(s[3] == ("threshold", "refine", "refine3", "list") for s in third[1:])
    # a caller's threshold: the first of several stages is gated, and both walks read the gate's word
    fixed = swg.debug_prune_stages(segs, fixed=True, refine=128, refine3=256)
    assert fixed[0][3] == ("gate", "refine", "refine3", "list") and all(s[3] == ("refine", "refine3", "list") for s in fixed[1:])
    # behind no second level; never with the prefix cut; a head and a rest
    assert swg.debug_prune_stages(segs, refine3=256)[1][3] == ("threshold", "refine3", "list")
    assert swg.debug_prune_stages(segs, refine=128, refine3=256, prefix_cut=True)[1][3] == ("threshold", "prefix_cut")
    head = swg.debug_prune_stages([(0, 40)], head_pairs=8, refine=128, refine3=256)
    assert [s[:2] for s in head] == [(0, 8), (8, 40)] and head[1][3] == ("threshold", "refine", "refine3", "list")
    # the hook without the third level is what it was
    a = np.array([0, 0, 128, 0, 3, 0, 10, 10, 25, 25, 31], dtype=np.int64)
    out = np.zeros((7, 4), dtype=np.int64)
    n = C_.c_size_t(0)
    assert swg.lib.swg_debug_prune_stages(a.ctypes.data_as(C_.c_void_p), out.ctypes.data_as(C_.c_void_p), 7, C_.byref(n)) == swg.SWG_OK
    assert n.value == 3 and [int(v) for v in out[:3, 3]] == [0, 1 | 8 | 16, 1 | 8 | 16]
