"""Shared builder of databases with planted, analytically known scores (plain module, no tests of its own).

The device top-K (swg_topk_hist_kernel -> swg_topk_threshold_kernel -> swg_topk_compact_kernel, then the host's sort of
the candidates or its fall-back) has edges that only show on databases far larger than an oracle run per test should
pay for, and at exact scores: the K-th best at a named histogram bin, exactly as many ties as the candidate list holds.
This construction plants any score 0 .. 4199 at the price of one np.repeat:

  table:     sub[A][A] = 100, sub[C][C] = 1, every other entry -4
  query:     A^a C^c                      (a = 41, c = 99 by default: 140 columns, one pass)
  sequence:  W^p A^i C^j W^s              (flanks p, s in 0 .. 8)
  score:     100 min(i, a) + min(j, c)    for any gap scores <= (0, -1): the best local alignment is the last min(i, a)
                                          A's followed by the first min(j, c) C's, no gap pays, W never scores

The flanks change a sequence's length, not its score: the database is sorted by length (stable, descending), so the
members of a tie land at sorted ranks unrelated to their original indices.  An empty record scores 0.  For a batch,
query r is A^(a_r) C^(c_r) and the same formula gives every query's scores of one database.

tests/test_topk_cases_host.py proves, with the oracle, that the analytic scores of every case below are the real ones
and that every case has the property it is named for; tests/test_gpu_topk.py then compares the library's hits with
oracle.topk(analytic scores, k).
"""
import numpy as np

A, C, W = 1, 3, 23                  # residue indices of the letters (letter - 'A' + 1)
GAPS = (-11, -1)
BIN = 128                           # sequences per bin of a packed database: slots = bins * 128, the rest padding
CAND_CAP, MULTI_CAP = 8192, 1024    # candidates the device keeps: a single search, each query of a batch
HIST_SWEEP, MULTI_SWEEP = 512 * 256, 64 * 256   # slots one sweep of the histogram's grid covers
LAST_BIN = 4095                     # every score >= 4095 shares the histogram's last bin


def table():
    sub = np.full((32, 32), -4, dtype=np.int8)
    sub[A, A] = 100
    sub[C, C] = 1
    return sub


def query(a=41, c=99):
    return np.repeat(np.array([A, C], dtype=np.int8), [a, c])


def pssm(a, c):
    """The position-specific twin of query(a, c): row x = the table's row of the query's residue x."""
    return table()[query(a, c).astype(np.int64)]


def analytic(i, j, a=41, c=99):
    return (100 * np.minimum(i, a) + np.minimum(j, c)).astype(np.int32)


def assemble(i, j, p, s):
    """Sequences W^p A^i C^j W^s -> (flat int8, offsets uint64[n + 1])."""
    parts = np.stack([p, i, j, s], axis=1).astype(np.int64)
    flat = np.repeat(np.tile(np.array([W, A, C, W], dtype=np.int8), len(i)), parts.ravel())
    off = np.zeros(len(i) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(parts.sum(axis=1))
    return flat, off


def sorted_order(off):
    """Original index of every sorted rank, as swg_db_pack orders a database: by length, descending, stable."""
    lens = np.diff(off.astype(np.int64))
    return np.argsort(-lens, kind="stable")


def n_slots(n):
    return (n + BIN - 1) // BIN * BIN


def _case(i, j, p, s, rng, shuffle=True, **extra):
    i, j, p, s = (np.asarray(v, dtype=np.int64) for v in (i, j, p, s))
    if shuffle:          # planted sequences spread over the original index range
        perm = rng.permutation(len(i))
        i, j, p, s = i[perm], j[perm], p[perm], s[perm]
    flat, off = assemble(i, j, p, s)
    return dict(flat=flat, offsets=off, i=i, j=j, n=len(i), scores=analytic(i, j), **extra)


def planted(plants, n_filler, filler_max, seed, flank_max=8):
    """plants: [(score, count)] (score = 100 i + j with j < 100); n_filler further sequences with scores drawn from
    0 .. filler_max; flanks drawn from 0 .. flank_max on both sides; shuffled."""
    rng = np.random.default_rng(seed)
    sc = np.concatenate([np.repeat(np.array([v for v, _ in plants], dtype=np.int64), [m for _, m in plants]),
                         rng.integers(0, filler_max + 1, size=n_filler)])
    assert sc.min() >= 0 and sc.max() <= 4199
    n = len(sc)
    return _case(sc // 100, sc % 100, rng.integers(0, flank_max + 1, size=n), rng.integers(0, flank_max + 1, size=n), rng)


# ---- single search: the K-th best score at a named bin -------------------------------------------------------------
# 4094: the last bin the device may select on; 4095, 4096: the shared last bin (host fall-back; from 4096 the f16 cells
# flag the pair and it is re-run first); 15 | 16 17 and 4079 | 4080: either side of a boundary between two threads of
# the threshold kernel (16 bins each); 0: k larger than the number of non-zero scores.
THRESHOLDS = (4094, 4095, 4096, 15, 16, 17, 4079, 4080, 0)


def threshold_case(T):
    """K-th best score exactly T, inside a tie of 4 (the 2nd of them): above it a handful of far higher scores (4200-class
    ones included) and 3 + 3 at T + 1 and T + 2 -- bins of the SAME thread of the threshold kernel unless T is a thread's
    last bin --, below it 300 fillers (all at 0 when T = 0).  333 or so sequences: the last bin has padding slots.
    ks: k (the named one), 1, the count of the far higher scores alone, and n - 1, n, n + 1."""
    high = [(v, m) for v, m in ((4199, 1), (4150, 1), (4100, 1), (4096, 2), (4095, 1), (2000, 2), (400, 1)) if v > T + 2]
    near = [(v, 3) for v in (T + 1, T + 2) if v <= 4199]
    c = planted(high + near + [(T, 4)], 300, min(max(T - 1, 0), 330), seed=1000 + T)
    above = sum(m for _, m in high + near)
    c["T"] = T
    c["k"] = above + 2
    c["ks"] = (c["k"], 1, sum(m for _, m in high), c["n"] - 1, c["n"], c["n"] + 1)
    return c


# ---- single search: ties against the candidate capacity ------------------------------------------------------------
TIES_T = 230
TIES_N = 12001
TIES_KS = (1, 100, 101, 150, 4096)                          # below, at and inside the tie
TIES_KS_HALF_CAP = (4095, 4096, 4097, 8193)                 # the device selects for k <= capacity / 2
TIES_KS_COUNT = (TIES_N - 1, TIES_N, TIES_N + 1)


def ties_case(n_tie):
    """12 001 sequences: 100 distinct-ish scores above T = 230 (231 .. 330, one each), exactly n_tie at T, the rest
    below.  n_tie = 8092: 8192 candidates for every k in 101 .. 8192 (the device's list, full); 8093: one more."""
    return planted([(v, 1) for v in range(TIES_T + 1, TIES_T + 101)] + [(TIES_T, n_tie)],
                   TIES_N - 100 - n_tie, TIES_T - 1, seed=8000 + n_tie)


# ---- single search: more slots than one sweep of the histogram's grid ----------------------------------------------
SWEEP_N = 150000
SWEEP_KS = (1, 50, 60, 4096)


def sweep_case():
    """150 000 sequences (not a multiple of 128).  The 50 best, 100 .. 103, are one A and 0 .. 3 C's without flanks,
    1 .. 4 residues: they sort LAST, beyond slot 131 072.  Everything else is C^j, j <= 30, with flanks of 5 .. 16."""
    rng = np.random.default_rng(150)
    nf = SWEEP_N - 50
    pf = rng.integers(0, 9, size=nf)
    i = np.concatenate([np.ones(50, np.int64), np.zeros(nf, np.int64)])
    j = np.concatenate([np.arange(50) % 4, rng.integers(0, 31, size=nf)])
    p = np.concatenate([np.zeros(50, np.int64), pf])
    s = np.concatenate([np.zeros(50, np.int64), np.maximum(rng.integers(0, 9, size=nf), 5 - pf)])
    return _case(i, j, p, s, rng)


# ---- single search: nothing but ties -------------------------------------------------------------------------------
ALL_TIES_KS = (5, 20, 4096)


def all_ties_case():
    """9000 empty records and 10 sequences of one W: 9010 scores of 0, more than the candidate list holds."""
    rng = np.random.default_rng(9)
    z = np.zeros(9010, np.int64)
    p = z.copy()
    p[:10] = 1
    return _case(z, z, p, z, rng)


# ---- a batch of queries ----------------------------------------------------------------------------------------------
BATCH_QUERIES = ((2, 20), (3, 10), (40, 95), (5, 50))
BATCH_K = 100
BATCH_KS = (1, BATCH_K, 512, 513)           # the device selects for k <= 512
BATCH_LONG = 110


def batch_case():
    """20 001 short sequences (more than 16 384 slots), and for k = 100:
      query 0 = A^2 C^20:  exactly 1024 sequences reach its best score 220 (i >= 2 and j >= 20): the device's list, full
      query 1 = A^3 C^10:  exactly 1025 reach its best score 310 (i >= 3 and j >= 10): that row alone falls back
      query 2 = A^40 C^95: 110 sequences reach its best score 4095 (the only long ones): the shared last bin
      query 3 = A^5 C^50:  ordinary
    Groups: the 110 long ones and 300 of (i = 3, j >= 20) count for queries 0 and 1, 614 of (i = 2, j >= 20) for query 0
    alone, 615 of (i = 3, 10 <= j < 20) for query 1 alone; the fillers reach neither."""
    rng = np.random.default_rng(20001)
    nf = 20001 - (BATCH_LONG + 300 + 614 + 615)
    fi = rng.integers(0, 4, size=nf)
    fj = rng.integers(0, 31, size=nf)
    fj = np.where(((fi == 2) & (fj >= 20)) | ((fi == 3) & (fj >= 10)), fj % 10, fj)
    i = np.concatenate([rng.integers(40, 42, size=BATCH_LONG), np.full(300, 3), np.full(614, 2), np.full(615, 3), fi])
    j = np.concatenate([rng.integers(95, 100, size=BATCH_LONG), rng.integers(20, 31, size=300), rng.integers(20, 31, size=614),
                        rng.integers(10, 20, size=615), fj])
    n = len(i)
    return _case(i, j, rng.integers(0, 9, size=n), rng.integers(0, 9, size=n), rng)


CHUNK_QUERIES = 300                          # a batch is searched in chunks of 256 queries
CHUNK_K = 5


def chunk_queries():
    return [(3 + r % 6, 20 + r % 21) for r in range(CHUNK_QUERIES)]


def chunk_case():
    """1500 sequences with i in 0 .. 8 and j in 0 .. 40 for 300 queries A^(3 .. 8) C^(20 .. 40): two chunks whose rows
    share the top-K buffers, every query's candidates few enough that two chunks' worth would still fit one row."""
    rng = np.random.default_rng(300)
    n = 1500
    return _case(rng.integers(0, 9, size=n), rng.integers(0, 41, size=n), rng.integers(0, 9, size=n),
                 rng.integers(0, 9, size=n), rng, shuffle=False)


def kth_and_count(scores, k):
    """-> (k-th best score, number of scores >= it): the threshold and the candidates of a selection of k."""
    s = np.sort(np.asarray(scores))[::-1]
    T = int(s[min(k, len(s)) - 1])
    return T, int((s >= T).sum())
