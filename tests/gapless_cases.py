"""Shared helpers of the gapless-search tests (plain module, no tests of its own).

The gapless score of a pair is the best-scoring ungapped diagonal segment, H[i][j] = max(0, H[i-1][j-1] + S(q_i, d_j)),
maximum over all cells.  Truth everywhere is the oracle with the gaps priced out (PRICED_OUT: no gap can pay while the
query's score bound 127 lq stays far below 2^20, i.e. for every query of the tests); gapless_numpy restates it directly,
as a running floored sum along every diagonal."""
import numpy as np

PRICED_OUT = (-(1 << 20), 0)


def oracle_gapless(orc, q, flat, off, sub):
    return orc.score_db(np.asarray(q, dtype=np.int8), flat, off, np.asarray(sub, dtype=np.int8), *PRICED_OUT)


def gapless_pair_numpy(S):
    """S[i, j] = score of query position i against residue j of the sequence -> best floored diagonal sum."""
    lq, ld = S.shape
    h = np.zeros(ld + 1, dtype=np.int64)
    best = 0
    for i in range(lq):
        h[1:] = np.maximum(0, h[:-1] + S[i])     # (the right-hand side is evaluated first: h[:-1] is the row above)
        h[0] = 0
        best = max(best, int(h.max()))
    return best


def gapless_numpy(q, flat, off, sub=None, pssm=None):
    """Scores of an index query (with its table) or of a PSSM (lq x 32) against every sequence."""
    rows = np.asarray(pssm, dtype=np.int64) if pssm is not None else np.asarray(sub, dtype=np.int64)[np.asarray(q, dtype=np.int64)]
    out = np.zeros(len(off) - 1, dtype=np.int32)
    for n in range(len(off) - 1):
        d = np.asarray(flat[int(off[n]):int(off[n + 1])], dtype=np.int64)
        out[n] = gapless_pair_numpy(rows[:, d]) if len(d) else 0
    return out


def pack(seqs):
    flat = np.concatenate(seqs).astype(np.int8) if seqs else np.zeros(0, dtype=np.int8)
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return flat, off


def expected_hits(truth, k, sel=None):
    sel = np.arange(len(truth)) if sel is None else np.unique(np.asarray(sel, dtype=np.int64))
    return [(-s, i) for s, i in sorted((-int(truth[i]), int(i)) for i in sel)[:k]]


def ceiling_db(rng, query, n_copies=40, n_random=2000):
    """The database of the ceiling tests: whole-sequence copies q[a:a+n] for n = 32 (127 n = 4064: exact, unflagged),
    33 (4191: flagged), 258 (32766) and 259 (32893: beyond int16) under diag127, n_copies of each with varying a, mixed
    with n_random random sequences of the same four lengths -> (flat, off, copy_len) with copy_len[i] = n or 0."""
    seqs, copy_len = [], []
    for n in (32, 33, 258, 259):
        for c in range(n_copies):
            a = int(rng.integers(0, len(query) - n + 1))
            seqs.append(query[a:a + n].copy())
            copy_len.append(n)
    for i in range(n_random):
        seqs.append(rng.integers(1, 32, size=(32, 33, 258, 259)[i % 4]).astype(np.int8))
        copy_len.append(0)
    order = rng.permutation(len(seqs))
    seqs = [seqs[i] for i in order]
    flat, off = pack(seqs)
    return flat, off, np.array(copy_len)[order]
