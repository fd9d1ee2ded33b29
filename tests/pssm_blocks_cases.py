"""Shared by the tests of the PSSM construction's options "pssm_blocks" (PSI-BLAST's per-column alignment blocks) and
"pssm_purge" (near-identical hits dropped): an independent numpy restatement of the equations of include/swg.h, column by
column and not segment by segment as the library works, and seeded generators of the cases the whole-query model cannot
tell apart.  The restatement sums in numpy's order: values agree with the library to 1e-9, the int8 PSSM in every entry
because no case has a value within 1e-6 of a half-integer (test_pssm_blocks_host.py asserts that margin)."""
import numpy as np

import pssm_build_cases as pc


# ---- the model, restated ---------------------------------------------------------------------------------------------
def extents_of(lq, alignments):
    """[rows, 2]: row 0 spans the query, a hit of score > 0 its path's [q_begin, q_end), a hit of score 0 nothing."""
    ext = np.zeros((len(alignments) + 1, 2), dtype=np.int64)
    ext[0] = (0, lq)
    for r, a in enumerate(alignments, start=1):
        if a["score"] > 0:
            ext[r] = (a["q_begin"], a["q_end"])
    return ext


def purge_numpy(X, ext, T):
    """The greedy purge on the raw rows (gaps and empty cells do not count; membership in A plays no part), in integers
    -> the purged rows' indices."""
    res = (X >= 1) & (X <= 31)
    kept, purged = [], []
    for r in range(1, len(X)):
        if ext[r, 0] >= ext[r, 1]:
            continue
        both = res[r] & res[0]
        c, i = int(both.sum()), int((both & (X[r] == X[0])).sum())
        drop = c >= 1 and i == c
        for s in kept:
            both = res[r] & res[s]
            c, i = int(both.sum()), int((both & (X[r] == X[s])).sum())
            drop = drop or (c >= 1 and 100 * i >= T * c)
        (purged if drop else kept).append(r)
    return purged


def _block(Xb):
    """Counts, weights and the diversity figure within one block over its member rows Xb [members, width] (0: empty)."""
    onehot = (Xb[:, :, None] == np.arange(32)[None, None, :]) & (Xb[:, :, None] > 0)
    N = onehot.sum(axis=0)
    k, m = (N > 0).sum(axis=1), N.sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        share = np.where(onehot, 1.0 / (k[None, :, None] * N[None, :, :]), 0.0)
    return share.sum(axis=(1, 2)), (float(k[m >= 1].mean()) if (m >= 1).any() else 0.0)


def model_numpy(sub, query, flat, offsets, alignments, freq=None, beta=10.0, blocks=False, purge=0):
    """pssm_build_cases.model_numpy with the two options -> the same dict, info with n_purged."""
    sub = np.asarray(sub, dtype=np.int64).reshape(32, 32)
    P = pc.builtin_freq() if freq is None else np.asarray(freq, dtype=np.float64)
    P = P / P.sum()
    inA = P > 0
    inA[0] = False
    lam = pc.lambda_numpy(sub, P)
    query = np.asarray(query, dtype=np.int64)
    lq = len(query)
    X = pc.rows_of(query, flat, offsets, alignments)
    ext = extents_of(lq, alignments)
    purged = purge_numpy(X, ext, purge) if purge else []
    X[purged] = 0
    ext[purged] = 0
    X = np.where((X >= 1) & (X <= 31) & inA[np.minimum(X, 31)], X, 0)
    m = (X > 0).sum(axis=0)
    F, nbar_p = np.zeros((lq, 32)), np.zeros(lq)
    cache = {}
    for p in range(lq):
        members = np.flatnonzero((ext[:, 0] <= p) & (p < ext[:, 1])) if blocks else np.arange(len(X))
        L, U = (int(ext[members, 0].max()), int(ext[members, 1].min())) if blocks else (0, lq)
        key = (members.tobytes(), L, U)
        if key not in cache:
            cache[key] = _block(X[members, L:U])
        w, nbar_p[p] = cache[key]
        col = X[members, p]
        for a in range(1, 32):
            F[p, a] = w[col == a].sum()
        if m[p] >= 1:
            F[p] /= w[col > 0].sum()
    E = np.exp(lam * sub)
    G = P[None, :] * (F[:, inA] @ E[inA, :])
    alpha = np.minimum(nbar_p, m) - 1.0
    with np.errstate(divide="ignore", invalid="ignore"):
        Q = (alpha[:, None] * F + beta * G) / (alpha + beta)[:, None]
        V = np.log(Q / P[None, :]) / lam
    have = (m >= 1)[:, None] & inA[None, :]
    values = np.where(have, V, 0.0)
    rounded = np.sign(values) * np.floor(np.abs(values) + 0.5)
    pssm = sub[query].copy()
    pssm[:, 0] = 0
    pssm = np.where(have, np.clip(rounded, -128, 127), pssm).astype(np.int8)
    info = {"lambda": lam, "n_distinct": float(nbar_p[m >= 1].mean()) if (m >= 1).any() else 0.0,
            "n_rows": 1 + sum(a["score"] > 0 for a in alignments) - len(purged),
            "n_observed": int(((X[1:] > 0).sum(axis=0) > 0).sum()),
            "n_clamped": int((have & ((rounded < -128) | (rounded > 127))).sum()), "n_purged": len(purged)}
    return {"pssm": pssm, "values": values, "m": m, "info": info, "have": have, "purged": purged, "ext": ext}


def segments_of(ext):
    """The number of runs of columns between two consecutive extent boundaries."""
    live = ext[ext[:, 0] < ext[:, 1]]
    return len(set(live.ravel().tolist())) - 1


# ---- generators ------------------------------------------------------------------------------------------------------
def staggered(seed=61, lq=90, n_hits=8):
    """Hits whose extents all begin and end in different columns, none at the query's ends: 2 n_hits + 1 segments.  The
    two columns at either end of an extent are kept as the query's so that the local alignment ends there."""
    rng = np.random.default_rng(seed)
    q = pc.random_seq(rng, lq)
    seqs = []
    for h in range(n_hits):
        lo, hi = 3 + 4 * h, lq - 4 - 5 * h
        seqs.append(pc.relative(rng, q, 0.25, keep=(lo, lo + 1, lo + 2, hi - 3, hi - 2, hi - 1), lo=lo, hi=hi, flank=0))
    flat, off = pc.pack(seqs)
    return q, flat, off, list(range(n_hits))


def two_domains(seed=52, lq=100):
    """Domain [5, 40) hit by 1 row, domain [55, 95) hit by 20: columns 0..4, 40..54 and 95..99 are row 0's alone."""
    rng = np.random.default_rng(seed)
    q = pc.random_seq(rng, lq)
    seqs = [pc.relative(rng, q, 0.3, keep=(5, 6, 38, 39), lo=5, hi=40, flank=0)]
    seqs += [pc.relative(rng, q, 0.1 + 0.02 * h, keep=(55, 56, 93, 94), lo=55, hi=95, flank=0) for h in range(20)]
    flat, off = pc.pack(seqs)
    return q, flat, off, list(range(21))


def gap_row(seed=53, lq=80):
    """Five partial hits of columns [10, 70); the first has columns 40 and 41 deleted, so its extent contains them and it
    shows a gap there."""
    rng = np.random.default_rng(seed)
    q = pc.random_seq(rng, lq)
    seqs = [pc.relative(rng, q, 0.1, keep=(10, 11, 68, 69), lo=10, hi=70, dele=[(40, 2)], flank=3)]
    seqs += [pc.relative(rng, q, 0.15 + 0.05 * h, keep=(10 + h, 11 + h, 68 - h, 69 - h), lo=10 + h, hi=70 - h, flank=3) for h in range(1, 5)]
    flat, off = pc.pack(seqs)
    return q, flat, off, list(range(5))


def _changed(rng, s, columns):
    """s with every listed column changed to another standard residue."""
    s = s.copy()
    for p in columns:
        s[p] = rng.choice([x for x in pc.STD_IDX if x != s[p]])
    return s


def purge_family(seed=54, lq=100):
    """A query and ungapped relatives that span it, with identities known by construction (all of 100 columns shared):
      0  A   = the query with 20 columns changed                     (80 % to the query)
      1  B94 = A with 6 more columns changed                         (94 % to A: dropped at 94)
      2  B93 = A with 7 other columns changed                        (93 % to A: kept at 94)
      3  the query itself                                            (dropped at any T)
      4  C   = B94 with 5 further columns changed                    (95 % to B94, 89 % to A, 82 % to B93)
    Columns 0..4 and 95..99 are never changed, so every local alignment spans the query."""
    rng = np.random.default_rng(seed)
    q = pc.random_seq(rng, lq)
    cols = rng.permutation(np.arange(5, lq - 5))
    a = _changed(rng, q, cols[:20])
    b94 = _changed(rng, a, cols[20:26])
    b93 = _changed(rng, a, cols[26:33])
    c = _changed(rng, b94, cols[33:38])
    flat, off = pc.pack([a, b94, b93, q.copy(), c])
    return q, flat, off


def blocks_cases(orc):
    """name -> a case dict as pssm_build_cases.host_cases gives them: the new cases of the per-column model."""
    b62, gaps = pc.table("BLOSUM62"), pc.MATRICES["BLOSUM62"]
    cases = {}
    for name, (q, flat, off, hits) in (("staggered", staggered()), ("two_domains", two_domains()), ("gap_row", gap_row())):
        cases[name] = dict(sub=b62, gaps=gaps, q=q, flat=flat, off=off, al=pc.align(orc, q, flat, off, hits, b62, gaps), freq=None, beta=10.0)
    return cases
