"""Shared by the PSSM-construction tests (swg_pssm_build*, swg_pssm_from_paths): seeded generators of queries with
families of hits, and an independent numpy restatement of the model in include/swg.h ("a PSSM from a query's hits").
The restatement is vectorised and sums in numpy's order, so it agrees with the library to rounding, not to the bit:
values within 1e-9, and the int8 PSSM in every entry because no case generated here has a value within 1e-6 of a
half-integer (test_pssm_build_host.py asserts that margin for every case)."""
import functools

import numpy as np

MATRICES = {"BLOSUM62": (-11, -1), "BLOSUM45": (-13, -3), "PAM250": (-10, -2)}
# the built-in background of swg_synth_db (percent), restated: the restatement reads no table of the library's
BUILTIN = dict(L=9.65, A=8.25, G=7.07, V=6.86, E=6.72, S=6.65, I=5.91, K=5.80, R=5.53, D=5.46,
               T=5.36, P=4.74, N=4.06, Q=3.93, F=3.86, Y=2.92, M=2.41, H=2.27, C=1.38, W=1.10)
STANDARD = "ARNDCQEGHILKMFPSTWYV"
GAP = 32


def idx(ch):
    return 31 if ch == "*" else ord(ch.upper()) - ord("A") + 1


def builtin_freq():
    f = np.zeros(32)
    for ch, v in BUILTIN.items():
        f[idx(ch)] = v
    return f


@functools.lru_cache(maxsize=None)
def table(name):
    import swg_loader
    t = swg_loader.load().load_scoring(name).table()
    t.setflags(write=False)
    return t


# ---- the model, restated ---------------------------------------------------------------------------------------------
def lambda_numpy(sub, freq=None):
    """The positive root of sum P_a P_b exp(lambda s_ab) = 1 by bisection; None when there is none."""
    P = builtin_freq() if freq is None else np.asarray(freq, dtype=np.float64)
    P = P / P.sum()
    A = np.flatnonzero(P > 0)
    S = np.asarray(sub, dtype=np.float64)[np.ix_(A, A)]
    PP = np.outer(P[A], P[A])
    if not ((PP * S).sum() < 0 and S.max() > 0):
        return None
    phi = lambda lam: (PP * np.exp(lam * S)).sum() - 1.0
    hi = 1.0
    while phi(hi) <= 0:
        hi *= 2
    lo = 0.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if phi(mid) > 0:
            hi = mid
        else:
            lo = mid
    return 0.5 * (lo + hi)


def rows_of(query, flat, offsets, alignments):
    """The query-anchored rows [1 + hits, lq]: 0 empty, 1..31 a residue, 32 a gap."""
    lq = len(query)
    X = np.zeros((len(alignments) + 1, lq), dtype=np.int64)
    X[0] = query
    for r, a in enumerate(alignments, start=1):
        if a["score"] <= 0:
            continue
        d = flat[int(offsets[a["index"]]):int(offsets[a["index"] + 1])]
        qp, dp = a["q_begin"], a["d_begin"]
        for op in a["ops"]:
            if op == "M":
                X[r, qp] = d[dp]; qp += 1; dp += 1
            elif op == "D":
                X[r, qp] = GAP; qp += 1
            else:
                dp += 1
        assert (qp, dp) == (a["q_end"], a["d_end"])
    return X


def model_numpy(sub, query, flat, offsets, alignments, freq=None, beta=10.0):
    """-> dict(pssm int8[lq, 32], values float64[lq, 32], m int[lq], info dict) by the equations of include/swg.h."""
    sub = np.asarray(sub, dtype=np.int64).reshape(32, 32)
    P = builtin_freq() if freq is None else np.asarray(freq, dtype=np.float64)
    P = P / P.sum()
    inA = P > 0
    inA[0] = False
    lam = lambda_numpy(sub, P)
    query = np.asarray(query, dtype=np.int64)
    X = rows_of(query, flat, offsets, alignments)
    R, lq = X.shape
    X = np.where((X >= 1) & (X <= 31) & inA[np.minimum(X, 31)], X, 0)        # gaps and residues outside A: empty
    onehot = (X[:, :, None] == np.arange(32)[None, None, :]) & (X[:, :, None] > 0)   # [R, lq, 32]
    N = onehot.sum(axis=0)                                                    # [lq, 32]
    k, m = (N > 0).sum(axis=1), N.sum(axis=1)
    nbar = float(k[m >= 1].mean()) if (m >= 1).any() else 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        share = np.where(onehot, 1.0 / (k[None, :, None] * N[None, :, :]), 0.0)      # 1 / (k_p n[p][x]) where the row shows x
        w = share.sum(axis=(1, 2))                                                # [R]
        F = (onehot * w[:, None, None]).sum(axis=0)
        F = F / F.sum(axis=1, keepdims=True)                                      # rows with m = 0: nan, unused
        E = np.exp(lam * sub)
        G = P[None, :] * (np.nan_to_num(F)[:, inA] @ E[inA, :])
        alpha = np.minimum(nbar, m) - 1.0
        Q = (alpha[:, None] * np.nan_to_num(F) + beta * G) / (alpha + beta)[:, None]
        V = np.log(Q / P[None, :]) / lam
    have = (m >= 1)[:, None] & inA[None, :]
    values = np.where(have, V, 0.0)
    rounded = np.sign(values) * np.floor(np.abs(values) + 0.5)
    pssm = sub[query].copy()
    pssm[:, 0] = 0
    pssm = np.where(have, np.clip(rounded, -128, 127), pssm).astype(np.int8)
    info = {"lambda": lam, "n_distinct": nbar, "n_rows": 1 + sum(a["score"] > 0 for a in alignments),
            "n_observed": int(((X[1:] > 0).sum(axis=0) > 0).sum()),
            "n_clamped": int((have & ((rounded < -128) | (rounded > 127))).sum())}
    return {"pssm": pssm, "values": values, "m": m, "k": k, "info": info, "have": have}


def half_integer_margin(values, have):
    """The least distance of a value from a half-integer (where rounding could go either way)."""
    v = values[have]
    return float(np.abs((v - 0.5) - np.rint(v - 0.5)).min()) if v.size else 1.0


# ---- generators ------------------------------------------------------------------------------------------------------
STD_IDX = np.array([idx(c) for c in STANDARD], dtype=np.int8)


def random_seq(rng, n):
    p = builtin_freq()[STD_IDX.astype(np.int64)]
    return rng.choice(STD_IDX, size=n, p=p / p.sum()).astype(np.int8)


def relative(rng, q, subst, keep=(), ins=(), dele=(), lo=0, hi=None, flank=0, odd=None):
    """A relative of q: columns [lo, hi) with point substitutions at rate subst (never in `keep`), then runs deleted
    (dele: (column, length), so the path has a run of 'D') and inserted (ins: (column, length), a run of 'I'), random
    flanks of `flank` residues on both sides; odd: {column: residue index} forced afterwards (X, B, Z, '*')."""
    hi = len(q) if hi is None else hi
    s = q.copy()
    for p in range(lo, hi):
        if p not in keep and rng.random() < subst:
            s[p] = random_seq(rng, 1)[0]
    for p, r in (odd or {}).items():
        s[p] = r
    parts, at = [], lo
    events = sorted([(p, "d", n) for p, n in dele] + [(p, "i", n) for p, n in ins])
    for p, kind, n in events:
        parts.append(s[at:p])
        if kind == "d":
            at = p + n
        else:
            parts.append(random_seq(rng, n))
            at = p
    parts.append(s[at:hi])
    return np.concatenate([random_seq(rng, flank)] + parts + [random_seq(rng, flank)]).astype(np.int8)


def pack(seqs):
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return np.concatenate(seqs).astype(np.int8), off


def align(orc, q, flat, off, indices, sub, gaps):
    """The oracle's alignments of q against the listed sequences, shaped like Context.align_hits' dicts."""
    out = []
    for i in indices:
        d = flat[int(off[i]):int(off[i + 1])]
        score, (qb, qe, db_, de), ops = orc.pair_trace(q, d, sub, *gaps)
        out.append({"score": score, "index": int(i), "q_begin": qb, "q_end": qe, "d_begin": db_, "d_end": de,
                    "n_ops": len(ops), "ops": ops})
    return out


def family(seed, lq, n_hits, n_random=0, subst=(0.1, 0.6), gapped=0, partial=0, flank=5, keep=()):
    """A query of lq residues and a database of n_hits relatives (the first `gapped` of them with a deleted and an
    inserted run, the next `partial` covering the middle third only) followed by n_random unrelated sequences of 20 to
    300 residues -> (q, flat, off, hit indices)."""
    rng = np.random.default_rng(seed)
    q = random_seq(rng, lq)
    seqs = []
    for h in range(n_hits):
        rate = subst[0] + (subst[1] - subst[0]) * (h / max(n_hits - 1, 1))
        if h < gapped and lq >= 30:
            seqs.append(relative(rng, q, min(rate, 0.25), keep, ins=[(lq // 3, 3)], dele=[(2 * lq // 3, 2)], flank=flank))
        elif h < gapped + partial and lq >= 9:
            seqs.append(relative(rng, q, min(rate, 0.3), keep, lo=lq // 3, hi=2 * lq // 3, flank=flank))
        else:
            seqs.append(relative(rng, q, rate, keep, flank=flank))
    seqs += [random_seq(rng, int(rng.integers(20, 301))) for _ in range(n_random)]
    flat, off = pack(seqs)
    return q, flat, off, list(range(n_hits))


def host_cases(orc):
    """name -> dict(sub, gaps, q, flat, off, al, freq, beta): every case of the host tests, alignments by the oracle."""
    b62, gaps = table("BLOSUM62"), MATRICES["BLOSUM62"]
    cases = {}

    def add(name, q, flat, off, hits, sub=b62, g=gaps, freq=None, beta=10.0):
        cases[name] = dict(sub=sub, gaps=g, q=q, flat=flat, off=off, al=align(orc, q, flat, off, hits, sub, g), freq=freq, beta=beta)

    for name, g in MATRICES.items():                                   # no hits: the matrix's own rows
        q, flat, off, _ = family(11, 40, 1)
        add("nohits_" + name, q, flat, off, [], sub=table(name), g=g)
    q = np.array([idx("W")], dtype=np.int8)                            # lq 1
    flat, off = pack([np.array([idx(c) for c in s], dtype=np.int8) for s in ("AWA", "GGWG", "W", "KYK")])
    add("lq1", q, flat, off, [0, 1, 2, 3])
    add("partial", *family(12, 90, 6, partial=6))
    q, flat, off, hits = family(13, 120, 24, gapped=8, flank=8)
    add("gaps", q, flat, off, hits)
    rng = np.random.default_rng(14)                                    # hits with X, B, Z and '*'
    q = random_seq(rng, 60)
    odd = [idx(c) for c in "XBZ*"]
    seqs = [relative(rng, q, 0.15, odd={int(p): odd[(h + j) % 4] for j, p in enumerate(rng.choice(60, 5, replace=False))}) for h in range(10)]
    add("odd_residues", q, *pack(seqs), list(range(10)))
    rng = np.random.default_rng(15)                                    # a query with X: columns without any residue of A
    q = random_seq(rng, 50)
    q[[0, 1, 20]] = idx("X")
    seqs = [relative(rng, q, 0.1, lo=2, odd={20: idx("X")}) for _ in range(5)]
    add("query_x", q, *pack(seqs), list(range(5)))
    q, flat, off, hits = family(16, 70, 5)
    add("duplicate", q, flat, off, [0, 1, 2, 1, 1])
    rng = np.random.default_rng(17)                                    # a hit of score 0: tryptophans against a query without W, Y, F
    q = random_seq(rng, 40)
    q[np.isin(q, [idx("W"), idx("Y"), idx("F"), idx("H")])] = idx("A")
    seqs = [relative(rng, q, 0.2), np.full(6, idx("W"), dtype=np.int8), relative(rng, q, 0.3)]
    add("score0", q, *pack(seqs), [0, 1, 2])
    rng = np.random.default_rng(18)                                    # clamping: a residue the background all but excludes
    q = random_seq(rng, 40)
    q[[5, 17]] = idx("W")
    freq = builtin_freq()
    freq[idx("W")] = 1e-60
    seqs = [relative(rng, q, 0.3, keep=(5, 17)) for _ in range(12)]
    add("clamp", q, *pack(seqs), list(range(12)), freq=freq)
    for n in (1, 24, 300):                                             # families of 1 to 300 hits of a 120-column query
        q, flat, off, hits = family(100 + n, 120, n, gapped=min(n // 3, 8))
        add("family_%d" % n, q, flat, off, hits)
    q, flat, off, hits = family(19, 64, 12, subst=(0.2, 0.5))
    add("pam250", q, flat, off, hits, sub=table("PAM250"), g=MATRICES["PAM250"], beta=5.5)
    return cases


# ---- the end-to-end fixture --------------------------------------------------------------------------------------------
E2E = dict(seed=2024, lq=100, n_random=400, n_family=30, include_score=60, top=30)


def e2e_database():
    """400 random sequences and 30 members of a family at graded divergence (15 of the 100 columns conserved, the
    others substituted at 30 to 100 percent), shuffled together -> (query: one more member at 30 percent, flat, off,
    is_family)."""
    rng = np.random.default_rng(E2E["seed"])
    lq = E2E["lq"]
    ancestor = random_seq(rng, lq)
    keep = set(int(p) for p in rng.choice(lq, 15, replace=False))
    members = [relative(rng, ancestor, 0.3 + 0.7 * h / (E2E["n_family"] - 1), keep, flank=int(rng.integers(0, 30))) for h in range(E2E["n_family"])]
    others = [random_seq(rng, int(rng.integers(20, 301))) for _ in range(E2E["n_random"])]
    seqs = members + others
    order = rng.permutation(len(seqs))
    flat, off = pack([seqs[i] for i in order])
    is_family = order < E2E["n_family"]
    query = relative(rng, ancestor, 0.3, keep)
    return query, flat, off, is_family


def family_in_top(scores, is_family, top):
    """Family members among the `top` best (higher score first, ties by lower index)."""
    order = np.lexsort((np.arange(len(scores)), -np.asarray(scores, dtype=np.int64)))
    return int(is_family[order[:top]].sum())
