#!/usr/bin/env python3
"""Randomised soak of swg_align_bounds_multi / _multi_pssm (alignment coordinates without the traceback): batches of 1 ..
12 queries of 1 .. 1100 columns (some beyond the kernel's 1024: the fallback), rows of 0 .. 40 hits with repeats, over
full and four-letter alphabets (ties), relatives of the queries planted, nine gap settings of every sign, option
bounds_groups 0 / 1 / 3, index queries and PSSMs; one batch in about thirty is instead one or two short queries against
a sequence of 2^19 .. 2^20 + 1 residues (the row half of the kernel's packed positions up to its sign bit, and the
hand-over to the fallback at 2^20 residues) with each query planted at a random row or in the last rows.  Every field
of every result against align_hits_multi(want_ops=False) on the same context, and for index queries against the int32
oracle's traceback.  Stops at the first mismatch or error.
usage: python tests/fuzz_bounds_gpu.py [seconds] [seed]"""
import sys, time, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import swg_loader

GAPS = [(-11, -1), (-2, -1), (0, -1), (0, 0), (-1, 0), (1, -3), (-3, 1), (2, 1), (0, 1)]
FIELDS = ("score", "index", "q_begin", "q_end", "d_begin", "d_end", "n_ops")
HALF, LEN_LIMIT = 1 << 19, 1 << 20        # rows from HALF on set a packed position's bit 31; LEN_LIMIT = SWG_BOUNDS_LEN


def main(budget=60.0, seed=1):
    swg = swg_loader.load(); orc = swg_loader.oracle()
    rng = np.random.default_rng(seed)
    ctx = swg.Context(0)
    ctx.set_option("autotune", 0)
    mats = ["BLOSUM62", "PAM250", "BLOSUM45"]
    t_end = time.time() + budget
    cases = pairs = fallback = 0
    while time.time() < t_end:
        letters = np.array([1, 3, 4, 5], dtype=np.int8) if rng.random() < 0.4 else np.arange(1, 26, dtype=np.int8)
        letters = letters[~np.isin(letters, (2, 10, 15, 21))] if len(letters) > 4 else letters     # B J O U: not in the tables
        n = int(rng.integers(1, 80))
        nq = int(rng.integers(1, 13))
        qlens = [int(rng.choice([1, 2, 7, 33, 64, 65, 128, 129, 300, 512, 513, 1024, 1025, 1100])) if rng.random() < 0.5
                 else int(rng.integers(1, 400)) for _ in range(nq)]
        queries = [letters[rng.integers(0, len(letters), size=L)] for L in qlens]
        seqs = [letters[rng.integers(0, len(letters), size=int(rng.integers(1, 500)))] for _ in range(n)]
        long_rows = rng.random() < 1.0 / 30
        if long_rows:                                 # one long sequence, short queries, a stretch of each somewhere in it
            n, nq = int(rng.integers(1, 4)), int(rng.integers(1, 3))
            qlens = [int(rng.choice([1, 8, 60, 65, 129])) for _ in range(nq)]
            queries = [letters[rng.integers(0, len(letters), size=L)] for L in qlens]
            seqs = [letters[rng.integers(0, len(letters), size=int(rng.integers(1, 500)))] for _ in range(n)]
            L = int(rng.choice([HALF, LEN_LIMIT - 1, LEN_LIMIT, LEN_LIMIT + 1])) if rng.random() < 0.5 else int(rng.integers(HALF, LEN_LIMIT + 2))
            seqs[0] = letters[rng.integers(0, len(letters), size=L)]
            for q in queries:
                at = int(rng.integers(0, L - len(q) + 1)) if rng.random() < 0.5 else L - len(q)
                seqs[0][at:at + len(q)] = q
        for _ in range(0 if long_rows else int(rng.integers(0, 6))):      # relatives: a stretch of a query inside a sequence
            qi, si = int(rng.integers(0, nq)), int(rng.integers(0, n))
            a = int(rng.integers(0, qlens[qi])); b = int(rng.integers(a + 1, qlens[qi] + 1))
            seqs[si] = np.concatenate([seqs[si][:int(rng.integers(0, 20))], queries[qi][a:b], seqs[si][:int(rng.integers(0, 20))]])
        lens = [len(s) for s in seqs]
        flat = np.concatenate(seqs).astype(np.int8); off = np.zeros(n + 1, dtype=np.uint64); off[1:] = np.cumsum(lens)
        hits = [[(0, int(i)) for i in rng.integers(0, n, size=int(rng.integers(0, 41)))] for _ in range(nq)]
        if long_rows:
            hits = [[(0, int(i)) for i in rng.permutation(n)] for _ in range(nq)]
        go, ge = GAPS[int(rng.integers(0, len(GAPS)))]
        tab = swg.load_scoring(str(rng.choice(mats))).table()
        groups = int(rng.choice([0, 1, 3]))
        pssm = rng.random() < 0.3
        ctx.set_scoring(tab, go, ge)
        ctx.set_option("bounds_groups", groups)
        db = swg.Database(flat, off).upload(ctx)
        what = dict(case=cases, seed=seed, nq=nq, qlens=qlens, n=n, gaps=(go, ge), groups=groups, pssm=pssm, longest=max(lens))
        try:
            if pssm:
                ps = [np.clip(tab[q.astype(np.int64)].astype(np.int64) + rng.integers(-3, 4, size=(len(q), 32)), -128, 127).astype(np.int8)
                      for q in queries]
                got = ctx.align_bounds_multi_pssm(db, ps, hits)
                want = ctx.align_hits_multi_pssm(db, ps, hits, want_ops=False)
            else:
                got = ctx.align_bounds_multi(db, queries, hits)
                want = ctx.align_hits_multi(db, queries, hits, want_ops=False)
            last = ctx.debug_bounds_last()
        except swg.SwgError as e:
            print("ERROR", e, what); return 1
        if got != want:
            bad = next((i, j) for i in range(nq) for j in range(len(hits[i])) if got[i][j] != want[i][j])
            print("MISMATCH against align_hits_multi", what, bad, got[bad[0]][bad[1]], want[bad[0]][bad[1]]); return 1
        if not pssm:
            for q, row in zip(queries, got):
                for a in row[:6]:
                    d = flat[int(off[a["index"]]):int(off[a["index"] + 1])]
                    sc, co, ops = orc.pair_trace(q, d, tab, go, ge)
                    if tuple(a[f] for f in FIELDS) != (sc, a["index"], co[0], co[1], co[2], co[3], len(ops)):
                        print("MISMATCH against the oracle", what, a, sc, co, len(ops)); return 1
        want_fb = sum(1 for r, L in zip(hits, qlens) for _, i in r if L > last["column_limit"] or lens[i] >= LEN_LIMIT)
        if last["fallback_pairs"] != want_fb or last["kernel_pairs"] != sum(len(r) for r in hits) - want_fb:
            print("ROUTE", what, last); return 1
        cases += 1; pairs += last["kernel_pairs"]; fallback += last["fallback_pairs"]
        db.close()
    ctx.set_option("bounds_groups", 0)
    print("ok: %d batches, %d pairs on the bounds kernel, %d on the fallback, seed %d" % (cases, pairs, fallback, seed))
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(float(sys.argv[1]) if len(sys.argv) > 1 else 60.0, int(sys.argv[2]) if len(sys.argv) > 2 else 1))
