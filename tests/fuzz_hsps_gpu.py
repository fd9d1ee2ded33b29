#!/usr/bin/env python3
"""Randomised soak of swg_align_hsps_multi / _multi_pssm (several non-overlapping alignments per hit): batches of 1 .. 8
queries of 1 .. 1800 columns (both sides of the 256-lane stride and of the LDS limit), rows of 0 .. 12 hits with repeats,
over full and four-letter alphabets (ties, crossings), repeats and pieces of the queries planted out of order, nine gap
settings of every sign, max_hsps 1 .. 9, index queries and PSSMs.  The number of alignments, every field, every path and
every count against the host twin swg_align_hsps_host, pair by pair.  Stops at the first mismatch or error.
usage: python tests/fuzz_hsps_gpu.py [seconds] [seed]"""
import sys, time, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import swg_loader

GAPS = [(-11, -1), (-2, -1), (0, -1), (0, 0), (-1, 0), (1, -3), (-3, 1), (2, 1), (0, 1)]


def main(budget=60.0, seed=1):
    swg = swg_loader.load()
    rng = np.random.default_rng(seed)
    ctx = swg.Context(0)
    ctx.set_option("autotune", 0)
    mats = ["BLOSUM62", "PAM250", "BLOSUM45"]
    t_end = time.time() + budget
    cases = pairs = found = 0
    while time.time() < t_end:
        letters = np.array([1, 3, 4, 5], dtype=np.int8) if rng.random() < 0.4 else np.arange(1, 26, dtype=np.int8)
        letters = letters[~np.isin(letters, (2, 10, 15, 21))] if len(letters) > 4 else letters     # B J O U: not in the tables
        n = int(rng.integers(1, 30))
        nq = int(rng.integers(1, 9))
        qlens = [int(rng.choice([1, 2, 7, 64, 255, 256, 257, 512, 513, 1700, 1701, 1800])) if rng.random() < 0.4
                 else int(rng.integers(1, 300)) for _ in range(nq)]
        queries = [letters[rng.integers(0, len(letters), size=L)] for L in qlens]
        seqs = [letters[rng.integers(0, len(letters), size=int(rng.integers(1, 200)))] for _ in range(n)]
        for _ in range(int(rng.integers(0, 12))):      # relatives: stretches of a query inside a sequence, in any order
            qi, si = int(rng.integers(0, nq)), int(rng.integers(0, n))
            a = int(rng.integers(0, qlens[qi])); b = int(rng.integers(a + 1, min(qlens[qi], a + 60) + 1))
            at = int(rng.integers(0, len(seqs[si]) + 1))
            seqs[si] = np.concatenate([seqs[si][:at], queries[qi][a:b], seqs[si][at:]])
        lens = [len(s) for s in seqs]
        flat = np.concatenate(seqs).astype(np.int8); off = np.zeros(n + 1, dtype=np.uint64); off[1:] = np.cumsum(lens)
        hits = [[(0, int(i)) for i in rng.integers(0, n, size=int(rng.integers(0, 13)))] for _ in range(nq)]
        go, ge = GAPS[int(rng.integers(0, len(GAPS)))]
        tab = swg.load_scoring(str(rng.choice(mats))).table()
        H, ms = int(rng.integers(1, 10)), int(rng.choice([1, 9, 25, 60]))
        pssm = rng.random() < 0.3
        ctx.set_scoring(tab, go, ge)
        db = swg.Database(flat, off).upload(ctx)
        what = dict(case=cases, seed=seed, nq=nq, qlens=qlens, n=n, gaps=(go, ge), max_hsps=H, min_score=ms, pssm=pssm)
        try:
            if pssm:
                ps = [np.clip(tab[q.astype(np.int64)].astype(np.int64) + rng.integers(-3, 4, size=(len(q), 32)), -128, 127).astype(np.int8)
                      for q in queries]
                got = ctx.align_hsps_multi_pssm(db, ps, hits, H, ms, want_counts=True)
            else:
                got = ctx.align_hsps_multi(db, queries, hits, H, ms, want_counts=True)
        except swg.SwgError as e:
            print("ERROR", e, what); return 1
        for i, row in enumerate(hits):
            for j, (_, index) in enumerate(row):
                kw = dict(pssm=ps[i]) if pssm else dict(query=queries[i])
                want = swg.align_hsps_host(None if pssm else tab, go, ge, seqs[index], H, ms, want_counts=True, **kw)
                if got[i][j] != [dict(a, index=index) for a in want]:
                    print("MISMATCH against the host twin", what, (i, j), got[i][j], want); return 1
                pairs += 1; found += len(want)
        cases += 1
        db.close()
    print("ok: %d batches, %d pairs, %d alignments, seed %d" % (cases, pairs, found, seed))
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(float(sys.argv[1]) if len(sys.argv) > 1 else 60.0, int(sys.argv[2]) if len(sys.argv) > 2 else 1))
