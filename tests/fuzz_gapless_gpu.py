#!/usr/bin/env python3
"""Randomised parity soak of the gapless search (swg_search_gapless and its batch forms): random database shapes, query
lengths (some beyond one pass: route 0), tables from BLOSUM-like to the ends of int8 with planted copies of the query
(scores on either side of 4096, 32767 and 65535), forced and free geometries, options f16 / engine / wide16 / batch /
workgroups, index and PSSM queries, with and without the score array.  Every score against the oracle with the gaps
priced out at every index, every hit list against its order.  Stops at the first mismatch or error.
usage: python tests/fuzz_gapless_gpu.py [seconds] [seed]"""
import sys, time, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import swg_loader
import gapless_cases as gc
import scoring_edges as se


def main(budget=60.0, seed=1):
    swg = swg_loader.load(); orc = swg_loader.oracle()
    rng = np.random.default_rng(seed)
    ctx = swg.Context(0)
    ctx.set_option("autotune", 0)
    mats = ["BLOSUM62", "PAM250", "BLOSUM45"]
    t_end = time.time() + budget
    cases, forms = 0, {}
    while time.time() < t_end:
        n = int(rng.integers(1, 1500))
        shape = rng.integers(0, 3)
        if shape == 0:   lens = rng.integers(1, 60, size=n)
        elif shape == 1: lens = rng.integers(1, 400, size=n)
        else:            lens = np.concatenate([rng.integers(600, 1500, size=min(n, 2)), rng.integers(1, 150, size=max(0, n - 2))])
        lq = int(rng.choice([1, 7, 33, 128, 200, 367, 500, 600, 2048, 2300])) if rng.random() < 0.5 else int(rng.integers(1, 600))
        if lq * int(lens.sum()) > 3e8:
            continue
        t = int(rng.integers(0, 4))
        sub = (swg.load_scoring(str(rng.choice(mats))).table() if t == 0 else se.diag127(rng, zero0=True) if t == 1
               else se.full_range(rng) if t == 2 else se.all_127())
        sub = np.array(sub, dtype=np.int8).reshape(32, 32)
        q = rng.integers(1, 27, size=lq).astype(np.int8)
        seqs = [rng.integers(1, 27, size=int(L)).astype(np.int8) for L in lens]
        for _ in range(int(rng.integers(0, 6))):          # planted copies of a stretch of the query
            si = int(rng.integers(0, n))
            m = int(rng.integers(1, min(lq, len(seqs[si])) + 1))
            a = int(rng.integers(0, lq - m + 1)); b = int(rng.integers(0, len(seqs[si]) - m + 1))
            seqs[si][b:b + m] = q[a:a + m]
        flat, off = gc.pack(seqs)
        for key, vals in (("f16", [1, 1, 1, 0]), ("engine", [0, 0, 0, 2, 1]), ("wide16", [1, 1, 0]), ("batch", [8, 1]),
                          ("workgroups", [0, 0, 3]), ("group_lanes", [0, 0, 16, 32, 64])):
            ctx.set_option(key, int(rng.choice(vals)))
        ctx.set_option("cols_per_wave", int(rng.integers(2, 33)) if rng.random() < 0.3 else 0)
        ctx.set_scoring(sub, int(rng.integers(-40, 1)), int(rng.integers(-5, 1)))
        pssm = rng.random() < 0.25
        if pssm:
            ctx.set_query_pssm(sub[q.astype(np.int64)])
        else:
            ctx.set_query(q)
        truth = gc.oracle_gapless(orc, q, flat, off, sub)
        db = swg.Database(flat, off).upload(ctx)
        k = int(rng.choice([0, 1, 4, 30, 2000]))
        ws = bool(rng.random() < 0.7) or k == 0
        try:
            scores, hits, st = ctx.search_gapless(db, want_scores=ws, k=k)
        except RuntimeError as e:
            if "no diagonal-engine geometry" in str(e) or "geometry" in str(e):   # (a forced geometry the engine does not have)
                db.close()
                continue
            raise
        if ws and not np.array_equal(scores, truth):
            bad = np.nonzero(scores != truth)[0]
            print("MISMATCH seed", seed, "case", cases, "n", n, "lq", lq, "table", t, st, bad[:8], scores[bad[:8]], truth[bad[:8]])
            return 1
        if hits != gc.expected_hits(truth, k):
            print("HITS differ seed", seed, "case", cases, st)
            return 1
        forms[st["cell_form"]] = forms.get(st["cell_form"], 0) + 1
        cases += 1
        db.close()
    print("ok: %d cases, cell forms %s" % (cases, forms))
    return 0


if __name__ == "__main__":
    sys.exit(main(float(sys.argv[1]) if len(sys.argv) > 1 else 60.0, int(sys.argv[2]) if len(sys.argv) > 2 else 1))
