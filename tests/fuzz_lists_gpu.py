#!/usr/bin/env python3
"""Randomised parity soak of swg_search_lists (every query of a batch against its own candidate list): batch sizes
from {1, 3, 255, 257}, lists of 0 .. 300 entries with duplicates and overlap between the queries' lists, random query
lengths (some beyond one pass: the batch then goes one list after another), tables, gap scores, cell forms (option f16
0 / 1), now and then a forced batch geometry (option batch_geometry = 1 with cols_per_wave and group_lanes, drawn as
tests/fuzz_multi_gpu.py draws it), with and without the score array.  Every score against the int32 oracle at every
entry, every hit list against the oracle's order over the list's distinct entries.  Stops at the first mismatch or error.
usage: python tests/fuzz_lists_gpu.py [seconds] [seed]"""
import sys, time, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import swg_loader
from fuzz_multi_gpu import forced_geometry


def main(budget=60.0, seed=1):
    swg = swg_loader.load(); orc = swg_loader.oracle()
    rng = np.random.default_rng(seed)
    grng = np.random.default_rng([seed, 0xBA7C])     # the forced geometries' own stream: the other draws stay what they were
    ctx = swg.Context(0)
    ctx.set_option("autotune", 0)
    mats = ["BLOSUM62", "PAM250", "BLOSUM45"]
    t_end = time.time() + budget
    cases, routes, forms, sizes = 0, {}, {}, {}
    while time.time() < t_end:
        n = int(rng.integers(1, 700))
        shape = rng.integers(0, 3)
        if shape == 0:   lens = rng.integers(1, 60, size=n)
        elif shape == 1: lens = rng.integers(1, 400, size=n)
        else:            lens = np.concatenate([rng.integers(600, 1500, size=min(n, 2)), rng.integers(1, 150, size=max(0, n - 2))])
        lens = [int(v) for v in lens]
        nq = int(rng.choice([1, 3, 255, 257], p=[.3, .4, .15, .15]))
        if nq > 200:
            qlens = [int(rng.choice([1, 5, 33, 64, 90])) for _ in range(nq)]
        elif rng.random() < 0.15:
            qlens = [int(rng.choice([5, 64, 300, 2300])) for _ in range(nq)]        # some need several passes
        else:
            base = int(rng.choice([1, 7, 33, 128, 200, 367, 500]))
            qlens = [max(1, int(base * rng.uniform(0.3, 1.2))) for _ in range(nq)]
        sc = swg.load_scoring(str(rng.choice(mats)))
        go, ge = [(-2, -1), (-10, -1), (0, -1), (-3, 0), (-11, -2), (1, -3)][int(rng.integers(0, 6))]
        seqs = [swg.synth_query(int(rng.integers(1, 1 << 30)), L) for L in lens]
        queries = [swg.synth_query(int(rng.integers(1, 1 << 30)), L) for L in qlens]
        if rng.random() < 0.3:     # relatives: a query copied into a few sequences (some scores beyond 4096)
            for _ in range(int(rng.integers(1, 4))):
                qi, si = int(rng.integers(0, nq)), int(rng.integers(0, n))
                m = min(len(queries[qi]), len(seqs[si]))
                seqs[si][:m] = queries[qi][:m]
        pool = rng.choice(n, size=max(1, n // int(rng.choice([1, 2, 10]))), replace=False)   # overlap: lists drawn from one pool
        lists = []
        for _ in range(nq):
            size = int(rng.integers(0, 301)) if nq < 200 else int(rng.integers(0, 40))
            l = rng.choice(pool, size=size, replace=True) if size else np.zeros(0, dtype=np.int64)
            lists.append(l)
        if sum(qlens[i] * sum(lens[j] for j in set(int(v) for v in lists[i])) for i in range(nq)) > 2e9:
            continue
        tab = sc.table()
        flat = np.concatenate(seqs); off = np.zeros(n + 1, dtype=np.uint64); off[1:] = np.cumsum(lens)
        ctx.set_scoring(tab, go, ge)
        f16 = int(rng.choice([0, 1]))
        ctx.set_option("f16", f16)
        geom = forced_geometry(grng, max(qlens)) if grng.random() < 0.2 else None
        ctx.set_option("batch_geometry", 1 if geom else 0)
        ctx.set_option("cols_per_wave", geom[0] if geom else 0)
        ctx.set_option("group_lanes", geom[1] if geom else 0)
        db = swg.Database(flat, off).upload(ctx)
        k = int(rng.choice([0, 1, 4, 30, 400]))
        want_scores = bool(rng.random() < 0.6) or k == 0
        got, hits, st = ctx.search_lists(db, queries, lists, k=k, want_scores=want_scores, fill=-7)
        for i, q in enumerate(queries):
            l = np.asarray(lists[i], dtype=np.int64)
            if len(l) == 0:
                ok = (not want_scores or got[i].size == 0) and hits[i] == []
                want = None
            else:
                want = orc.score_db(q, flat, off, tab, go, ge)
                sel = np.unique(l)
                exp = [(-s, j) for s, j in sorted((-int(want[j]), int(j)) for j in sel)[:k]]
                ok = (not want_scores or np.array_equal(got[i], want[l])) and hits[i] == exp
            if not ok:
                print("MISMATCH case", cases, "query", i, "of", nq, "lq", len(q), "n", n, "list", len(l), "gaps", go, ge, "f16", f16,
                      "geometry", geom, "k", k, "scores asked", want_scores, "stats", st)
                return 1
        db.close()
        cases += 1
        route = "launch" if st["fill_launches"] else "one_by_one"
        routes[route] = routes.get(route, 0) + 1
        forms[int(st["cell_form"])] = forms.get(int(st["cell_form"]), 0) + 1
        sizes[nq] = sizes.get(nq, 0) + 1
        if cases % 20 == 0:
            print("cases", cases, "last: nq", nq, "qlens", qlens[:4], "n", n, "k", k, "scores", want_scores, "launches", st["fill_launches"],
                  "form", st["cell_form"], "K", st["cols_per_wave"], "G", st["group_lanes"], flush=True)
    print("OK", cases, "cases; by route", dict(sorted(routes.items())), "by cell form", dict(sorted(forms.items())), "by batch size",
          dict(sorted(sizes.items())))
    return 0


if __name__ == "__main__":
    sys.exit(main(float(sys.argv[1]) if len(sys.argv) > 1 else 60.0, int(sys.argv[2]) if len(sys.argv) > 2 else 1))
