"""swg_search_lists beside the only other route to the same answers: per query a view of its list, swg_set_query,
swg_search, swg_db_free.

Config 2's database (100 000 sequences, PAM250).  Shapes: 64 queries of 128 aa x 500 candidates, 256 queries of 367 aa x
1 000 candidates, 8 queries x 20 000 candidates, and a skewed set (one list of 20 000, 63 lists of 50).  In ONE process the
two routes alternate (ROUNDS times each, the order swapped every round); a route's time is the wall time of the whole
batch, hits (k = 10) included.  Reported: the median and the spread of the rounds, and the GCUPS of each route from the
batch's real cells.  The hits of both routes are compared.  With SWG_LISTS_EQUAL_SHARES set in the environment the one
launch deals its workgroups one share per row instead of by work: run the tool a second time that way to see what the
dealing is worth on the skewed shape.

    python tools/sweeps/lists_vs_views.py [out.txt]      (GPU box)
"""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import swg_loader  # noqa: E402

ROUNDS, N, SEED, K = 7, 100000, 0x5EED0002, 10


def ms(f):
    t0 = time.perf_counter()
    r = f()
    return (time.perf_counter() - t0) * 1e3, r


def main():
    swg = swg_loader.load()
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()

    sc = swg.load_scoring("PAM250")
    flat, off = swg.synth_db(SEED, N)
    lens = np.diff(off.astype(np.int64))
    ctx = swg.Context(0)
    ctx.set_scoring(sc, -2, -1)
    ctx.set_option("autotune", 0)
    db = swg.Database(flat, off).upload(ctx)
    rng = np.random.default_rng(2)
    shapes = [("64 x 128 aa x 500", [128] * 64, [500] * 64), ("256 x 367 aa x 1000", [367] * 256, [1000] * 256),
              ("8 x 367 aa x 20000", [367] * 8, [20000] * 8), ("skewed: 1 x 20000 + 63 x 50 (367 aa)", [367] * 64, [20000] + [50] * 63)]
    say("config 2's database: %d sequences, %d residues; k = %d; %d alternating rounds; workgroups dealt %s" % (
        N, len(flat), K, ROUNDS, "one share per row" if os.environ.get("SWG_LISTS_EQUAL_SHARES") else "by work"))

    def views(qs, lists):
        hits = []
        for q, l in zip(qs, lists):
            v = db.view(ctx, l)
            ctx.set_query(q)
            hits.append(ctx.search(v, want_scores=False, k=K)[1])
            v.close()
        return hits

    for label, qlens, sizes in shapes:
        qs = [swg.synth_query(SEED + 17 * i, lq) for i, lq in enumerate(qlens)]
        lists = [rng.choice(N, size=s, replace=False) for s in sizes]
        cells = sum(lq * int(lens[l].sum()) for lq, l in zip(qlens, lists))
        views(qs[:2], lists[:2])                                            # warm both routes once
        ctx.search_lists(db, qs, lists, k=K, want_scores=False)
        t = {"views": [], "lists": []}
        fill = []
        for rnd in range(ROUNDS):
            for route in (("views", "lists") if rnd % 2 == 0 else ("lists", "views")):
                if route == "views":
                    dt, h_v = ms(lambda: views(qs, lists))
                else:
                    dt, (_, h_l, st) = ms(lambda: ctx.search_lists(db, qs, lists, k=K, want_scores=False))
                    fill.append(st["fill_ms"])
                t[route].append(dt)
            assert h_v == h_l, label
        med = statistics.median
        say("%-40s cells %.3e  launches %d  K %d G %d W %d workgroups %d form %d" % (label, cells, st["fill_launches"], st["cols_per_wave"],
                                                                               st["group_lanes"], st["waves"], st["workgroups"], st["cell_form"]))
        for route in ("views", "lists"):
            say("    %-6s median %9.2f ms  [%9.2f .. %9.2f]  %8.1f GCUPS" % (route, med(t[route]), min(t[route]), max(t[route]),
                                                                            cells / med(t[route]) / 1e6))
        say("    lists, the fill alone: median %.2f ms [%.2f .. %.2f]  %.1f GCUPS; views / lists = %.1f x" % (
            med(fill), min(fill), max(fill), cells / med(fill) / 1e6, med(t["views"]) / med(t["lists"])))
    db.close()
    ctx.close()


if __name__ == "__main__":
    main()
