"""The headline with and without the fifth pruning level (profiles/prune_adjacent_ab.txt, section 2).

    python tools/sweeps/prune_adjacent_ab.py [--nseq N] [--reps R] [--auto-only]

The protocol of tools/sweeps/prune_gate_ab.py: config 4's whole database (10M sequences, one shard), its 3000-column
query and scoring through the Python wrapper, autotune off, ctx.search(db, want_scores=False, k=100), one search in
flight.  For prune_refine5 = 1 (off), 5256 (forced) and 0 (automatic), everything else automatic: R searches with the
tables resident, then two searches each behind a set_query of the same query (a new epoch: the search pays its tables
again; wall_ms is the host clock around the whole search).  One JSON line per search.  --auto-only sets no pruning option
at all, so the script also runs on a library without the level (the parent of an A/B; SWG_ROOT names its built
checkout)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.environ.get("SWG_ROOT") or os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import swg_loader  # noqa: E402

swg = swg_loader.load()

CANDIDATES = [("fifth off", {"prune_refine5": 1}), ("fifth forced", {"prune_refine5": 5256}), ("auto", {"prune_refine5": 0})]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nseq", type=int, default=10000000)
    ap.add_argument("--lq", type=int, default=3000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--auto-only", action="store_true", help="the library's defaults only: no pruning option is set")
    a = ap.parse_args()
    seed = 0x5EED0004
    q = swg.synth_query(seed, a.lq)
    sh = swg.synth_db_shard(seed, a.nseq, 0, 1, query=None, fraction=0.0, subst=0.05)
    ctx = swg.Context(0)
    ctx.set_scoring(swg.load_scoring("BLOSUM62"), -2, -1)
    ctx.set_query(q)
    ctx.set_option("autotune", 0)
    db = swg.Database(sh["flat"], sh["offsets"], index=sh["index"], n_total=a.nseq).upload(ctx)
    want = None
    for name, options in ([("defaults", {})] if a.auto_only else CANDIDATES):
        for key, value in options.items():
            ctx.set_option(key, value)
        for rep in range(a.reps + 2):
            fresh = rep >= a.reps
            if fresh:
                ctx.set_query(q)
            t0 = time.perf_counter()
            _, hits, st = ctx.search(db, want_scores=False, k=100)
            wall = (time.perf_counter() - t0) * 1e3
            info = ctx.prune_last()
            fifth = ctx.debug_prune_tables5() if hasattr(ctx, "debug_prune_tables5") else None
            if want is None:
                want = hits
            print(json.dumps({"candidate": name, **options, "fresh_query": fresh, "rep": rep, "fourth": ctx.debug_prune_tables4()["refine4"],
                              "fifth": fifth, "wall_ms": round(wall, 2), "fill_ms": st["fill_ms"], "total_ms": st["total_ms"], "info": info,
                              "rows_kept_frac": round(1.0 - info["pair_rows_skipped"] / max(1, info["pair_rows"]), 5),
                              "hits_equal_first": hits == want}), flush=True)
    db.close()


if __name__ == "__main__":
    main()
