"""The headline with and without the gate in front of the first pruning level (profiles/prune_gate_ab.txt, section 2).

    python tools/sweeps/prune_gate_ab.py [--nseq N] [--reps R] [--auto-only] [--count-gate]

The protocol of tools/sweeps/prune_deep_ab.py: config 4's whole database (10M sequences, one shard), its 3000-column
query and scoring through the Python wrapper, autotune off, ctx.search(db, want_scores=False, k=100), one search in
flight.  For prune_gate = 1 (off), 2 (forced) and 0 (automatic), everything else automatic: R searches with the tables
resident, then two searches each behind a set_query of the same query (a new epoch: the search pays its tables again;
wall_ms is the host clock around the whole search).  One JSON line per search.  --auto-only sets no pruning option at
all, so the script also runs on a library without the gate (the parent of an A/B; SWG_ROOT names its built checkout).
--count-gate: behind the forced candidate's searches, the pairs that left at the gate, read from the pair bounds against
U_1 = max(U_1x, U_1y) of the host mirror (swg_debug_prune_bound): pairs behind the first stage with U_1 below the T of
the gated launch, every one of which must hold exactly U_1; and the share of the pair rows behind the first stage that
was walked."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.environ.get("SWG_ROOT") or os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import swg_loader  # noqa: E402

swg = swg_loader.load()

CANDIDATES = [("gate off", {"prune_gate": 1}), ("gate forced", {"prune_gate": 2}), ("auto", {"prune_gate": 0})]


def count_gate(ctx, db, sh, q):
    sub = np.asarray(swg.load_scoring("BLOSUM62").table(), dtype=np.int8).reshape(32, 32)
    u = swg.debug_prune_bound(sub, q, sh["flat"], sh["offsets"])[1].astype(np.int64)
    lens = np.diff(sh["offsets"].astype(np.int64))
    order = np.fromiter((int(v) for v in db.order()), dtype=np.int64)
    x, y = order[0::2], order[1::2]
    ok = y != 0xFFFFFFFF
    # (the order names original indices: back to the shard's own positions)
    at = np.zeros(int(sh["index"].max()) + 1, dtype=np.int64)
    at[sh["index"].astype(np.int64)] = np.arange(len(sh["index"]))
    x, y = at[x], np.where(ok, at[np.where(ok, y, 0)], 0)
    u1 = u[x].copy()
    u1[ok] = np.maximum(u1[ok], u[y[ok]])
    got = ctx.debug_prune_refine_read(db)
    b = got["bounds"].astype(np.int64)[:len(u1)]
    begin, _, T, _ = got["stages"][0]
    behind = np.arange(len(u1)) >= begin
    left = behind & (u1 < T)
    rows = (2 + lens[x] + 3) // 4 * 4
    return {"gate_T": int(T), "first_stage_pairs": int(begin), "first_stage_not_bounded": bool(np.all(b[:begin] == 0xFFFFFFFF)),
            "pairs_behind": int(behind.sum()), "pairs_left_at_gate": int(left.sum()), "left_hold_u1": bool(np.array_equal(b[left], u1[left])),
            "walked_hold_at_most_u1": bool(np.all(b[behind & ~left] <= u1[behind & ~left])),
            "rows_first_stage_share": float(rows[:begin].sum()) / float(rows.sum()),
            "rows_walked_share_of_all": float(rows[behind & ~left].sum()) / float(rows.sum()),
            "rows_walked_share_behind": float(rows[behind & ~left].sum()) / float(rows[behind].sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nseq", type=int, default=10000000)
    ap.add_argument("--lq", type=int, default=3000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--auto-only", action="store_true", help="the library's defaults only: no pruning option is set")
    ap.add_argument("--count-gate", action="store_true", help="the pairs that left at the gate, from the pair bounds against U_1")
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
            got = ctx.debug_prune_refine_read(db, arrays=False)
            gated = ctx.debug_prune_gate() if hasattr(ctx, "debug_prune_gate") else None
            if want is None:
                want = hits
            print(json.dumps({"candidate": name, **options, "fresh_query": fresh, "rep": rep, "k_used": got["k"], "S_used": got["segments"],
                              "gated": gated, "wall_ms": round(wall, 2), "fill_ms": st["fill_ms"], "total_ms": st["total_ms"], "info": info,
                              "rows_kept_frac": 1.0 - info["pair_rows_skipped"] / max(1, info["pair_rows"]),
                              "hits_equal_first": hits == want}), flush=True)
        if a.count_gate and options.get("prune_gate") == 2:
            print(json.dumps({"candidate": name, **count_gate(ctx, db, sh, q)}), flush=True)
    db.close()


if __name__ == "__main__":
    main()
