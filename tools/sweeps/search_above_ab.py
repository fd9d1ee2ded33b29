"""swg_search_above beside the two ways the parent commit answers "every sequence that scores at least S": its top-K
search (which also gives the threshold: S = the score of its 100th hit) and its score-array search plus a host filter.

    python tools/sweeps/search_above_ab.py --leg LEG --shape h|3 [--tree DIR] [--opt KEY=VALUE] [--out FILE]      (GPU box)
    python tools/sweeps/search_above_ab.py --all PARENT_TREE [--rounds 2] [--out FILE]

Shapes: (h) the headline -- config 4's whole database, 10M sequences in one shard, 3000-aa query, BLOSUM62, a range of
several launch segments; (3) config 3 -- 570 000 sequences, 500-aa query, BLOSUM62, a range of ONE segment.  Gaps -2 / -1,
autotune off, one search in flight.
Legs of the library in --tree (a built checkout of the parent commit; they use nothing the parent does not have):
  parent_topk    swg_search(k = 100), default options: pruned on (h), unpruned on (3)
  parent_scores  swg_search with the score array, then numpy: the indices at or above T, sorted in the library's order
Legs of this tree's library, T = the score of the 100th hit of a top-100 search run first in the same process:
  above_p2_T  above_auto_T  above_p0_T      swg_search_above(T) under option prune = 2, 1 (automatic), 0
  above_p2_2T above_auto_2T                 swg_search_above(2 T)
A leg is one process: it builds the database, runs the top-100 search, then times 20 calls after 5 warm-ups with the host
clock around the C call (parent_scores: around the call and the filter) and prints one JSON line: the median, min and max,
the medians of the search's own fill and read-out times (swg_stats fill_ms, topk_ms: the compaction kernel and the
host's sort), what swg_prune_last says, and a digest of the hits, which must be equal in every leg of a shape at the
same threshold -- the parent's 100 hits are the head of the list at T.  --all runs the legs of both shapes, parent and
new alternating, `--rounds` times: each leg a fresh child process under its own time limit, and the first leg that
fails, hangs or disagrees ends the run."""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
WARMUP, STEPS, K = 5, 20, 100
CAP = 1 << 20
SHAPES = {"h": dict(lq=3000, n=10000000, seed=0x5EED0004, sharded=True), "3": dict(lq=500, n=570000, seed=0x5EED0003, sharded=False)}
PARENT_LEGS = ("parent_topk", "parent_scores")
NEW_LEGS = {"above_p2_T": (2, 1), "above_auto_T": (1, 1), "above_p0_T": (0, 1), "above_p2_2T": (2, 2), "above_auto_2T": (1, 2)}
# (parent_topk three times: its run-to-run spread is what the automatic rule is held against)
ORDER = ("parent_topk", "above_p2_T", "parent_scores", "above_auto_T", "parent_topk", "above_p2_2T", "parent_topk", "above_auto_2T", "above_p0_T")
LEG_SECONDS = 300


def _digest(hits):
    return hashlib.sha1(repr([(int(s), int(i)) for s, i in hits]).encode()).hexdigest()[:16]


def leg(a):
    sys.path.insert(0, os.path.abspath(a.tree) if a.tree else ROOT)
    import numpy as np
    import swg_loader
    swg = swg_loader.load()
    sh = SHAPES[a.shape]
    q = swg.synth_query(sh["seed"], sh["lq"])
    ctx = swg.Context(0)
    ctx.set_option("autotune", 0)
    ctx.set_scoring(swg.load_scoring("BLOSUM62"), -2, -1)
    ctx.set_query(q)
    if sh["sharded"]:
        s = swg.synth_db_shard(sh["seed"], sh["n"], 0, 1, query=None, fraction=0.0, subst=0.05)
        db = swg.Database(s["flat"], s["offsets"], index=s["index"], n_total=sh["n"]).upload(ctx)
    else:
        flat, off = swg.synth_db(sh["seed"], sh["n"])
        db = swg.Database(flat, off).upload(ctx)
    for kv in a.opt:
        key, v = kv.split("=", 1)
        ctx.set_option(key, int(v))
    _, top, _ = ctx.search(db, want_scores=False, k=K)
    assert len(top) == K
    T100 = top[-1][0]
    res = {"shape": a.shape, "leg": a.leg, "T100": T100}
    if a.opt:
        res["opt"] = a.opt
    vp = C.c_void_p
    st = swg.Stats()
    nh = C.c_size_t(0)
    if a.leg == "parent_topk":
        hits = (swg.Hit * K)()
        T = T100

        def call():
            rc = swg.lib.swg_search(ctx.handle, db.handle, None, C.cast(hits, vp), K, C.byref(nh), C.byref(st))
            return rc, [(hits[i].score, hits[i].index) for i in range(nh.value)] if rc == 0 else None
        timed_extra = None
    elif a.leg == "parent_scores":
        scores = np.zeros(db.total_count, dtype=np.int32)
        T = T100

        def call():
            rc = swg.lib.swg_search(ctx.handle, db.handle, scores.ctypes.data_as(vp), None, 0, C.byref(nh), C.byref(st))
            ix = np.flatnonzero(scores >= T)
            ix = ix[np.lexsort((ix, -scores[ix].astype(np.int64)))]
            return rc, list(zip(scores[ix].tolist(), ix.tolist()))
        timed_extra = None
    else:
        mode, mult = NEW_LEGS[a.leg]
        T = T100 * mult
        ctx.set_option("prune", mode)
        hits = (swg.Hit * CAP)()
        nt = C.c_uint64(0)
        view = np.frombuffer(hits, dtype=np.dtype([("score", np.int32), ("index", np.uint32)]))

        def call():
            rc = swg.lib.swg_search_above(ctx.handle, db.handle, T, C.cast(hits, vp), CAP, C.byref(nh), C.byref(nt), C.byref(st))
            return rc, (nh.value, nt.value)
        timed_extra = lambda: list(zip(view["score"][:nh.value].tolist(), view["index"][:nh.value].tolist()))  # noqa: E731
    ms, fill, readout = [], [], []
    out = None
    for step in range(WARMUP + STEPS):
        t0 = time.perf_counter()
        rc, out = call()
        t1 = time.perf_counter()
        if rc != 0:
            print("call failed: %d %s" % (rc, swg.lib.swg_last_error(ctx.handle)), flush=True)
            return 1
        if step >= WARMUP:
            ms.append((t1 - t0) * 1e3)
            fill.append(st.fill_ms)
            readout.append(st.topk_ms)
    if timed_extra:
        n_hits, n_total = out
        out = timed_extra()
        assert n_hits == n_total == len(out), (n_hits, n_total)
        if T == T100:
            assert out[:K] == top and all(s >= T for s, _ in out) and (len(out) == K or out[K][0] == T), "not the parent's hits plus ties"
        res["n_total"] = n_total
    info = ctx.prune_last()
    res.update({"T": T, "ms_median": round(statistics.median(ms), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
                "fill_ms": round(statistics.median(fill), 3), "readout_ms": round(statistics.median(readout), 4), "pruned": info["pruned"],
                "threshold": info["threshold"], "pairs_skipped": info["pairs_skipped"],
                "rows_kept": round(1.0 - info["pair_rows_skipped"] / max(1, info["pair_rows"]), 5),
                "lane_groups": int(st.streams), "pairs_per_lane_group": round((db.count + 1) // 2 / max(1, int(st.streams)), 1),
                "n_hits": len(out), "digest": _digest(out)})
    if a.leg == "parent_topk":
        res["digest_head"] = res.pop("digest")           # (the first 100 of the list at T)
    elif T == T100:
        res["digest_head"] = _digest(out[:K])
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    db.close()
    ctx.close()
    return 0


def run_all(a):
    for shape in ("3", "h"):
        seen = {}
        for rnd in range(a.rounds):
            for which in ORDER:
                cmd = [sys.executable, os.path.abspath(__file__), "--leg", which, "--shape", shape]
                if which in PARENT_LEGS:
                    cmd += ["--tree", a.all]
                if a.out:
                    cmd += ["--out", a.out]
                try:
                    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=LEG_SECONDS)
                except subprocess.TimeoutExpired:
                    print("round %d shape %s leg %s: no end after %d s -- stopping" % (rnd, shape, which, LEG_SECONDS), flush=True)
                    return 1
                print(r.stdout, end="", flush=True)
                if r.returncode != 0:
                    print("round %d shape %s leg %s: exit status %d -- stopping" % (rnd, shape, which, r.returncode), flush=True)
                    return 1
                d = json.loads(r.stdout.strip().splitlines()[-1])
                for key in ("digest", "digest_head"):
                    if key in d and seen.setdefault((key, d["T"]), d[key]) != d[key]:
                        print("shape %s: %s of leg %s differs from the legs before it -- stopping" % (shape, key, which), flush=True)
                        return 1
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=PARENT_LEGS + tuple(NEW_LEGS))
    ap.add_argument("--shape", choices=tuple(SHAPES))
    ap.add_argument("--tree", help="parent legs: the built checkout whose library runs them")
    ap.add_argument("--all", metavar="PARENT_TREE", help="both shapes, every leg, parent and new alternating, each leg a child process")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--opt", action="append", default=[], metavar="KEY=VALUE", help="a leg: set this option first (experiments)")
    ap.add_argument("--out", help="append the result lines to this file")
    a = ap.parse_args()
    if a.all:
        return run_all(a)
    if not a.leg or not a.shape:
        ap.error("--leg and --shape, or --all PARENT_TREE")
    return leg(a)


if __name__ == "__main__":
    sys.exit(main())
