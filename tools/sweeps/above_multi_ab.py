"""swg_search_above_multi beside the ways the parent commit answers "for every query of a batch, every sequence that scores
at least that query's S": swg_search_multi with the score arrays plus a host cut, and the loop swg_set_query +
swg_search_above.

    python tools/sweeps/above_multi_ab.py --leg LEG --shape a|b [--cand N] [--tree DIR] [--out FILE]      (GPU box)
    python tools/sweeps/above_multi_ab.py --all PARENT_TREE [--out FILE]

Shapes: (a) 64 queries of 128 aa against config 1's 1 024 sequences, each at its 10th-best score: a database one query
cannot fill.  (b) 8 queries against the first database of CANDIDATES on which BOTH routes are possible: plan_batch admits
the batch to one launch (swg_stats.fill_launches >= 1 under above_batch = 1) AND swg_search_above of one of its queries
reports pruned = 1 under option prune = 1; at the score of each query's 100th hit (T) and at twice that (2T).  BLOSUM62,
gaps -2 / -1, autotune off.
Legs of the library in --tree (a built checkout of the parent commit; they use nothing the parent does not have):
  parent_scores      swg_search_multi with the score arrays, then numpy per query: the indices at or above its S, sorted in
                     the library's order
  parent_loop[_2T]   for every query swg_set_query + swg_search_above, option prune = 1 (the default)
Legs of this tree's library (swg_search_above_multi):
  new_launch[_2T]    above_batch = 1: the one launch per class and the per-row read-out on the device
  new_loop[_2T]      above_batch = 2: one query after another, each cut at its own score where the plan admits it
  new_auto[_2T]      above_batch = 0: the automatic rule
  probe              shape (b): whether candidate --cand offers both routes
A leg is one process: it builds the database, finds the thresholds with a top-K batch search, then times 12 calls after 3
warm-ups with the host clock around the C calls (parent_scores: around the call and the cut) and prints one JSON line: the
median, min and max, the fill and read-out times of swg_stats, what swg_prune_last says, and a digest of all rows, which
must be equal in every leg of a shape at the same level.  --all runs shape (a), finds shape (b)'s database, then runs its
legs, parent and new alternating: each leg a fresh child process under its own time limit, and the first leg that fails,
hangs or disagrees ends the run."""
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
WARMUP, STEPS = 3, 12
# shape (b): (sequences, query columns, seed); the first is BASELINE config 3, whose single search is pruned under prune = 1
CANDIDATES = ((570000, 500, 0x5EED0003), (570000, 256, 0x5EED0003), (1000000, 128, 0x5EED0013), (2000000, 128, 0x5EED0023))
SHAPES = {"a": dict(nq=64, lq=128, n=1024, seed=0x5EED0001, kth=10, cap=1024), "b": dict(nq=8, kth=100, cap=4096)}
PARENT_LEGS = ("parent_scores", "parent_loop", "parent_loop_2T")
NEW_LEGS = {"new_launch": 1, "new_loop": 2, "new_auto": 0}
ORDER = {"a": ("parent_scores", "new_launch", "parent_loop", "new_auto", "parent_scores", "new_launch", "new_loop"),
         "b": ("parent_loop", "new_launch", "new_loop", "parent_scores", "new_auto", "parent_loop", "new_launch", "new_loop",
               "parent_loop_2T", "new_launch_2T", "new_loop_2T", "new_auto_2T")}
LEG_SECONDS = 300


def _digest(rows):
    return hashlib.sha1(repr([[(int(s), int(i)) for s, i in r] for r in rows]).encode()).hexdigest()[:16]


def leg(a):
    sys.path.insert(0, os.path.abspath(a.tree) if a.tree else ROOT)
    import numpy as np
    import swg_loader
    swg = swg_loader.load()
    sh = dict(SHAPES[a.shape])
    if a.shape == "b":
        sh["n"], sh["lq"], sh["seed"] = CANDIDATES[a.cand]
    nq, cap = sh["nq"], sh["cap"]
    qs = [swg.synth_query(sh["seed"] + 0x100 * (i + 1), sh["lq"]) for i in range(nq)]
    ctx = swg.Context(0)
    ctx.set_option("autotune", 0)
    ctx.set_scoring(swg.load_scoring("BLOSUM62"), -2, -1)
    flat, off = swg.synth_db(sh["seed"], sh["n"])
    db = swg.Database(flat, off).upload(ctx)
    _, top, _ = ctx.search_multi(db, qs, k=sh["kth"], want_scores=False)
    mult = 2 if a.leg.endswith("_2T") else 1
    T = [max(1, t[-1][0]) * mult for t in top]
    name = a.leg[:-3] if mult == 2 else a.leg
    res = {"shape": a.shape, "leg": a.leg, "n": sh["n"], "lq": sh["lq"], "queries": nq, "level": "2T" if mult == 2 else "T", "T": T[:4]}
    vp = C.c_void_p
    qoff = np.zeros(nq + 1, dtype=np.uint64)
    qoff[1:] = np.cumsum([len(q) for q in qs])
    qflat = np.ascontiguousarray(np.concatenate(qs), dtype=np.int8)
    ms_arr = np.array(T, dtype=np.int32)
    st = swg.Stats()
    hit_t = np.dtype([("score", np.int32), ("index", np.uint32)])
    hits = np.zeros(nq * cap, dtype=hit_t)
    nh = np.zeros(nq, dtype=np.uintp)
    nt = np.zeros(nq, dtype=np.uint64)

    def rows_of():
        return [list(zip(hits["score"][i * cap:i * cap + int(nh[i])].tolist(), hits["index"][i * cap:i * cap + int(nh[i])].tolist())) for i in range(nq)]

    if a.leg == "probe":
        ctx.set_option("above_batch", 1)
        _, _, s1 = ctx.search_above_multi(db, qs, T, cap=0)
        ctx.set_option("prune", 1)
        ctx.set_query(qs[0])
        ctx.search_above(db, T[0], cap=0)
        info = ctx.prune_last()
        res.update({"cand": a.cand, "admitted": s1["fill_launches"] >= 1, "classes": 2 if s1["long_pairs"] else 1, "cell_form": s1["cell_form"],
                    "single_pruned": info["pruned"], "ok": bool(s1["fill_launches"] >= 1 and info["pruned"])})
        print(json.dumps(res), flush=True)
        return 0
    if name == "parent_scores":
        scores = np.zeros((nq, db.total_count), dtype=np.int32)
        out_rows = [None]

        def call():
            rc = swg.lib.swg_search_multi(ctx.handle, db.handle, qflat.ctypes.data_as(vp), qoff.ctypes.data_as(vp), nq, scores.ctypes.data_as(vp),
                                          None, 0, None, C.byref(st))
            rows = []
            for i in range(nq):
                ix = np.flatnonzero(scores[i] >= T[i])
                ix = ix[np.lexsort((ix, -scores[i][ix].astype(np.int64)))][:cap]
                rows.append(list(zip(scores[i][ix].tolist(), ix.tolist())))
            out_rows[0] = rows
            return rc, [st.fill_ms], [st.topk_ms]
        rows_now = lambda: out_rows[0]  # noqa: E731
    elif name == "parent_loop":
        ctx.set_option("prune", 1)
        one_h, one_t = C.c_size_t(0), C.c_uint64(0)

        def call():
            fill, read = 0.0, 0.0
            for i, q in enumerate(qs):
                rc = swg.lib.swg_set_query(ctx.handle, q.ctypes.data_as(vp), len(q))
                if rc == 0:
                    rc = swg.lib.swg_search_above(ctx.handle, db.handle, T[i], hits[i * cap:].ctypes.data_as(vp), cap, C.byref(one_h), C.byref(one_t),
                                                  C.byref(st))
                if rc != 0:
                    return rc, None, None
                nh[i], nt[i] = one_h.value, one_t.value
                fill += st.fill_ms
                read += st.topk_ms
            return 0, [fill], [read]
        rows_now = rows_of
    else:
        ctx.set_option("prune", 1)
        ctx.set_option("above_batch", NEW_LEGS[name])

        def call():
            rc = swg.lib.swg_search_above_multi(ctx.handle, db.handle, qflat.ctypes.data_as(vp), qoff.ctypes.data_as(vp), nq, ms_arr.ctypes.data_as(vp),
                                                hits.ctypes.data_as(vp), cap, nh.ctypes.data_as(vp), nt.ctypes.data_as(vp), C.byref(st))
            return rc, [st.fill_ms], [st.topk_ms]
        rows_now = rows_of
    ms, fill, readout = [], [], []
    for step in range(WARMUP + STEPS):
        t0 = time.perf_counter()
        rc, f, r = call()
        t1 = time.perf_counter()
        if rc != 0:
            print("call failed: %d %s" % (rc, swg.lib.swg_last_error(ctx.handle)), flush=True)
            return 1
        if step >= WARMUP:
            ms.append((t1 - t0) * 1e3)
            fill += f
            readout += r
    rows = rows_now()
    info = ctx.prune_last() if name != "parent_scores" else {"pruned": False, "pairs_skipped": 0}
    cells = sum(len(q) for q in qs) * int(np.diff(off.astype(np.int64)).sum())
    res.update({"ms_median": round(statistics.median(ms), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
                "fill_ms": round(statistics.median(fill), 3), "readout_ms": round(statistics.median(readout), 4),
                "gcups_wall": round(cells / (statistics.median(ms) * 1e-3) / 1e9, 1), "fill_launches": int(st.fill_launches),
                "pruned": bool(info["pruned"]), "pairs_skipped": int(info["pairs_skipped"]), "hits": sum(len(r) for r in rows),
                "digest": _digest(rows)})
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    db.close()
    ctx.close()
    return 0


def _child(a, which, shape, cand=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", which, "--shape", shape]
    if cand is not None:
        cmd += ["--cand", str(cand)]
    if which in PARENT_LEGS:
        cmd += ["--tree", a.all]
    if a.out:
        cmd += ["--out", a.out]
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=LEG_SECONDS)
    except subprocess.TimeoutExpired:
        print("shape %s leg %s: no end after %d s -- stopping" % (shape, which, LEG_SECONDS), flush=True)
        return None
    print(r.stdout, end="", flush=True)
    if r.returncode != 0:
        print("shape %s leg %s: exit status %d -- stopping" % (shape, which, r.returncode), flush=True)
        return None
    return json.loads(r.stdout.strip().splitlines()[-1])


def run_all(a):
    cand = None
    for shape in ("a", "b"):
        if shape == "b":
            for c in range(len(CANDIDATES)):
                d = _child(a, "probe", "b", c)
                if d is None:
                    return 1
                if d["ok"]:
                    cand = c
                    break
            if cand is None:
                print("shape b: no candidate database offers both routes -- NOT MEASURED", flush=True)
                return 2
        seen = {}
        for which in ORDER[shape]:
            d = _child(a, which, shape, cand)
            if d is None:
                return 1
            if seen.setdefault(d["level"], d["digest"]) != d["digest"]:
                print("shape %s: the rows of leg %s differ from the legs before it -- stopping" % (shape, which), flush=True)
                return 1
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=PARENT_LEGS + tuple(NEW_LEGS) + tuple(k + "_2T" for k in NEW_LEGS) + ("probe",))
    ap.add_argument("--shape", choices=tuple(SHAPES))
    ap.add_argument("--cand", type=int, default=0, help="shape b: which of CANDIDATES")
    ap.add_argument("--tree", help="parent legs: the built checkout whose library runs them")
    ap.add_argument("--all", metavar="PARENT_TREE", help="both shapes, every leg, parent and new alternating, each leg a child process")
    ap.add_argument("--out", help="append the result lines to this file")
    a = ap.parse_args()
    if a.all:
        return run_all(a)
    if not a.leg or not a.shape:
        ap.error("--leg and --shape, or --all PARENT_TREE")
    return leg(a)


if __name__ == "__main__":
    sys.exit(main())
