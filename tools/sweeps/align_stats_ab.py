"""swg_align_stats_multi beside what a user of the parent commit does for the same four counts -- swg_align_hits_multi with
path strings, then counting identities, aligned columns, gap openings and gap steps from the strings with numpy -- and
beside swg_align_bounds_multi of this build, which shows what the two counters cost.

    python tools/sweeps/align_stats_ab.py --leg parent|stats|bounds --shape a|b|c [--tree DIR] [--out FILE]      (GPU box)
    python tools/sweeps/align_stats_ab.py --all PARENT_TREE [--rounds 2] [--out FILE]

Shapes, those of DESIGN 8.2: (a) 64 queries of 128 aa against config 1 (1 024 sequences, BLOSUM62), top 10; (b) 8 queries
of 367 aa against config 2's shape (100 000 sequences, PAM250), top 100; (c) the pipeline's shape: 256 queries of 128 aa,
the top 100 each of config 2's 100 000 sequences.
  parent   swg_align_hits_multi(..., ops, stride) of the library in --tree (a built checkout of the parent commit) plus the
           counting on the host (vectorised over the steps of all paths; the residues each M step compares are gathered with
           cumulative sums); it uses nothing the parent does not have
  stats    swg_align_stats_multi of this tree's library
  bounds   swg_align_bounds_multi of this tree's library (no counts: its digest covers the seven shared fields only)
A leg is one process: it builds the database, searches the hits once (swg_search_multi), then times 20 calls after 5
warm-ups with the host clock around the call and, in the parent leg, the counting (the C call ends in a stream
synchronisation; the Python wrapper's dicts are not timed) and prints the median, the min - max and two digests: of the
seven shared fields of every result, equal in all three legs, and of the four counts, equal in parent and stats.  --all
runs the legs of every shape alternately, `--rounds` times: each leg a fresh child process under its own time limit, and
the first leg that fails, hangs or disagrees ends the run."""
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
WARMUP, STEPS = 5, 20
SHAPES = {
    "a": dict(nq=64, lq=128, config=1, n=1024, matrix="BLOSUM62", k=10),
    "b": dict(nq=8, lq=367, config=2, n=100000, matrix="PAM250", k=100),
    "c": dict(nq=256, lq=128, config=2, n=100000, matrix="PAM250", k=100),
}
LEGS = ("parent", "stats", "bounds")
LEG_SECONDS = 240


def count_from_ops(np, ops, stride, out, qflat, qoff, flat, off, k):
    """The four counts of every hit from its path string: ops uint8[n, stride], out uint32[n, 8] (swg_alignment)."""
    n = out.shape[0]
    n_ops = out[:, 6].astype(np.int64)
    stride = max(int(n_ops.max()), 1)          # (no step lies past the longest path)
    ops = ops[:, :stride]
    valid = np.arange(stride)[None, :] < n_ops[:, None]
    m = (ops == ord("M")) & valid
    ins = (ops == ord("I")) & valid
    dele = (ops == ord("D")) & valid
    # position of every step in the query and in the sequence: the columns / residues consumed before it
    qpos = np.cumsum(m | dele, axis=1) - (m | dele) + out[:, 2].astype(np.int64)[:, None]
    dpos = np.cumsum(m | ins, axis=1) - (m | ins) + out[:, 4].astype(np.int64)[:, None]
    qbase = np.repeat(qoff[:-1].astype(np.int64), k)[:, None]
    dbase = off[out[:, 1].astype(np.int64)].astype(np.int64)[:, None]
    qi = np.where(m, qbase + qpos, 0)
    di = np.where(m, dbase + dpos, 0)
    ident = ((qflat[qi] == flat[di]) & m).sum(axis=1)
    prev = np.concatenate([np.zeros((n, 1), dtype=ops.dtype), ops[:, :-1]], axis=1)
    opens = ((ins | dele) & (ops != prev)).sum(axis=1)
    match = m.sum(axis=1)
    return np.stack([ident, match, opens, n_ops - match], axis=1).astype(np.uint32)


def leg(a):
    sys.path.insert(0, os.path.abspath(a.tree) if a.tree else ROOT)
    import numpy as np
    import swg_loader
    swg = swg_loader.load()
    sh = SHAPES[a.shape]
    seed = 0x5EED0000 + sh["config"]
    sc = swg.load_scoring(sh["matrix"])
    flat, off = swg.synth_db(seed, sh["n"])
    queries = [swg.synth_query(0xAB0 + 131 * i, sh["lq"]) for i in range(sh["nq"])]
    ctx = swg.Context(0)
    ctx.set_option("autotune", 0)
    ctx.set_scoring(sc, -2, -1)
    db = swg.Database(flat, off).upload(ctx)
    _, hits, _ = ctx.search_multi(db, queries, k=sh["k"], want_scores=False)
    nq, k = sh["nq"], sh["k"]
    assert all(len(r) == k for r in hits)
    arr = (swg.Hit * (nq * k))()
    for i, r in enumerate(hits):
        for j, (s, ix) in enumerate(r):
            arr[i * k + j].score, arr[i * k + j].index = s, ix
    nh = (C.c_size_t * nq)(*([k] * nq))
    out = np.zeros((nq * k, 8), dtype=np.uint32)
    cnt = np.zeros((nq * k, 4), dtype=np.uint32)
    qoff = np.arange(nq + 1, dtype=np.uint64) * sh["lq"]
    qflat = np.ascontiguousarray(np.concatenate(queries), dtype=np.int8)
    flat = np.ascontiguousarray(flat, dtype=np.int8)
    vp = C.c_void_p
    args = [ctx.handle, db.handle, qflat.ctypes.data_as(vp), qoff.ctypes.data_as(vp), nq, C.cast(arr, vp), k, C.cast(nh, vp),
            out.ctypes.data_as(vp)]
    if a.leg == "parent":
        stride = int(swg.lib.swg_align_ops_bound_multi(db.handle, qoff.ctypes.data_as(vp), nq))
        ops = np.zeros((nq * k, stride), dtype=np.uint8)

        def call():
            rc = swg.lib.swg_align_hits_multi(*args, ops.ctypes.data_as(vp), stride)
            if rc == 0:
                cnt[:] = count_from_ops(np, ops, stride, out, qflat, qoff, flat, off, k)
            return rc
    elif a.leg == "stats":
        call = lambda: swg.lib.swg_align_stats_multi(*args, cnt.ctypes.data_as(vp))   # noqa: E731
    else:
        call = lambda: swg.lib.swg_align_bounds_multi(*args)                          # noqa: E731
    ms = []
    for step in range(WARMUP + STEPS):
        t0 = time.perf_counter()
        rc = call()
        t1 = time.perf_counter()
        if rc != 0:
            print("call failed: %d %s" % (rc, swg.lib.swg_last_error(ctx.handle)), flush=True)
            return 1
        if step >= WARMUP:
            ms.append((t1 - t0) * 1e3)
    cells = sum(sh["lq"] * int(off[ix + 1] - off[ix]) for r in hits for _, ix in r)
    med = statistics.median(ms)
    res = {"shape": a.shape, "leg": a.leg, "pairs": nq * k, "cells": cells, "ms_median": round(med, 4), "ms_min": round(min(ms), 4),
           "ms_max": round(max(ms), 4), "gcups": round(cells / med / 1e6, 2), "digest": hashlib.sha1(out.tobytes()).hexdigest()[:16],
           "counts_digest": None if a.leg == "bounds" else hashlib.sha1(cnt.tobytes()).hexdigest()[:16],
           "gapped": int((cnt[:, 2] > 0).sum()), "ident": int(cnt[:, 0].sum())}
    if a.leg != "parent":
        res["bounds_last"] = ctx.debug_bounds_last()
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    db.close()
    ctx.close()
    return 0


def run_all(a):
    digests, counts = {}, {}
    for rnd in range(a.rounds):
        for shape in "abc":
            for which in LEGS:
                cmd = [sys.executable, os.path.abspath(__file__), "--leg", which, "--shape", shape]
                if which == "parent":
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
                if digests.setdefault(shape, d["digest"]) != d["digest"]:
                    print("shape %s: the legs' coordinates differ -- stopping" % shape, flush=True)
                    return 1
                if which != "bounds" and counts.setdefault(shape, d["counts_digest"]) != d["counts_digest"]:
                    print("shape %s: the legs' counts differ -- stopping" % shape, flush=True)
                    return 1
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=LEGS)
    ap.add_argument("--shape", choices=tuple(SHAPES))
    ap.add_argument("--tree", help="parent leg: the built checkout whose library runs it")
    ap.add_argument("--all", metavar="PARENT_TREE", help="every shape, all legs alternating, each leg a child process")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", help="append the result lines to this file")
    a = ap.parse_args()
    if a.all:
        return run_all(a)
    if not a.leg or not a.shape:
        ap.error("--leg and --shape, or --all PARENT_TREE")
    return leg(a)


if __name__ == "__main__":
    sys.exit(main())
