"""swg_pssm_build_multi under options "pssm_blocks" and "pssm_purge", measured three ways on the shapes of pssm_build_ab.py:

  default   options 0 / 0 on this build beside another build of the library (--parent DIR: the tree of the parent commit,
            built) -- the default path is meant to run the kernels it ran before;
  blocks    pssm_blocks = 1, the device leg beside the host leg;
  purge     pssm_purge = 94, the device leg beside the host leg.

The host leg is what a caller can do without the device path: swg_align_hits_multi with the paths over PCIe, then
swg_pssm_from_paths_ex with the same two options per query.

    python tools/sweeps/pssm_blocks_ab.py --leg host|device --shape a|b|c --blocks 0|1 --purge 0|94 [--root DIR] [--out FILE]
    python tools/sweeps/pssm_blocks_ab.py --all [--parent DIR] [--rounds 2] [--out FILE]

One leg = one process: 20 timed calls after 5 warm-ups, the host clock around the C calls (each of which ends in a stream
synchronisation), one JSON line: median, min and max in ms, a digest of every PSSM byte -- the same in both legs of a pair
-- and the purged hits.  --all runs the pairs' legs alternating for --rounds rounds, each a fresh child process under its
own time limit; the first leg that fails, hangs or disagrees ends the run."""
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
LEG_SECONDS = 240


def leg(a):
    sys.path.insert(0, os.path.abspath(a.root))
    import numpy as np
    import swg_loader
    swg = swg_loader.load()
    sh = SHAPES[a.shape]
    seed = 0x5EED0000 + sh["config"]
    sc = swg.load_scoring(sh["matrix"])
    sub = np.ascontiguousarray(sc.table(), dtype=np.int8)
    flat, off = swg.synth_db(seed, sh["n"])
    queries = [swg.synth_query(0xAB0 + 131 * i, sh["lq"]) for i in range(sh["nq"])]
    ctx = swg.Context(0)
    ctx.set_option("autotune", 0)
    if a.blocks or a.purge:                                            # (a build without the options runs the default leg only)
        ctx.set_option("pssm_blocks", a.blocks)
        ctx.set_option("pssm_purge", a.purge)
    ctx.set_scoring(sc, -2, -1)
    db = swg.Database(flat, off).upload(ctx)
    _, hits, _ = ctx.search_multi(db, queries, k=sh["k"], want_scores=False)
    nq, k, lq = sh["nq"], sh["k"], sh["lq"]
    assert all(len(r) == k for r in hits)
    arr = (swg.Hit * (nq * k))()
    for i, r in enumerate(hits):
        for j, (s, ix) in enumerate(r):
            arr[i * k + j].score, arr[i * k + j].index = s, ix
    nh = (C.c_size_t * nq)(*([k] * nq))
    qoff = np.arange(nq + 1, dtype=np.uint64) * lq
    qflat = np.ascontiguousarray(np.concatenate(queries), dtype=np.int8)
    flat = np.ascontiguousarray(flat, dtype=np.int8)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    pssm = np.zeros((nq * lq, 32), dtype=np.int8)
    info = (swg.PssmInfo * nq)()
    vp = C.c_void_p
    head = [ctx.handle, db.handle, qflat.ctypes.data_as(vp), qoff.ctypes.data_as(vp), nq, C.cast(arr, vp), k, C.cast(nh, vp)]
    if a.leg == "host":
        stride = int(swg.lib.swg_align_ops_bound_multi(db.handle, qoff.ctypes.data_as(vp), nq))
        al = (swg.Alignment * (nq * k))()
        ops = np.zeros((nq * k, stride), dtype=np.uint8)
        al_bytes = C.sizeof(swg.Alignment)

        def call():
            rc = swg.lib.swg_align_hits_multi(*head, C.cast(al, vp), ops.ctypes.data_as(vp), stride)
            for i in range(nq):
                if rc != 0:
                    break
                rc = swg.lib.swg_pssm_from_paths_ex(sub.ctypes.data_as(vp), None, 10.0, qflat[i * lq:].ctypes.data_as(vp), lq,
                                                    flat.ctypes.data_as(vp), off.ctypes.data_as(vp), C.c_void_p(C.addressof(al) + i * k * al_bytes),
                                                    ops[i * k:].ctypes.data_as(vp), stride, k, a.blocks, a.purge, pssm[i * lq:].ctypes.data_as(vp),
                                                    None, C.byref(info[i]))
            return rc
    else:
        call = lambda: swg.lib.swg_pssm_build_multi(*head, None, 10.0, pssm.ctypes.data_as(vp), None, C.cast(info, vp))   # noqa: E731
    ms = []
    for step in range(WARMUP + STEPS):
        t0 = time.perf_counter()
        rc = call()
        t1 = time.perf_counter()
        if rc != 0:
            print("call failed: %d %s / %s" % (rc, swg.lib.swg_last_error(ctx.handle), swg.lib.swg_global_error()), flush=True)
            return 1
        if step >= WARMUP:
            ms.append((t1 - t0) * 1e3)
    med = statistics.median(ms)
    purged = sum(getattr(info[i], "n_purged", 0) for i in range(nq))
    res = {"shape": a.shape, "leg": a.leg, "blocks": a.blocks, "purge": a.purge, "build": a.tag, "pairs": nq * k, "ms_median": round(med, 4),
           "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "digest": hashlib.sha1(pssm.tobytes()).hexdigest()[:16],
           "n_distinct0": round(info[0].n_distinct, 6), "n_observed": sum(info[i].n_observed for i in range(nq)), "n_purged": purged}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    db.close()
    ctx.close()
    return 0


def run_all(a):
    pairs = []                                                        # (legs of a pair: (leg, blocks, purge, root, tag))
    if a.parent:
        pairs.append([("device", 0, 0, ROOT, "this"), ("device", 0, 0, a.parent, "parent")])
    pairs.append([("host", 1, 0, ROOT, "this"), ("device", 1, 0, ROOT, "this")])
    pairs.append([("host", 0, 94, ROOT, "this"), ("device", 0, 94, ROOT, "this")])
    digests = {}
    for rnd in range(a.rounds):
        for shape in "abc":
            for pair in pairs:
                for which, blocks, purge, root, tag in pair:
                    cmd = [sys.executable, os.path.abspath(__file__), "--leg", which, "--shape", shape, "--blocks", str(blocks), "--purge", str(purge),
                           "--root", root, "--tag", tag]
                    if a.out:
                        cmd += ["--out", a.out]
                    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=LEG_SECONDS)
                    out = [l for l in r.stdout.splitlines() if l.startswith("{")]
                    if r.returncode != 0 or not out:
                        print("leg %s (%s), shape %s, blocks %d, purge %d failed: rc %d\n%s\n%s" % (which, tag, shape, blocks, purge, r.returncode,
                                                                                                 r.stdout[-1000:], r.stderr[-2000:]), flush=True)
                        return 1
                    print(out[-1], flush=True)
                    if digests.setdefault((shape, blocks, purge), json.loads(out[-1])["digest"]) != json.loads(out[-1])["digest"]:
                        print("leg %s (%s), shape %s, blocks %d, purge %d disagrees with the legs before it" % (which, tag, shape, blocks, purge), flush=True)
                        return 1
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("host", "device"))
    ap.add_argument("--shape", choices=sorted(SHAPES), default="a")
    ap.add_argument("--blocks", type=int, choices=(0, 1), default=0)
    ap.add_argument("--purge", type=int, default=0)
    ap.add_argument("--root", default=ROOT, help="the tree whose build of the library the leg loads")
    ap.add_argument("--tag", default="this")
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--parent", help="the built tree of the parent commit, for the default legs")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out")
    args = ap.parse_args()
    sys.exit(run_all(args) if args.all else leg(args))
