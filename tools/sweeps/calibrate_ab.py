"""swg_calibrate / swg_calibrate_multi beside what a caller can do without them: score the same random sequences with
swg_search / swg_search_multi, take the score arrays over PCIe, histogram and fit on the host.

    python tools/sweeps/calibrate_ab.py --leg host|device --queries N [--out FILE]      (GPU box; one leg = one process)
    python tools/sweeps/calibrate_ab.py --all [--out FILE]

Shapes: N = 1 (swg_calibrate of one 300-aa query), 64 and 1000 (swg_calibrate_multi; 300 aa each), BLOSUM62 -11 / -1,
the default calibration size (8192 random sequences of 384 residues, seed 1), autotune off.
Legs:
  host     the random database (swg_synth_db_iid, the same sequences) packed and uploaded once, outside the timing; per
           call swg_search (N = 1) or swg_search_multi with the score arrays, then per query numpy.bincount and the
           library's own host fit (swg_gumbel_fit_hist: a caller without this library would bring a slower one)
  device   swg_calibrate / swg_calibrate_multi (the random database is made by the first, untimed call and kept)
A leg times 12 calls after 3 warm-ups with the host clock around the C calls and prints one JSON line: median, min and
max in ms, and a digest of every query's (lambda, mu) rounded to 9 digits, which must be the same in both legs.  The host
leg also reports the fill time of swg_stats; the device leg's share outside the fill is its fit kernel and the 32 bytes
per query.  --all runs the legs alternating, each a fresh child process under its own time limit; the first leg that
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
WARMUP, STEPS = 3, 12
LQ, SEQS, LEN, SEED = 300, 8192, 384, 1
LEG_SECONDS = 240
ORDER = [(leg, n) for n in (1, 64, 1000) for leg in ("host", "device", "host", "device")]


def _digest(fits):
    return hashlib.sha1(repr([("%.9g" % lam, "%.9g" % mu) for lam, mu in fits]).encode()).hexdigest()[:16]


def leg(a):
    sys.path.insert(0, ROOT)
    import numpy as np
    import swg_loader
    swg = swg_loader.load()
    nq = a.queries
    qs = [swg.synth_query(0xCA11 + i, LQ) for i in range(nq)]
    ctx = swg.Context(0)
    ctx.set_option("autotune", 0)
    ctx.set_scoring(swg.load_scoring("BLOSUM62"), -11, -1)
    ctx.set_query(qs[0])
    vp = C.c_void_p
    qoff = np.zeros(nq + 1, dtype=np.uint64)
    qoff[1:] = np.cumsum([len(q) for q in qs])
    qflat = np.ascontiguousarray(np.concatenate(qs), dtype=np.int8)
    res = {"leg": a.leg, "queries": nq, "lq": LQ, "calib_seqs": SEQS, "calib_len": LEN}
    fill = []
    if a.leg == "host":
        flat, off = swg.synth_db_iid(SEED, SEQS, LEN)
        db = swg.Database(flat, off).upload(ctx)
        scores = np.zeros((nq, db.total_count), dtype=np.int32)
        st = swg.Stats()
        fits = [None] * nq

        def call():
            if nq == 1:
                rc = swg.lib.swg_search(ctx.handle, db.handle, scores.ctypes.data_as(vp), None, 0, None, C.byref(st))
            else:
                rc = swg.lib.swg_search_multi(ctx.handle, db.handle, qflat.ctypes.data_as(vp), qoff.ctypes.data_as(vp), nq, scores.ctypes.data_as(vp),
                                              None, 0, None, C.byref(st))
            for i in range(nq):
                f = swg.gumbel_fit_hist(np.bincount(np.minimum(scores[i], 4095), minlength=4096))
                fits[i] = (f["lambda"], f["mu"])
            fill.append(st.fill_ms)
            return rc
    else:
        out = (swg.EvalueParams * nq)()
        fits = [None] * nq

        def call():
            if nq == 1:
                rc = swg.lib.swg_calibrate(ctx.handle, None, 0, C.cast(out, vp))
            else:
                rc = swg.lib.swg_calibrate_multi(ctx.handle, qflat.ctypes.data_as(vp), qoff.ctypes.data_as(vp), nq, None, 0, C.cast(out, vp))
            for i in range(nq):
                fits[i] = (out[i].lambda_, out[i].mu)
            return rc
    times = []
    for it in range(WARMUP + STEPS):
        t0 = time.perf_counter()
        rc = call()
        dt = (time.perf_counter() - t0) * 1e3
        if rc != 0:
            print(json.dumps(dict(res, error=swg.lib.swg_last_error(ctx.handle).decode())), flush=True)
            return 1
        if it >= WARMUP:
            times.append(dt)
    res.update({"ms_median": round(statistics.median(times), 3), "ms_min": round(min(times), 3), "ms_max": round(max(times), 3),
                "digest": _digest(fits), "lambda0": fits[0][0]})
    if fill:
        res["fill_ms_median"] = round(statistics.median(fill[WARMUP:]), 3)
    print(json.dumps(res), flush=True)
    return 0


def run_all(a):
    lines, digests = [], {}
    for name, n in ORDER:
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", name, "--queries", str(n)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=LEG_SECONDS)
        out = [l for l in r.stdout.splitlines() if l.startswith("{")]
        if r.returncode != 0 or not out:
            print("leg %s (%d queries) failed: rc %d\n%s" % (name, n, r.returncode, r.stderr[-2000:]), flush=True)
            return 1
        rec = json.loads(out[-1])
        lines.append(out[-1])
        print(out[-1], flush=True)
        if digests.setdefault(n, rec["digest"]) != rec["digest"]:
            print("leg %s (%d queries) disagrees with the legs before it" % (name, n), flush=True)
            return 1
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("host", "device"))
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    sys.exit(run_all(args) if args.all else leg(args))
