"""Timings behind DESIGN 8.6 (swg_align_hsps*), on one MI355X; every mode is one process on one build.

    python tools/sweeps/align_hsps_ab.py hits   [ROOT]   swg_align_hits on config 2's top 100, with and without paths
                                                         (ROOT: the tree whose build is timed; run on this build and on the
                                                         parent commit's alternately, a fresh process each)
    python tools/sweeps/align_hsps_ab.py loop            swg_align_hsps, max_hsps = 1 / min_score = 1, against swg_align_hits
                                                         on the same hits, alternating in one process
    python tools/sweeps/align_hsps_ab.py rounds          config 2's shape with 0.1 % two-domain relatives planted, top 100,
                                                         max_hsps 1 / 2 / 4 / 8 at the min_score E = 1e-3 gives the query

Warm (2 calls), then 7 timed repeats a case; host clock around the Python call, which ends in a stream synchronise."""
import hashlib
import importlib
import os
import sys
import time

import numpy as np

MODE = sys.argv[1] if len(sys.argv) > 1 else "loop"
ROOT = os.path.abspath(sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, ROOT)
swg = importlib.import_module("seq-align-gpu_amd")
LQ, N, MAT, GAPS, K = 367, 100000, "PAM250", (-2, -1), 100


def timed(fn, warm=2, reps=7):
    for _ in range(warm):
        out = fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, ts


def show(label, ts):
    print("  %-44s median %.3f ms; range %.3f..%.3f (%.3f ms)" % (label, float(np.median(ts)), min(ts), max(ts), max(ts) - min(ts)), flush=True)


def digest(x):
    return hashlib.sha1(repr(x).encode()).hexdigest()[:12]


def config2(two_domain=False):
    sc = swg.load_scoring(MAT)
    q = swg.synth_query(0x5EED0002, LQ)
    if not two_domain:
        flat, off, _ = swg.synth_db(0x5EED0002, N, query=q, fraction=0.001, subst=0.05)
    else:
        # 0.1 % of the sequences become two-domain relatives: the query's two halves, 5 % substituted, in swapped order
        # or in order with an insert of 40 .. 120 residues between them, inside random flanks
        flat, off = swg.synth_db(0x5EED0002, N)
        rng = np.random.default_rng(0x2D0A)
        seqs = [flat[int(off[i]):int(off[i + 1])] for i in range(N)]
        aa = np.arange(1, 21, dtype=np.int8)
        aa = aa[~np.isin(aa, (2, 10, 15))]

        def mutated(x):
            return np.where(rng.random(x.size) < 0.05, rng.choice(aa, x.size), x).astype(np.int8)

        for i in rng.choice(N, N // 1000, replace=False):
            a, b = mutated(q[:LQ // 2]), mutated(q[LQ // 2:])
            gap = rng.choice(aa, int(rng.integers(40, 121)))
            parts = [b, rng.choice(aa, 8), a] if rng.random() < 0.5 else [a, gap, b]
            seqs[i] = np.concatenate([rng.choice(aa, int(rng.integers(5, 60)))] + parts + [rng.choice(aa, int(rng.integers(5, 60)))])
        off = np.zeros(N + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(s) for s in seqs])
        flat = np.ascontiguousarray(np.concatenate(seqs), dtype=np.int8)
    ctx = swg.Context(0)
    ctx.set_option("autotune", 0)
    ctx.set_scoring(sc, *GAPS)
    ctx.set_query(q)
    db = swg.Database(flat, off).upload(ctx)
    _, hits, _ = ctx.search(db, want_scores=False, k=K)
    return ctx, db, hits, off


if MODE == "hits":
    ctx, db, hits, _ = config2()
    print("swg_align_hits, config 2 top %d, build %s" % (len(hits), ROOT))
    for want_ops in (True, False):
        out, ts = timed(lambda: ctx.align_hits(db, hits, want_ops=want_ops))
        show("paths" if want_ops else "no paths", ts)
        print("  digest %s" % digest(out))
elif MODE == "loop":
    ctx, db, hits, _ = config2()
    print("swg_align_hsps(max_hsps 1, min_score 1) against swg_align_hits, config 2 top %d, alternating" % len(hits))
    for want_ops in (True, False):
        a, b = [], []
        for _ in range(3):
            want, ts = timed(lambda: ctx.align_hits(db, hits, want_ops=want_ops), reps=5)
            a += ts
            got, ts = timed(lambda: ctx.align_hsps(db, hits, 1, 1, want_ops=want_ops), reps=5)
            b += ts
        assert [[x] for x in want] == got
        show("align_hits, %s" % ("paths" if want_ops else "no paths"), a)
        show("align_hsps 1, %s" % ("paths" if want_ops else "no paths"), b)
elif MODE == "rounds":
    ctx, db, hits, off = config2(two_domain=True)
    cal = ctx.calibrate()
    ms = swg.evalue_min_score(cal, int(off[-1]), 1e-3)
    print("config 2's shape, 0.1 %% two-domain relatives, top %d; E = 1e-3 -> min_score %d (lambda %.4f, K %.4f)" % (len(hits), ms, cal["lambda"], cal["K"]))
    _, ts = timed(lambda: ctx.align_hits(db, hits, want_ops=True))
    show("align_hits, paths", ts)
    base = None
    for H in (1, 2, 4, 8):
        out, ts = timed(lambda: ctx.align_hsps(db, hits, H, ms, want_ops=True, want_counts=True))
        found = sum(len(x) for x in out)
        # a pair whose rounds ended below the score ran one fill more than it has alignments: the wasted fill
        fills = sum(len(x) + (len(x) < H) for x in out)
        show("align_hsps max_hsps %d" % H, ts)
        med = float(np.median(ts))
        base = med if base is None else base
        print("    alignments %d over %d pairs; fills %d, of which %d ended below the score; pairs with 2 or more: %d; %.3f ms over max_hsps 1"
              % (found, len(out), fills, sum(len(x) < H for x in out), sum(len(x) >= 2 for x in out), med - base), flush=True)
else:
    sys.exit("mode: hits | loop | rounds")
