"""swg_comp_adjust / swg_comp_adjust_multi beside the only route a caller has without them, built from calls that exist
apart from this family, at F = 1 (where the rescaled scores are an int8 table and so a PSSM): per hit the sequence read
back (swg_db_sequence), its composition and lambda_hit on the host (numpy: Newton from the right of the root), one
rescaled PSSM per hit, and ONE swg_search_lists_pssm call with one-candidate lists for all of them.

    python tools/sweeps/comp_adjust_ab.py [--shape a|b] [--out FILE]          (GPU box; one process, the legs alternating)

Shapes: (a) one query of 367 aa against config 2's shape (100 000 sequences, PAM250 -10 / -2), its top 100; (b) 64
queries of 128 aa against config 1's shape (1 024 sequences, BLOSUM62 -11 / -1), the top 10 of each.
Both legs run in one process and alternate call by call: 5 warm-ups, then 20 timed calls each, the host clock around the
whole leg (the host leg's numpy included: it is part of that route).  Printed per shape: each leg's median, min and max
in ms, the host leg's split (read-back and lambdas, PSSMs, the search call), and whether every scaled score and ratio16
agree (they must).  The device leg also runs at F = 32, the default, for its own time."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
WARMUP, STEPS = 5, 20
SHAPES = {
    "a": dict(nq=1, lq=367, config=2, n=100000, matrix="PAM250", gaps=(-10, -2), k=100),
    "b": dict(nq=64, lq=128, config=1, n=1024, matrix="BLOSUM62", gaps=(-11, -1), k=10),
}


def lambda_newton(np, w, s):
    """The positive root of sum w exp(lambda s) = sum w, or None: bracket by doubling, Newton from the right."""
    if not (w * s).sum() < 0 or not (w[s > 0] > 0).any():
        return None
    W, hi = w.sum(), 1.0 / s[w > 0].max()
    while (w * np.exp(hi * s)).sum() <= W:
        hi *= 2.0
    lam = hi
    for _ in range(100):
        e = w * np.exp(lam * s)
        step = (e.sum() - W) / (s * e).sum()
        lam -= step
        if abs(step) <= 1e-12 * lam:
            return lam
    return None


def run(shape, out):
    sys.path.insert(0, ROOT)
    import numpy as np
    import swg_loader
    swg = swg_loader.load()
    sh = SHAPES[shape]
    sc = swg.load_scoring(sh["matrix"])
    sub = sc.table().astype(np.int64)
    flat, off = swg.synth_db(0x5EED0000 + sh["config"], sh["n"])
    queries = [swg.synth_query(0xAB0 + 131 * i, sh["lq"]) for i in range(sh["nq"])]
    ctx = swg.Context(0)
    ctx.set_option("autotune", 0)
    ctx.set_scoring(sc, *sh["gaps"])
    db = swg.Database(flat, off).upload(ctx)
    _, hits, _ = ctx.search_multi(db, queries, k=sh["k"], want_scores=False)
    ctx.set_query(queries[0])
    s = np.arange(-128, 128, dtype=np.float64)
    # the built-in background, from the library's own draws (a caller of the parent has no other way to it)
    f = np.bincount(swg.synth_db_iid(1, 64, 4096)[0].astype(np.int64), minlength=32).astype(np.float64)
    A = f > 0
    P = f / f.sum()
    split = {"lambda": [], "pssm": [], "search": []}

    def device(F):
        ctx.set_option("comp_scale", F)
        if sh["nq"] == 1:
            recs, _ = ctx.comp_adjust(db, hits[0], freq=f)
            return [recs]
        return ctx.comp_adjust_multi(db, queries, hits, freq=f)[0]

    def host():
        t0 = time.perf_counter()
        pssms, lists, ratios = [], [], []
        for q, row in zip(queries, hits):
            R = sub[q.astype(np.int64)]
            C = np.stack([np.bincount(R[:, a] + 128, minlength=256) for a in range(32)]).astype(np.float64)
            lam_std = lambda_newton(np, P[A] @ C[A], s)
            for _, ix in row:
                c = np.bincount(db.sequence(ix).astype(np.int64), minlength=32).astype(np.float64)
                lam_hit = lambda_newton(np, c[A] @ C[A], s) if c[A].sum() > 0 and lam_std else None
                ratios.append(65536 if lam_hit is None else int(np.floor(min(1.0, max(0.5, lam_hit / lam_std)) * 65536 + 0.5)))
                lists.append([ix])
        t1 = time.perf_counter()
        at = 0
        for q, row in zip(queries, hits):
            R = sub[q.astype(np.int64)]
            for _ in row:
                pssms.append(((R * ratios[at] + 32768) >> 16).astype(np.int8))
                at += 1
        t2 = time.perf_counter()
        scores, _, _ = ctx.search_lists_pssm(db, pssms, lists)
        t3 = time.perf_counter()
        split["lambda"].append((t1 - t0) * 1e3), split["pssm"].append((t2 - t1) * 1e3), split["search"].append((t3 - t2) * 1e3)
        return ratios, [int(x[0]) for x in scores]

    times = {"device_F1": [], "device_F32": [], "host_F1": []}
    same = True
    for it in range(WARMUP + STEPS):
        for name, fn in (("device_F1", lambda: device(1)), ("host_F1", host), ("device_F32", lambda: device(32))):
            t0 = time.perf_counter()
            got = fn()
            dt = (time.perf_counter() - t0) * 1e3
            if it >= WARMUP:
                times[name].append(dt)
            if name == "device_F1":
                dev = got
            elif name == "host_F1":
                flat_dev = np.concatenate(dev)
                same &= [int(r) for r in flat_dev["ratio16"]] == got[0] and [int(r) for r in flat_dev["scaled_score"]] == got[1]
    res = {"shape": shape, **{k: v for k, v in sh.items() if k != "gaps"}, "pairs": sum(len(r) for r in hits), "agree": bool(same),
           "last": ctx.debug_comp_last()["class_pairs"].__repr__()}
    for name, t in times.items():
        res[name] = {"ms_median": round(statistics.median(t), 3), "ms_min": round(min(t), 3), "ms_max": round(max(t), 3)}
    res["host_split_ms_median"] = {k: round(statistics.median(v[WARMUP:]), 3) for k, v in split.items()}
    line = json.dumps(res)
    print(line, flush=True)
    if out:
        with open(out, "a") as fh:
            fh.write(line + "\n")
    db.close()
    ctx.close()
    return 0 if same else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=tuple(SHAPES))
    ap.add_argument("--out")
    a = ap.parse_args()
    rc = 0
    for shp in ([a.shape] if a.shape else sorted(SHAPES)):
        rc |= run(shp, a.out)
    sys.exit(rc)
