"""swg_db_translate beside the only route a caller without it has to a resident six-frame translation: the host twin over
every sequence on all cores (swg_translate_flat), then swg_db_pack and swg_db_upload of the frames.

    python tools/sweeps/db_translate_ab.py --leg device|host --config 2|3 [--out FILE]      (GPU box)
    python tools/sweeps/db_translate_ab.py --all [--rounds 2] [--out FILE]

The databases are synthetic nucleotide sequences (A, C, G, T drawn evenly) of about the residues of bench.py's
configurations 2 and 3: a third of the configuration's sequences, each three times as long, so that a frame has the
lengths of the configuration's proteins (about 36 M and 207 M bases).
  device   Database.translate on the resident parent: the wall time of the call, and within it the kernel (HIP events) and
           the device-to-host copy that makes the host image (swg_translate_info reports both); the kernel's achieved
           bytes per second count 2 L read and 2 L written per L bases
  host     translate_flat + Database(...) + upload, each timed
A leg is one process: it generates and uploads the database, then times 7 rounds after 2 warm-ups and prints the medians
and a digest -- the codons and the residue composition of the resident result (swg_db_composition), equal in both legs.
--all runs the legs of both configurations alternately, `--rounds` times: each leg a fresh child process under its own
time limit, and the first leg that fails, hangs or disagrees ends the run."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
WARMUP, STEPS = 2, 7
N_SEQS = {2: 100000 // 3, 3: 570000 // 3}
LEGS = ("device", "host")
LEG_SECONDS = 300


def nucleotides(swg, config):
    _, poff = swg.synth_db(0x5EED0000 + config, N_SEQS[config])
    off = (poff.astype(np.uint64) * np.uint64(3)).astype(np.uint64)
    rng = np.random.default_rng(config)
    flat = np.array([20, 3, 1, 7], dtype=np.int8)[rng.integers(0, 4, size=int(off[-1]), dtype=np.int8)]
    return flat, off


def leg(a):
    sys.path.insert(0, ROOT)
    import swg_loader
    swg = swg_loader.load()
    flat, off = nucleotides(swg, a.config)
    ctx = swg.Context(0)
    parent = swg.Database(flat, off).upload(ctx)
    rows = []
    digest = None
    for step in range(WARMUP + STEPS):
        if a.leg == "device":
            t0 = time.perf_counter()
            m = parent.translate(ctx)
            t1 = time.perf_counter()
            info = m.translate_info()
            row = {"total_ms": (t1 - t0) * 1e3, "kernel_ms": info["kernel_ms"], "host_image_ms": info["host_image_ms"],
                   "kernel_GBps": 4.0 * int(off[-1]) / (info["kernel_ms"] * 1e-3) / 1e9}
            codons = int(info["codons"])
        else:
            t0 = time.perf_counter()
            frames, foff = swg.translate_flat(flat, off)
            t1 = time.perf_counter()
            m = swg.Database(frames, foff)
            t2 = time.perf_counter()
            m.upload(ctx)
            t3 = time.perf_counter()
            row = {"total_ms": (t3 - t0) * 1e3, "twin_ms": (t1 - t0) * 1e3, "pack_ms": (t2 - t1) * 1e3, "upload_ms": (t3 - t2) * 1e3}
            codons = int(foff[-1])
        if step >= WARMUP:
            rows.append(row)
        if digest is None:
            digest = hashlib.sha1(repr((codons, m.order()[:4096].tolist(), m.composition(ctx).tolist())).encode()).hexdigest()[:16]
        m.close()
    res = {"config": a.config, "leg": a.leg, "sequences": N_SEQS[a.config], "bases": int(off[-1]), "codons": codons, "digest": digest}
    for key in rows[0]:
        v = [r[key] for r in rows]
        res[key] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    parent.close()
    ctx.close()
    return 0


def run_all(a):
    digests = {}
    for rnd in range(a.rounds):
        for config in sorted(N_SEQS):
            for which in LEGS:
                cmd = [sys.executable, os.path.abspath(__file__), "--leg", which, "--config", str(config)]
                if a.out:
                    cmd += ["--out", a.out]
                try:
                    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=LEG_SECONDS)
                except subprocess.TimeoutExpired:
                    print("round %d config %d leg %s: no end after %d s -- stopping" % (rnd, config, which, LEG_SECONDS), flush=True)
                    return 1
                print(r.stdout, end="", flush=True)
                if r.returncode != 0:
                    print("round %d config %d leg %s: exit status %d -- stopping" % (rnd, config, which, r.returncode), flush=True)
                    return 1
                d = json.loads(r.stdout.strip().splitlines()[-1])
                if digests.setdefault(config, d["digest"]) != d["digest"]:
                    print("config %d: the legs' results differ -- stopping" % config, flush=True)
                    return 1
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=LEGS)
    ap.add_argument("--config", type=int, choices=tuple(N_SEQS))
    ap.add_argument("--all", action="store_true", help="both configurations, the legs alternating, each leg a child process")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", help="append the result lines to this file")
    a = ap.parse_args()
    if a.all:
        return run_all(a)
    if not a.leg or not a.config:
        ap.error("--leg and --config, or --all")
    return leg(a)


if __name__ == "__main__":
    sys.exit(main())
