"""The gapless cells beside the only way the library had to produce the same scores: the gapped search with the gaps
priced out on the int16 cells.

    python tools/sweeps/gapless_ab.py --leg gapless|emulate --config 2|3 [--out FILE] [--check]      (GPU box)

Builds the benchmark's config 2 (lq 367, 100 000 sequences, PAM250) or config 3 (lq 500, 570 000 sequences, BLOSUM62)
database as bench.py does (same seeds, same generator), then times 20 steady-state searches (top-100, no score array:
bench.py's step) after 5 warm-ups and prints the median and the min - max of the wall time per search and of the fill
kernel's device time.
  gapless   Context.search_gapless, default options (autotune 0, as bench.py runs)
  emulate   Context.search after set_scoring(sub, -32766, -1) with option f16 = 0: gap magnitude 32767 on the int16
            cells, where no gap can pay below the flag level.  This leg uses nothing the parent commit does not have:
            run it from a build of the parent to compare the commits.
One process per leg; alternate the legs in the job script.  --check compares the leg's top-100 with the other leg's
definition computed here (gapless: against an emulate search in the same process)."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import swg_loader  # noqa: E402

CONFIGS = {2: dict(lq=367, n=100000, matrix="PAM250"), 3: dict(lq=500, n=570000, matrix="BLOSUM62")}
WARMUP, STEPS, K = 5, 20, 100
# the VALU issue peak of the gapless row: 3.5 packed instructions per column pair = per 2 cells of a lane, 64 lanes per
# wave-instruction, one wave-instruction per SIMD every 4 cycles, 256 CUs x 4 SIMDs at 2.4 GHz
PEAK_GCUPS = 256 * 4 * (2.4e9 / 4.0) * (64 * 2 / 3.5) / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("gapless", "emulate"), required=True)
    ap.add_argument("--config", type=int, choices=(2, 3), required=True)
    ap.add_argument("--out", help="append the result line to this file")
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    swg = swg_loader.load()
    cfg = CONFIGS[a.config]
    seed = 0x5EED0000 + a.config
    sc = swg.load_scoring(cfg["matrix"])
    q = swg.synth_query(seed, cfg["lq"])
    flat, off = swg.synth_db(seed, cfg["n"])
    ctx = swg.Context(0)
    ctx.set_option("autotune", 0)
    if a.leg == "emulate":
        ctx.set_scoring(sc, -32766, -1)
        ctx.set_option("f16", 0)
        search = lambda: ctx.search(db, want_scores=False, k=K)
    else:
        ctx.set_scoring(sc, -2, -1)
        search = lambda: ctx.search_gapless(db, want_scores=False, k=K)
    ctx.set_query(q)
    db = swg.Database(flat, off).upload(ctx)
    for _ in range(WARMUP):
        _, hits, st = search()
    wall, fill = [], []
    for _ in range(STEPS):
        t0 = time.perf_counter()
        _, hits, st = search()                      # (returns when the hits are on the host)
        wall.append((time.perf_counter() - t0) * 1e3)
        fill.append(st["fill_ms"])
    cells = st["cells"]
    med, fmed = statistics.median(wall), statistics.median(fill)
    res = {"leg": a.leg, "config": a.config, "wall_ms_median": round(med, 4), "wall_ms_min": round(min(wall), 4),
           "wall_ms_max": round(max(wall), 4), "fill_ms_median": round(fmed, 4), "fill_ms_min": round(min(fill), 4),
           "fill_ms_max": round(max(fill), 4), "gcups_wall": round(cells / med / 1e6, 1), "gcups_fill": round(cells / fmed / 1e6, 1),
           "cell_form": st["cell_form"], "K": st["cols_per_wave"], "G": st["group_lanes"], "W": st["waves"],
           "workgroups": st["workgroups"], "n_rescored": st["n_rescored"], "top": hits[0]}
    if a.leg == "gapless":
        res["fraction_of_3.5_instr_valu_peak_fill"] = round(cells / fmed / 1e6 / PEAK_GCUPS, 4)
    if a.check and a.leg == "gapless":
        ctx.set_scoring(sc, -32766, -1)
        ctx.set_option("f16", 0)
        _, ehits, _ = ctx.search(db, want_scores=False, k=K)
        res["top100_equals_emulation"] = ehits == hits
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    db.close()
    ctx.close()
    return 0 if res.get("top100_equals_emulation", True) else 1


if __name__ == "__main__":
    sys.exit(main())
