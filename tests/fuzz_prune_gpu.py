#!/usr/bin/env python3
"""Randomised soak of the pruned searches: cases of tests/prune_fuzz_cases.py past the pinned slice -- tables, gap points,
query kinds and lengths, database families, launch segments and forced levels of the bound drawn together -- each through
every check of test_gpu_prune_fuzz.check_case: top-K pruned and not, the pruned score array, search_above with its count,
capacities and pairs_skipped, a view, a shard and two searches in flight, against the int32 oracle.
On a mismatch: the case's (seed, i), its options and swg_prune_last.
usage: python tests/fuzz_prune_gpu.py [seconds] [seed]"""
import sys, time, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import swg_loader
import prune_fuzz_cases as pc
from test_gpu_prune_fuzz import check_case

def main(budget=300.0, seed=pc.SLICE[0]):
    swg = swg_loader.load(); orc = swg_loader.oracle()
    ctx = swg.Context(0)
    t_end = time.time() + budget
    i = pc.SLICE[1]   # (the slice's own cases are the GPU test's)
    cases = cut = 0
    try:
        while time.time() < t_end:
            c = pc.case(seed, i)
            try:
                out = check_case(swg, orc, ctx, c)
            except AssertionError as e:
                print("MISMATCH case (seed %#x, i %d)" % (seed, i), pc.describe(c))
                print("  options", c["options"], "prune_last", ctx.prune_last())
                print("  ", str(e)[:2000])
                return 1
            cases += 1; cut += out["skipped"] > 0; i += 1
            if cases % 10 == 0:
                print("cases", cases, "last:", pc.describe(c), "skipped", out["skipped"], flush=True)
    finally:
        ctx.close()
    print("OK", cases, "cases (seed %#x, i %d .. %d);" % (seed, pc.SLICE[1], i - 1), cut, "skipped a pair")
    return 0

if __name__ == "__main__":
    sys.exit(main(float(sys.argv[1]) if len(sys.argv) > 1 else 300.0, int(sys.argv[2], 0) if len(sys.argv) > 2 else pc.SLICE[0]))
