#!/usr/bin/env python3
"""Randomised soak of the call order (tests/call_order_cases.py): walks of 150 calls drawn from the movers -- every probe,
set_query to another content, length or a PSSM, the other scoring, the other handles, every forced route, every option
flipped away and back, tickets left outstanding, refused calls, masks and views made and closed -- and the probes, each
walk on a fresh context at default options with autotune on.  Every probe's answer against the CPU's truth, exactly.
Stops at the first mismatch or error and prints the walk that led to it; the seed of that walk repeats it.
usage: python tests/fuzz_calls_gpu.py [seconds] [seed]"""
import sys, time, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import swg_loader


def main(budget=60.0, seed=1):
    swg = swg_loader.load()
    import call_order_cases as co
    from test_gpu_pssm_build import _assert_same
    co.all_truths()
    t_end = time.time() + budget
    walks = calls = 0
    while time.time() < t_end:
        s = co.Session(swg, _assert_same)
        try:
            co.walk(s, np.random.default_rng(seed + walks), 150)
        except (AssertionError, swg.SwgError) as e:
            print("MISMATCH" if isinstance(e, AssertionError) else "ERROR", "in walk", walks, "of seed", seed + walks, "after", len(s.log), "calls")
            print(str(e)[:4000])
            print("the walk:", " > ".join(s.log))
            return 1
        finally:
            calls += len(s.log)
            s.close()
            co.reset_process_wide(swg)
        walks += 1
    print("ok: %d walks, %d calls, seeds %d .. %d" % (walks, calls, seed, seed + walks - 1))
    return 0


if __name__ == "__main__":
    sys.exit(main(float(sys.argv[1]) if len(sys.argv) > 1 else 60.0, int(sys.argv[2]) if len(sys.argv) > 2 else 1))
