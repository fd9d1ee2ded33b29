#!/usr/bin/env python3
"""Generates tests/golden/grids/prune_levels_grid.npz: what the pruned search's host decisions -- the chain of refinement levels
(swg_debug_prune_refine5_choice), the gate (swg_debug_prune_gate_choice) and the stage list (swg_debug_prune_stages6) --
answer over the grids of tests/prune_levels_grid.py.  A characterisation: it was recorded from the code as it stood before
the levels became rows of one table, so that test_prune_levels_host.py holds every later spelling to the same answers.
Run it again only where a rule is changed on purpose.  No device needed.

Fixture format: numpy .npz (arrays only): choice_rc int32[n], choice_out int16[n, 6] (k, S, S2 .. S5); gate_rc, gate_out
int16[n, 3] (k, S, gate); stage_rc, stage_out int16[n, 4, 4] ({begin, end, segment, queued} per stage, -1 behind the last).
The inputs are not stored: prune_levels_grid.py builds them in a fixed order.  (The file lies in a directory of its own:
every .npz directly under tests/golden/ is taken for a database-and-scores fixture, conftest.golden_names.)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import prune_levels_grid  # noqa: E402
import swg_loader  # noqa: E402

if __name__ == "__main__":
    swg_loader.build_module().build(verbose=False)
    grids = prune_levels_grid.compute(swg_loader.load())
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "grids", "prune_levels_grid.npz")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    np.savez_compressed(out, **grids)
    print("%s: %d bytes; %d choice rows (%d distinct answers), %d gate rows, %d stage rows" % (
        out, os.path.getsize(out), len(grids["choice_out"]), len(np.unique(grids["choice_out"], axis=0)), len(grids["gate_out"]),
        len(grids["stage_out"])))
