"""The grids over which the pruned search's host decisions are characterised (tests/golden/grids/prune_levels_grid.npz, written by
tests/golden/make_prune_levels_grid.py; compared by test_prune_levels_host.py): the inputs of the choice, gate and stage hooks,
and the hooks run over them.  No device needed."""
import ctypes as C
import itertools

import numpy as np

# (lq, pair rows) of the ranges: the headline, the third level's floor, a small database, an empty range
RANGES = ((3000, 1900000000), (3000, 200000000), (300, 2000000), (100, 0))
KMER = (0, 1, 4, 5)
SEGMENTS = (0, 1, 32)
REFINE = (0, 1, 64, 128)
REFINE3 = (0, 1, 256)
REFINE4 = (0, 1, 5256)
REFINE5 = (0, 1, 5256)
BITS = (8, 16)
GATE = (0, 1, 2)
SEGMENT_LISTS = (((0, 10),), ((0, 3),), ((0, 10), (10, 25)), ((0, 4), (4, 9), (9, 30)))
STAGE_CAP = 4   # stages a list of SEGMENT_LISTS can give: its segments, or the head and the rest of a lone one
STAGE_WORDS = 9 + 2 * max(len(s) for s in SEGMENT_LISTS)


def choice_inputs():
    """-> int64[n, 15]: swg_debug_prune_refine5_choice's in[0..14], the full product (default rates, pruned)"""
    rows = [(k, 1, lq, pr, 0, 0, seg, r2, r3, b4, r4, b5, r5, adm, fx)
            for k, seg, r2, r3, r4, r5, b4, b5, adm, fx, (lq, pr) in itertools.product(
                KMER, SEGMENTS, REFINE, REFINE3, REFINE4, REFINE5, BITS, BITS, (0, 1), (0, 1), RANGES)]
    return np.array(rows, dtype=np.int64)


def gate_inputs():
    """-> int64[n, 9]: swg_debug_prune_gate_choice's in[0..8]"""
    rows = [(k, 1, lq, pr, 0, 0, seg, 0, g) for k, seg, (lq, pr), g in itertools.product(KMER, SEGMENTS, RANGES, GATE)]
    return np.array(rows, dtype=np.int64)


def stage_inputs():
    """-> int64[n, STAGE_WORDS]: swg_debug_prune_stages6's in (head_pairs, fixed, refine, prefix_cut, refine3, refine4, gate,
    refine5, n, the segments), zero-filled behind the last segment"""
    rows = []
    for head, fx, cut, gate, r2, r3, r4, r5, segs in itertools.product((0, 4), (0, 1), (0, 1), (0, 1), (0, 128), (0, 256), (0, 256), (0, 256),
                                                                       SEGMENT_LISTS):
        row = [head, fx, r2, cut, r3, r4, gate, r5, len(segs)] + [v for s in segs for v in s]
        rows.append(row + [0] * (STAGE_WORDS - len(row)))
    return np.array(rows, dtype=np.int64)


def run_choice_hook(hook, inputs, n_out):
    """hook(in, out) over every row of inputs -> (return codes int32[n], out int64[n, n_out])"""
    inputs = np.ascontiguousarray(inputs, dtype=np.int64)
    rc = np.zeros(len(inputs), dtype=np.int32)
    out = np.zeros((len(inputs), n_out), dtype=np.int64)
    a, o = inputs.ctypes.data, out.ctypes.data
    sa, so = inputs.strides[0], out.strides[0]
    for i in range(len(inputs)):
        rc[i] = hook(C.c_void_p(a + i * sa), C.c_void_p(o + i * so))
    return rc, out


def run_stage_hook(hook, inputs):
    """a swg_debug_prune_stages* hook over every row -> (return codes, stages int64[n, STAGE_CAP, 4] with -1 behind the last)"""
    inputs = np.ascontiguousarray(inputs, dtype=np.int64)
    rc = np.zeros(len(inputs), dtype=np.int32)
    out = np.full((len(inputs), STAGE_CAP, 4), -1, dtype=np.int64)
    n = C.c_size_t(0)
    for i in range(len(inputs)):
        row = np.zeros((STAGE_CAP, 4), dtype=np.int64)
        rc[i] = hook(inputs[i].ctypes.data_as(C.c_void_p), row.ctypes.data_as(C.c_void_p), STAGE_CAP, C.byref(n))
        assert n.value <= STAGE_CAP
        out[i, :n.value] = row[:n.value]
    return rc, out


def compute(swg):
    """-> the three grids' answers as the fixture stores them"""
    lib = swg.lib
    c_rc, c_out = run_choice_hook(lib.swg_debug_prune_refine5_choice, choice_inputs(), 6)
    g_rc, g_out = run_choice_hook(lib.swg_debug_prune_gate_choice, gate_inputs(), 3)
    s_rc, s_out = run_stage_hook(lib.swg_debug_prune_stages6, stage_inputs())
    return {"choice_rc": c_rc, "choice_out": c_out.astype(np.int16), "gate_rc": g_rc, "gate_out": g_out.astype(np.int16),
            "stage_rc": s_rc, "stage_out": s_out.astype(np.int16)}
