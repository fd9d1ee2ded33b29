"""CPU: the gate in front of the first pruning level (option prune_gate) -- when it is taken
(swg_debug_prune_gate_choice -> swg_prune_gate_choice) and where the first level's launch then sits in the stage list
(swg_debug_prune_stages5 -> swg_prune_stages), the mirror rule of prune_gate_cases, and the hooks from before the gate,
which keep their answers."""
import numpy as np
import pytest

from prune_gate_cases import CASES, NOT_BOUNDED, expected_bounds
from test_prune_stages_host import CASES as STAGE_CASES, ONE, THREE, TWO, _expected

HEADLINE = dict(lq=3000, pair_rows=1938193684)


def test_the_choice(swg):
    # automatic: a segmented first level chosen automatically, on a range the third level pays on
    k, S, gate = swg.debug_prune_gate_choice(**HEADLINE)
    assert (k, S) == (4, 32) and gate
    assert swg.debug_prune_gate_choice(gate=1, **HEADLINE) == (4, 32, False)
    assert swg.debug_prune_gate_choice(gate=2, **HEADLINE) == (4, 32, True)
    # a forced first level keeps the ungated launch unless the gate is forced as well
    for forced in (dict(segments=32), dict(segments=8), dict(forced=4, segments=32), dict(forced=5, segments=8)):
        k, S, gate = swg.debug_prune_gate_choice(**forced, **HEADLINE)
        assert S > 1 and not gate, forced
        assert swg.debug_prune_gate_choice(gate=2, **forced, **HEADLINE)[2], forced
        assert not swg.debug_prune_gate_choice(gate=1, **forced, **HEADLINE)[2], forced
    # an unsegmented or colmax first level has no gate, whoever asks
    for forced in (dict(forced=1), dict(forced=4), dict(forced=4, segments=1), dict(forced=5, segments=1)):
        assert not swg.debug_prune_gate_choice(gate=2, **forced, **HEADLINE)[2], forced
    # not pruned: nothing
    assert swg.debug_prune_gate_choice(gate=2, pruned=0, **HEADLINE) == (0, 0, False)
    with pytest.raises(Exception):
        swg.debug_prune_gate_choice(gate=3, **HEADLINE)


def test_the_automatic_floor_is_the_third_levels(swg):
    """Automatic takes the gate exactly where the third level's rule holds for an automatic first level of (4, 32): every
    test-sized range stays ungated."""
    seen = set()
    for rows in (10 ** 5, 10 ** 7, 5 * 10 ** 7, 10 ** 8, 2 * 10 ** 8, 4 * 10 ** 8, 10 ** 9, 1938193684):
        k, S, gate = swg.debug_prune_gate_choice(lq=3000, pair_rows=rows)
        _, _, S2, S3 = swg.debug_prune_refine3_choice(lq=3000, pair_rows=rows)
        assert gate == (k == 4 and S > 1 and S3 == 256), (rows, k, S, S2, S3, gate)
        seen.add(gate)
    assert seen == {False, True}
    assert not swg.debug_prune_gate_choice(lq=300, pair_rows=10 ** 6)[2]


GATED = ("threshold", "bound")


def test_where_the_launch_sits(swg):
    # the K-th best route: the second stage only, behind the threshold kernel and in front of everything else
    assert swg.debug_prune_stages(THREE, gate=True) == [(0, 5, 0, ()), (5, 9, 1, GATED + ("list",)), (9, 10, 2, ("threshold", "list"))]
    assert swg.debug_prune_stages(ONE, head_pairs=4, gate=True) == [(0, 4, 0, ()), (4, 10, 0, GATED + ("list",))]
    assert swg.debug_prune_stages(THREE, gate=True, refine=128, refine3=256, refine4=256) == [
        (0, 5, 0, ()), (5, 9, 1, GATED + ("refine", "refine3", "refine4", "list")), (9, 10, 2, ("threshold", "refine", "refine3", "refine4", "list"))]
    assert swg.debug_prune_stages(THREE, gate=True, prefix_cut=True) == [
        (0, 5, 0, ()), (5, 9, 1, GATED + ("prefix_cut",)), (9, 10, 2, ("threshold", "prefix_cut"))]
    # one uncut stage: no stage has a threshold, so none queues the launch (the fill bounds every pair up front)
    assert swg.debug_prune_stages(ONE, gate=True) == [(0, 10, 0, ())]
    # a caller's threshold: the first stage, in front of the refine levels' own gate
    assert swg.debug_prune_stages(THREE, fixed=True, gate=True) == [(0, 5, 0, ("bound", "list")), (5, 9, 1, ("list",)), (9, 10, 2, ("list",))]
    assert swg.debug_prune_stages(THREE, fixed=True, refine=128, gate=True) == [
        (0, 5, 0, ("bound", "gate", "refine", "list")), (5, 9, 1, ("refine", "list")), (9, 10, 2, ("refine", "list"))]
    assert swg.debug_prune_stages(ONE, fixed=True, gate=True) == [(0, 10, 0, ("bound", "list"))]


@pytest.mark.parametrize("segments,plan", STAGE_CASES)
def test_no_flag_without_the_gate_and_only_the_flag_with_it(swg, segments, plan):
    plain = swg.debug_prune_stages(segments, **plan)
    assert plain == _expected(segments, **plan)
    assert all("bound" not in names for _, _, _, names in plain)
    gated = swg.debug_prune_stages(segments, gate=True, **plan)
    at = 0 if plan.get("fixed") else 1
    for si, ((b, e, sg, names), (gb, ge, gsg, gnames)) in enumerate(zip(plain, gated)):
        assert (b, e, sg) == (gb, ge, gsg)
        assert tuple(n for n in gnames if n != "bound") == names
        assert ("bound" in gnames) == (si == at)
    assert len(gated) == len(plain)


def test_the_hooks_from_before_the_gate_keep_their_answers(swg):
    """The vectors the earlier host tests use, word for word through the raw hooks: no eighth bit anywhere"""
    import ctypes as C
    lib = swg.lib
    for hook, head in ((lib.swg_debug_prune_stages, [0, 0, 64, 0]), (lib.swg_debug_prune_stages3, [0, 1, 128, 0, 256]),
                       (lib.swg_debug_prune_stages4, [0, 0, 128, 0, 256, 256]), (lib.swg_debug_prune_stages4, [4, 0, 0, 1, 0, 0])):
        for segments in (ONE, TWO, THREE):
            a = np.array(head + [len(segments)] + [v for sg in segments for v in sg], dtype=np.int64)
            out = np.zeros((8, 4), dtype=np.int64)
            n = C.c_size_t(0)
            assert hook(a.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), 8, C.byref(n)) == 0
            assert n.value >= len(segments) and not np.any(out[:, 3] & 128)
    # the choices of the levels do not read the new option
    assert swg.debug_prune_refine4_choice(**HEADLINE) == (4, 32, 128, 256, 256)
    assert swg.debug_prune_refine3_choice(**HEADLINE) == (4, 32, 128, 256)
    assert swg.debug_prune_refine3_choice(lq=300, pair_rows=10 ** 6)[3] == 0


def test_the_mirror_rule():
    ungated = np.array([900, 700, 650, 300, 280, 40, 30, 0])
    u1 = np.array([2000, 1500, 1200, 500, 290, 45, 30, 0])
    stages = [(2, 5, 400, None), (5, 8, 450, None)]
    # the K-th best route: the first stage is not bounded; behind it U_1 where it is below the first cut stage's T
    assert list(expected_bounds(ungated, u1, stages, False)) == [NOT_BOUNDED, NOT_BOUNDED, 650, 300, 290, 45, 30, 0]
    # a caller's threshold: every pair is behind the gate
    assert list(expected_bounds(ungated, u1, [(0, 5, 400, None), (5, 8, 400, None)], True)) == [900, 700, 650, 300, 290, 45, 30, 0]
    # T = 0 gates nothing; no cut stage: the ungated launch
    assert list(expected_bounds(ungated, u1, [(2, 8, 0, None)], False)) == [NOT_BOUNDED, NOT_BOUNDED, 650, 300, 280, 40, 30, 0]
    assert list(expected_bounds(ungated, u1, [], False)) == list(ungated)


def test_the_cases_name_what_the_gpu_test_needs():
    dbs = {c[0] for c in CASES.values()}
    assert {"main", "long_short", "small", "view", "shard"} <= dbs
    assert {c[2]["prune_segments"] for c in CASES.values()} >= {8, 16, 32}
    assert any(c[2]["prune_kmer"] == 5 for c in CASES.values()) and any(c[1] == "pssm" for c in CASES.values())
    assert any(c[2].get("prune_table_bits") == 16 for c in CASES.values())
    assert {c[3] for c in CASES.values()} >= {("above", "inside"), ("above", "over"), ("topk", 10)}
