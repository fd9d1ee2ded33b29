"""CPU: what swg_search_above decides about pruning ("A caller's threshold"), through the plan hook
(swg_debug_prune_plan_above -> swg_prune_plan with a fixed threshold, the one function the search asks).

The rules: the threshold stands before the first kernel, so only the structural conditions count -- non-positive gap
scores, the 16-bit lane groups off the work queue, one class, one cell form, not gapless, not in a batch -- and neither the
number of segments nor prune_head has a say: there is no head.  Option prune = 0 never prunes, 2 prunes wherever the
conditions hold, 1 (auto) asks for SWG_PRUNE_ABOVE_AUTO_PAIRS = 16 pairs per resident lane group on top."""
import ctypes as C
import itertools
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# condition -> (the value under which a search is pruned, one under which it is not)
STRUCTURAL = {
    "gap_open": (-2, 1), "gap_extend": (-1, 1), "bits": (16, 32), "use_diag": (1, 0), "n_classes": (1, 2), "work_queue": (1, 0),
    "both_forms": (0, 1), "gapless": (0, 1), "batch": (0, 1),
}


def test_abi(swg):
    for name in ("swg_search_above", "swg_search_gapless_above"):
        assert name in swg.ABI_SYMBOLS and hasattr(swg.lib, name), name
    assert hasattr(swg.lib, "swg_debug_prune_plan_above")
    assert callable(getattr(swg.Context, "search_above", None))
    assert swg.lib.swg_abi_version() == 3          # functions were added, no struct changed
    text = open(os.path.join(ROOT, "include", "swg.h")).read()
    assert "int swg_search_above(" in text and "int swg_search_gapless_above(" in text


def test_null_arguments(swg):
    nh, nt = C.c_size_t(7), C.c_uint64(7)
    for fn in (swg.lib.swg_search_above, swg.lib.swg_search_gapless_above):
        assert fn(None, None, 10, None, 0, C.byref(nh), C.byref(nt), None) == swg.SWG_ERR_ARG
        assert nh.value == 0 and nt.value == 0


@pytest.mark.parametrize("mode", [1, 2])
def test_on_exactly_when_every_structural_condition_holds(swg, mode):
    """The cross product of the structural conditions (2^9 asks), each in ranges of one segment and of several and with two
    values of prune_head: pruned exactly when all hold."""
    names = list(STRUCTURAL)
    seen_on = 0
    for bits in itertools.product((0, 1), repeat=len(names)):
        ask = {n: STRUCTURAL[n][b] for n, b in zip(names, bits)}
        want = not any(bits)
        for n_segments, prune_head in ((1, 4), (8, 4), (1, 0), (3, 4096)):
            got = swg.debug_prune_plan_above(mode=mode, n_segments=n_segments, prune_head=prune_head, **ask)
            assert got == (want, 0), (ask, n_segments, prune_head, got)
        seen_on += want
    assert seen_on == 1


@pytest.mark.parametrize("excluded", [dict(gap_open=5, gap_extend=-1), dict(gap_open=0, gap_extend=3), dict(bits=8), dict(n_classes=0),
                                      dict(range_pairs=0)], ids=lambda d: ",".join("%s=%s" % kv for kv in d.items()))
def test_other_excluded_values(swg, excluded):
    for mode in (1, 2):
        assert swg.debug_prune_plan_above(mode=mode, **excluded) == (False, 0)


def test_zero_gaps_are_prunable(swg):
    assert swg.debug_prune_plan_above(gap_open=0, gap_extend=0) == (True, 0)
    assert swg.debug_prune_plan_above(gap_open=-11, gap_extend=-1, mode=2) == (True, 0)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_segments_and_head_have_no_say(swg, mode):
    base = swg.debug_prune_plan_above(mode=mode)
    assert base == (mode != 0, 0)
    for n_segments in (0, 1, 2, 8, 1000):
        for prune_head in (-1, 0, 1, 4, 4096):
            assert swg.debug_prune_plan_above(mode=mode, n_segments=n_segments, prune_head=prune_head) == base, (n_segments, prune_head)


def test_mode_0_is_off(swg):
    assert swg.debug_prune_plan_above(mode=0) == (False, 0)
    assert swg.debug_prune_plan_above(mode=0, n_segments=1) == (False, 0)
    assert swg.debug_prune_plan_above(mode=0, range_pairs=50000000, groups=64) == (False, 0)


@pytest.mark.parametrize("groups", [1, 64, 1024, 12288])
def test_auto_asks_for_sixteen_pairs_per_lane_group(swg, groups):
    """Mode 1: a range whose fills are too short for the bound and list kernels to vanish in them stays unpruned, whatever
    its segments; mode 2 ignores the size."""
    floor = 16 * groups
    for n_segments in (1, 8):
        assert swg.debug_prune_plan_above(mode=1, range_pairs=floor - 1, groups=groups, n_segments=n_segments) == (False, 0)
        assert swg.debug_prune_plan_above(mode=1, range_pairs=floor, groups=groups, n_segments=n_segments) == (True, 0)
        assert swg.debug_prune_plan_above(mode=2, range_pairs=1, groups=groups, n_segments=n_segments) == (True, 0)
    assert swg.debug_prune_plan_above(mode=1, range_pairs=16, groups=0) == (True, 0)          # (no lane group counted: one)


def test_top_k_plan_keeps_its_answers(swg):
    """swg_debug_prune_plan still takes its 16 inputs and answers as before (rows of tests/test_prune_plan_host.py)."""
    assert swg.debug_prune_plan() == (True, 0)
    assert swg.debug_prune_plan(n_segments=1, range_pairs=1000000) == (False, 0)
    assert swg.debug_prune_plan(mode=2, n_segments=1, range_pairs=16 * 1024, groups=1024, prune_head=4, k=10) == (True, 4 * 1024)
    assert swg.debug_prune_plan(mode=2, range_pairs=2000, groups=8192, prune_head=4, k=10, n_segments=1) == (True, 500)
    assert swg.debug_prune_plan(k=0) == (False, 0) and swg.debug_prune_plan(k=4097, mode=2) == (False, 0)
    assert swg.debug_prune_plan(mode=1, want_scores=1) == (False, 0) and swg.debug_prune_plan(mode=2, want_scores=1) == (True, 0)
    assert swg.debug_prune_plan(k=198, groups=1, prune_head=4, range_pairs=100, n_segments=1, mode=2) == (True, 99)
    assert len(swg.PRUNE_PLAN_KEYS) == 16


def test_hook_argument_errors(swg):
    assert swg.lib.swg_debug_prune_plan_above(None, None) == swg.SWG_ERR_ARG
    with pytest.raises(TypeError):
        swg.debug_prune_plan_above(k=10)
    with pytest.raises(swg.SwgError):
        swg.debug_prune_plan_above(range_pairs=-1)
