"""CPU: the interface of swg_search_above_multi* (every hit at or above a score, per query of a batch; DESIGN 4.2.1, "A
caller's threshold, per query of a batch") as far as it stands without a device: the symbols, the NULL-argument errors with
zeroed outputs, and the truth table of the rule that chooses between the one launch and one query after another
(swg_debug_above_multi_route -> swg_above_multi_route, the one function the call asks)."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("swg_search_above_multi", "swg_search_above_multi_pssm", "swg_search_gapless_above_multi", "swg_search_gapless_above_multi_pssm")


def test_abi(swg):
    text = open(os.path.join(ROOT, "include", "swg.h")).read()
    for name in NAMES:
        assert name in swg.ABI_SYMBOLS and hasattr(swg.lib, name), name
        assert "int %s(" % name in text, name
    assert hasattr(swg.lib, "swg_debug_above_multi_route")
    for method in ("search_above_multi", "search_above_multi_pssm"):
        assert callable(getattr(swg.Context, method, None)), method
    assert swg.lib.swg_abi_version() == 3          # functions were added, no struct changed
    assert '"above_batch"' in text


def test_null_arguments(swg):
    q = np.array([1, 2, 3, 4], dtype=np.int8)
    off = np.array([0, 2, 4], dtype=np.uint64)
    ms = np.array([5, 5], dtype=np.int32)
    vp = C.c_void_p
    for name in NAMES:
        fn = getattr(swg.lib, name)
        for args in ((None, None, None), (q.ctypes.data_as(vp), off.ctypes.data_as(vp), None),
                     (q.ctypes.data_as(vp), off.ctypes.data_as(vp), ms.ctypes.data_as(vp))):
            nh = np.full(2, 7, dtype=np.uintp)
            nt = np.full(2, 7, dtype=np.uint64)
            rc = fn(None, None, args[0], args[1], 2, args[2], None, 0, nh.ctypes.data_as(vp), nt.ctypes.data_as(vp), None)
            assert rc == swg.SWG_ERR_ARG, name
            assert not nh.any() and not nt.any(), name
        # the count arrays are optional
        assert fn(None, None, None, None, 2, None, None, 0, None, None, None) == swg.SWG_ERR_ARG


def test_route_truth_table(swg):
    """option x admitted x single_pruned: 2 always goes one by one; a batch plan_batch refuses does too, whatever the option;
    1 takes the launch wherever it is admitted; 0 takes it where it is admitted and a single search of the longest query
    would not be pruned."""
    want = {
        (0, True, False): 1, (0, True, True): 2, (0, False, False): 2, (0, False, True): 2,
        (1, True, False): 1, (1, True, True): 1, (1, False, False): 2, (1, False, True): 2,
        (2, True, False): 2, (2, True, True): 2, (2, False, False): 2, (2, False, True): 2,
    }
    assert set(want) == set(itertools.product((0, 1, 2), (True, False), (True, False)))
    for (option, admitted, pruned), route in want.items():
        assert swg.debug_above_multi_route(option, admitted, pruned) == route, (option, admitted, pruned)
    assert swg.debug_above_multi_route() == 1


@pytest.mark.parametrize("option", [-1, 3, 100])
def test_route_option_outside_0_to_2(swg, option):
    assert swg.lib.swg_debug_above_multi_route(option, 1, 0) == swg.SWG_ERR_ARG
    with pytest.raises(swg.SwgError):
        swg.debug_above_multi_route(option)
