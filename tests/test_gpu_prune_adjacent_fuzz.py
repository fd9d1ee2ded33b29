"""GPU (-m gpu): sixteen further cases of tests/prune_fuzz_cases.py's generator -- the cases behind the pinned slice, drawn
the same way -- with the fifth level of the pruning bound forced (option prune_refine5 = 5256, and the list and byte
tables it needs), each held to the int32 oracle by every check of tests/test_gpu_prune_fuzz.py's check_case: the top-K
unpruned and pruned, the pruned score array, search_above at thresholds from the oracle's scores, a random view, shard 1
of 2 and two searches in flight, all on one context.  A case whose gaps' further residues are free, or whose tables are
no bytes, runs without the level and builds no second table; every other case builds it (the host mirror says which: six
of the sixteen)."""
import numpy as np
import pytest

import prune_fuzz_cases as pc
import test_gpu_prune_fuzz as pf

pytestmark = pytest.mark.gpu

SEED = pc.SLICE[0]
FIRST, COUNT = pc.SLICE[1], 16
RAN = {}


@pytest.fixture(scope="module")
def actx(swg):
    c = swg.Context(0)
    yield c
    c.close()


def _case(i):
    c = pc.case(SEED, i)
    c["options"].update({"prune_refine5": 5256, "prune_cut": 0, "prune_table_bits": 0})
    return c


def _admitted(swg, c):
    """Whether the case's scoring and query admit the level: the mirror's answer"""
    rows, q = (c["pssm"], None) if c["pssm"] is not None else (c["table"], c["query"])
    one, off = np.array([1], dtype=np.int8), np.array([0, 1], dtype=np.uint64)
    return pc.structural(c) and swg.debug_prune_kmer_refine5(rows, q, c["gap_open"], c["gap_extend"], 256, one, off) is not None


def _run(swg, orc, actx, i):
    c = _case(i)
    before = actx.debug_prune_tables5()["refine5_builds"]
    out = pf.check_case(swg, orc, actx, c)
    RAN[i] = actx.debug_prune_tables5()["refine5_builds"] - before
    actx.set_option("prune_refine5", 0)
    print(i, pc.describe(c), "skipped", out["skipped"], "second tables built", RAN[i])
    assert (RAN[i] > 0) == (_admitted(swg, c) and c["expect_pruned"]["above"]), (i, RAN[i])


@pytest.mark.parametrize("i", range(FIRST, FIRST + COUNT))
def test_case_with_the_fifth_level_forced(swg, orc, actx, i):
    _run(swg, orc, actx, i)


def test_the_fifth_level_ran(swg, orc, actx):
    """(cases that did not run in this session -- the test selected alone -- are run here)"""
    for i in range(FIRST, FIRST + COUNT):
        if i not in RAN:
            _run(swg, orc, actx, i)
    assert sum(1 for i in RAN if _admitted(swg, _case(i))) == 6 and sum(1 for v in RAN.values() if v > 0) == 6, RAN
