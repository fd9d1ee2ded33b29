"""GPU (-m gpu): every fixed-stream fill instantiation (swg_diag_kernel: each K of SWG_DIAG_VARIANTS in one pass, in several
and in the wide form; option work_queue = 0) and every systolic one (swg_fill_kernel: int16, packed-f16 and int32 cells at
every strip width and at 1, 2 and the most wavefronts, several passes, the int32 list re-score; option engine = 1) of
tests/engine_instantiation_cases.py against the int32 oracle, bit-exact, with the stats and the launch log saying that the
intended kernel ran.  One test item is the cases of one family at one group width (fixed streams) or strip width (systolic):
searches of 9 .. 2032 columns against 267 sequences.  tests/test_engine_instantiation_cases_host.py proves the matrix
complete and its inputs fit, without a device."""
import numpy as np
import pytest

import engine_instantiation_cases as ec
from test_gpu_parity import _reset_options

pytestmark = pytest.mark.gpu

GROUPS = ec.groups()
K_HITS = 7


@pytest.fixture(autouse=True)
def _options(swg, ctx):
    yield
    swg.debug_launch_log(False)
    _reset_options(ctx)
    ctx.set_option("autotune", 1)


@pytest.fixture(scope="module")
def db(swg, ctx):
    flat, off = ec.database()
    d = swg.Database(flat, off).upload(ctx)
    yield d
    d.close()


def _records(log, listed):
    return [(r["family"], r["K"], r["G"], r["W"], r["form"], r["edges"], r["fma"]) for r in log if bool(r["list"]) == listed]


def _run_case(swg, orc, ctx, db, c):
    want = ec.truth(c)
    ctx.set_scoring(ec.table(swg, c["scoring"]), *c["gaps"])
    ctx.set_query(np.ascontiguousarray(ec.query()[:c["lq"]]))
    _reset_options(ctx)
    for k, v in c["options"].items():
        ctx.set_option(k, v)
    swg.debug_launch_log(True)
    scores, hits, st = ctx.search(db, k=K_HITS)
    log = swg.debug_launch_log_read()
    swg.debug_launch_log(False)
    label = (c["id"], st, log)
    assert np.array_equal(scores, want), (c["id"], np.nonzero(scores != want)[0][:8], scores[scores != want][:8], want[scores != want][:8], st, log)
    assert hits == orc.topk(want, K_HITS), label
    assert (st["engine"], st["work_queue"], st["path_bits"], st["cell_form"]) == (c["engine"], 0, c["bits"], c["form"]), label
    assert (st["cols_per_wave"], st["group_lanes"], st["waves"], st["passes"]) == (c["K"], c["G"], c["W"], c["passes"]), label
    ceiling = ec.cell_ceiling(c)
    assert st["n_rescored"] == (int((want >= ceiling).sum()) if ceiling else 0), label
    assert _records(log, False) == ec.expected_launches(c), label
    # launches off a device-side list: the systolic int32 re-score where the case names one (elsewhere re-runs of flagged
    # sequences are allowed, and there are none to run)
    if c["rescore"]:
        assert _records(log, True) == ec.expected_list_launches(c), label


@pytest.mark.parametrize("family,width", sorted(GROUPS), ids=["%s-%d" % g for g in sorted(GROUPS)])
def test_engine_instantiations_against_the_oracle(swg, orc, ctx, db, family, width):
    for c in GROUPS[(family, width)]:
        _run_case(swg, orc, ctx, db, c)
