"""GPU (-m gpu): every lane-group fill instantiation a single search can force -- each K of SWG_DIAG_VARIANTS in each
family of tests/instantiation_cases.py -- against the int32 oracle, bit-exact, with the launch log saying that the
intended kernel ran: family, K (the last pass's own K included), edges, and the f16 cells' pairing.  One test item is the
cases of one family at one group width: a few dozen searches of 40 .. 2200 columns against 151 sequences.
tests/test_instantiation_cases_host.py proves the matrix complete and its inputs fit, without a device."""
import numpy as np
import pytest

import instantiation_cases as ic
from test_gpu_parity import _reset_options

pytestmark = pytest.mark.gpu

GROUPS = ic.groups()
CELL_FORM = {0: 0, 1: 1, 2: 2, 3: 6}      # kernel form -> swg_stats.cell_form
K_HITS = 7


@pytest.fixture(autouse=True)
def _options(swg, ctx):
    yield
    swg.debug_launch_log(False)
    _reset_options(ctx)
    ctx.set_option("autotune", 1)
    ctx.set_option("f16_pair", 0)


@pytest.fixture(scope="module")
def db(swg, ctx):
    flat, off = ic.database()
    d = swg.Database(flat, off).upload(ctx)
    yield d
    d.close()


def _force(ctx, c):
    _reset_options(ctx)
    opts = {"engine": 2, "autotune": 0, "long_split": -1, "f16_pair": 0, "cols_per_wave": c["K"], "group_lanes": c["G"],
            "max_waves": c["W"]}
    opts.update(c["options"])
    for k, v in opts.items():
        ctx.set_option(k, v)


def _main_fill(log):
    """The records of the launches that work off the database itself, as (family, K, lanes, form, edges, fma or exact);
    launches off a device-side list are re-runs of what those flagged: allowed, and not asserted."""
    return [(r["family"], r["K"], r["G"], r["form"], r["edges"], r["fma"]) for r in log if not r["list"]]


def _run_case(swg, orc, ctx, db, c):
    want = ic.truth(c)
    ctx.set_scoring(ic.table(swg, c["scoring"]), *c["gaps"])
    ctx.set_query(np.ascontiguousarray(ic.query()[:c["lq"]]))
    _force(ctx, c)
    swg.debug_launch_log(True)
    scores, hits, st = (ctx.search_gapless if c["family"] == "gapless" else ctx.search)(db, k=K_HITS)
    log = swg.debug_launch_log_read()
    swg.debug_launch_log(False)
    label = (c["id"], st, log)
    assert np.array_equal(scores, want), (c["id"], np.nonzero(scores != want)[0][:8], scores[scores != want][:8], want[scores != want][:8], st, log)
    assert hits == orc.topk(want, K_HITS), label
    assert (st["engine"], st["work_queue"], st["path_bits"]) == (2, 1, c["bits"]), label
    assert st["cell_form"] == (CELL_FORM[c["form"]] if c["bits"] == 16 else 0), label
    ceiling = ic.cell_ceiling(c)
    assert st["n_rescored"] == (int((want >= ceiling).sum()) if ceiling else 0), label
    main = _main_fill(log)
    if c["replaced"]:
        # beyond what the exact cells hold the library runs a geometry of its own: what ran is what the log says, and it
        # must be a geometry of the exact cells that covers the query in the passes reported
        K, G, passes = st["cols_per_wave"], st["group_lanes"], st["passes"]
        assert 2 <= K <= ic.X32_MAX_K and G in ic.WIDTHS and G * K * (passes - 1) < c["lq"] <= G * K * passes, label
        assert main == [("q32", K, G, 0, 1 if passes > 1 else 0, 1)] * passes, label
        return
    assert (st["cols_per_wave"], st["group_lanes"], st["passes"], st["last_pass_cols"]) == (c["K"], c["G"], c["passes"], c["last_k"]), label
    if c["W"]:
        assert st["waves"] == c["W"] and all(r["W"] == c["W"] for r in log if not r["list"]), label
    assert main == ic.expected_main_launches(c), label


@pytest.mark.parametrize("family,lanes", sorted(GROUPS), ids=["%s-G%d" % g for g in sorted(GROUPS)])
def test_instantiations_against_the_oracle(swg, orc, ctx, db, family, lanes):
    for c in GROUPS[(family, lanes)]:
        _run_case(swg, orc, ctx, db, c)
