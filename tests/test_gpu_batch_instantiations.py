"""GPU (-m gpu): every batch instantiation of the lane-group fill -- two queries per lane (swg_diag_qq_kernel<K>) at 16, 32
and 64 lanes, the batch launch of swg_diag_dyn_kernel on both cell forms, and its LISTS instantiations on both -- forced
through option batch_geometry = 1 with every K of SWG_DIAG_VARIANTS (tests/batch_instantiation_cases.py), against the
int32 oracle, bit-exact, with the launch log saying that the batch's own launcher ran at the forced K and lanes and that
nothing fell back to single searches.  One test item is the cases of one family at one group width: up to 31 batches of
five queries of 1 .. 2032 columns against 151 sequences.  tests/test_batch_instantiation_cases_host.py proves the matrix
complete and able to fail, without a device."""
import numpy as np
import pytest

import batch_instantiation_cases as bc
import instantiation_cases as ic
from test_gpu_parity import _reset_options

pytestmark = pytest.mark.gpu

GROUPS = bc.groups()
K_HITS = 7
FILL = -7
OWN_LQ = 40               # the context's own query: a prefix of QUERY no case's batch holds


@pytest.fixture(autouse=True)
def _options(swg, ctx):
    yield
    swg.debug_launch_log(False)
    _reset_options(ctx)
    ctx.set_option("batch_geometry", 0)
    ctx.set_option("autotune", 1)


@pytest.fixture(scope="module")
def db(swg, ctx):
    flat, off = ic.database()
    d = swg.Database(flat, off).upload(ctx)
    yield d
    d.close()


def _force(ctx, c):
    _reset_options(ctx)
    opts = {"engine": 2, "autotune": 0, "batch_geometry": 1, "cols_per_wave": c["K"], "group_lanes": c["G"]}
    opts.update(c["options"])
    for k, v in opts.items():
        ctx.set_option(k, v)


def _records(log):
    return [(r["family"], r["K"], r["G"], r["form"], r["edges"], r["fma"], r["list"], r["grid_rows"]) for r in log]


def _expected_list_hits(truth_row, held, k):
    return [(-s, i) for s, i in sorted((-int(truth_row[i]), int(i)) for i in np.unique(held))[:k]]


def _run_case(swg, orc, ctx, db, c):
    want, qs = bc.truth(c), [np.asarray(q) for q in bc.queries(c)]
    _force(ctx, c)
    swg.debug_launch_log(True)
    if c["lists"]:
        ls = bc.lists(c)
        scores, hits, st = ctx.search_lists(db, qs, ls, k=K_HITS, fill=FILL)
    else:
        scores, hits, st = ctx.search_multi(db, qs, k=K_HITS)
    log = swg.debug_launch_log_read()
    swg.debug_launch_log(False)
    label = (c["id"], st, log)
    # the launch first: a batch that fell back computes the same scores on other kernels
    assert _records(log) == bc.expected_launches(c), label
    assert (st["engine"], st["work_queue"], st["path_bits"], st["passes"], st["fill_launches"]) == (2, 1, 16, 1, 1), label
    assert (st["cols_per_wave"], st["group_lanes"], st["cell_form"]) == (c["K"], c["G"], c["cell_form"]), label
    assert st["waves"] == log[0]["W"], label
    if c["lists"]:
        # parallel to the lists; the empty list has no score, no hit and no launch of its own (the log holds one launch)
        assert len(scores) == len(ls), label
        for i, l in enumerate(ls):
            assert scores[i].shape == (len(l),), (c["id"], i)
            bad = np.nonzero(scores[i] != want[i][l])[0]
            assert bad.size == 0, (c["id"], i, l[bad][:8], scores[i][bad][:8], want[i][l][bad][:8], st, log)
            assert hits[i] == _expected_list_hits(want[i], l, K_HITS), (c["id"], i, st)
        assert len(ls[3]) == 0 and hits[3] == [], label
    else:
        assert scores.shape == want.shape, label
        for i in range(len(qs)):
            bad = np.nonzero(scores[i] != want[i])[0]
            assert bad.size == 0, (c["id"], i, bad[:8], scores[i][bad][:8], want[i][bad][:8], st, log)
            assert hits[i] == orc.topk(want[i], K_HITS), (c["id"], i, st)


def _own_query_survives(ctx, db, c):
    """The context's own query after the batch: a plain search of it (default options) reports its scores."""
    _reset_options(ctx)
    ctx.set_option("batch_geometry", 0)
    ctx.set_option("engine", 2)
    scores, _, st = ctx.search(db)
    assert np.array_equal(scores, ic._truth(OWN_LQ, bc.SCORING, bc.GAPS[0], bc.GAPS[1], False)), (c["id"], st)


@pytest.mark.parametrize("family,lanes", sorted(GROUPS), ids=["%s-G%d" % g for g in sorted(GROUPS)])
def test_batch_instantiations_against_the_oracle(swg, orc, ctx, db, family, lanes):
    ctx.set_scoring(ic.table(swg, bc.SCORING), *bc.GAPS)
    ctx.set_query(np.ascontiguousarray(ic.query()[:OWN_LQ]))
    for c in GROUPS[(family, lanes)]:
        _run_case(swg, orc, ctx, db, c)
        _own_query_survives(ctx, db, c)


def test_without_the_option_a_forced_geometry_still_goes_one_by_one(swg, orc, ctx, db):
    """Default behaviour is what it was: cols_per_wave and group_lanes without batch_geometry send the batch through one
    search per query, each at the forced geometry; and the option takes 0 or 1 only."""
    c = next(c for c in bc.cases() if c["family"] == "batch_f16" and c["K"] == 5)
    want, qs = bc.truth(c), [np.asarray(q) for q in bc.queries(c)]
    ctx.set_scoring(ic.table(swg, bc.SCORING), *bc.GAPS)
    with pytest.raises(swg.SwgError):
        ctx.set_option("batch_geometry", 2)
    for lists in (None, bc._lists(c["K"], c["G"])):
        _force(ctx, c)
        ctx.set_option("batch_geometry", 0)
        swg.debug_launch_log(True)
        if lists is None:
            scores, _, st = ctx.search_multi(db, qs, k=K_HITS)
        else:
            scores, _, st = ctx.search_lists(db, qs, lists, k=K_HITS, fill=FILL)
        log = [r for r in swg.debug_launch_log_read() if not r["list"]]
        swg.debug_launch_log(False)
        # (fill_launches: the batch's own launches, none on this route; every launch there was is one query's)
        assert st["fill_launches"] == 0 and log and all(r["family"] not in ("qq", "lists") and r["grid_rows"] == 1 for r in log), (st, log)
        if lists is None:
            assert [(r["family"], r["K"], r["G"]) for r in log] == [("dyn", c["K"], c["G"])] * len(qs), log
        for i in range(len(qs)):
            assert np.array_equal(scores[i], want[i] if lists is None else want[i][lists[i]]), (i, st)
