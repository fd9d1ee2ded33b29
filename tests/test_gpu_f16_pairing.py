"""GPU (-m gpu): the packed-f16 cells with either pairing of the sequences' profile words (option f16_pair: 1 v_perm_b32,
2 v_pk_fma_f16 wherever its profile fits) give identical scores and flags, equal to the int32 oracle -- on the golden
vectors (the *_f16_boundary ones straddle the f16 cells' ceiling) and on queries of several passes, where the launch log
says which pairing's kernels ran."""
import numpy as np
import pytest

from conftest import golden_names, load_golden

pytestmark = pytest.mark.gpu

FORCED = ("cols_per_wave", "group_lanes")


def _search(swg, ctx, sub, go, ge, q, flat, off, f16_pair, cols=0, group=0, log=None):
    """log: a list that receives the launch log's records of the search."""
    ctx.set_scoring(sub, go, ge)
    ctx.set_query(q)
    ctx.set_option("f16", 2)
    ctx.set_option("f16_pair", f16_pair)
    ctx.set_option("cols_per_wave", cols)
    ctx.set_option("group_lanes", group)
    db = swg.Database(flat, off).upload(ctx)
    try:
        if log is not None:
            swg.debug_launch_log(True)
        scores, hits, st = ctx.search(db, k=10)
        if log is not None:
            log.extend(swg.debug_launch_log_read())
        return scores, hits, st
    finally:
        swg.debug_launch_log(False)
        db.close()
        ctx.set_option("f16", 1)
        ctx.set_option("f16_pair", 0)
        for k in FORCED:
            ctx.set_option(k, 0)


@pytest.mark.parametrize("name", golden_names())
def test_golden_both_pairings(swg, ctx, name):
    g = load_golden(name)
    go, ge = int(g["gaps"][0]), int(g["gaps"][1])
    ctx.set_option("engine", 2)
    try:
        runs = [_search(swg, ctx, g["sub"], go, ge, g["query"], g["flat"], g["offsets"], fp) for fp in (1, 2)]
    finally:
        ctx.set_option("engine", 0)
    (s1, h1, st1), (s2, h2, st2) = runs
    assert np.array_equal(s1, g["oracle32"]), (name, st1)
    assert np.array_equal(s2, s1), (name, st2)
    assert h1 == h2
    assert st1["cell_form"] == st2["cell_form"] and st1["n_rescored"] == st2["n_rescored"], (st1, st2)
    # (the magnitude of a gap's first position is -(gap_open + gap_extend): gapedge_2048_1 is 2049 and takes int16 cells)
    if go <= 0 and ge <= 0 and -(go + ge) <= 2048 and -ge <= 2048:
        assert st2["cell_form"] == 2 and st2["n_rescored"] == int((g["oracle32"] >= 4096).sum()), st2


# several passes: 16 lanes x 32 columns (4 passes of 512 for 1700 columns, the last one on 11 columns per lane);
# 16 x 21 (an odd K: the fma slice pads it to 22 columns, 6 passes); 32 x 14 (4 passes); the library's own geometry
@pytest.mark.parametrize("cols,group", [(32, 16), (21, 16), (14, 32), (0, 0)])
def test_several_passes_both_pairings(swg, ctx, orc, cols, group):
    lq = 1700
    q = swg.synth_query(0x5EED00F1, lq)
    flat, off, _ = swg.synth_db(0x5EED00F1, 400, query=q, fraction=0.05, subst=0.1)
    sc = swg.load_scoring("BLOSUM62")
    want = orc.score_db(q, flat, off, sc.table(), -11, -1)
    assert (want >= 4096).any() and (want < 4096).any() # some pairs are flagged, the others finish on the f16 cells
    logs = {1: [], 2: []}
    res = [_search(swg, ctx, sc, -11, -1, q, flat, off, fp, cols, group, log=logs[fp]) for fp in (1, 2)]
    (s1, h1, st1), (s2, h2, st2) = res
    assert np.array_equal(s1, want), st1
    assert np.array_equal(s2, want), st2
    assert h1 == h2
    assert st1["cell_form"] == st2["cell_form"] == 2
    assert st1["n_rescored"] == st2["n_rescored"] == int((want >= 4096).sum())
    if cols:
        assert st1["passes"] == st2["passes"] >= 3, st2
    # which kernels ran: the f16 fill's launches off the database itself (the re-runs of flagged pairs work off a list, on int16 cells)
    fills = {fp: [r for r in logs[fp] if r["family"] == "dyn" and r["form"] == 2 and not r["list"]] for fp in (1, 2)}
    assert fills[1] and not any(r["fma"] for r in logs[1]), logs[1]     # f16_pair = 1: the fma kernels never
    if cols:
        # f16_pair = 2 at (32, 16), (21, 16) and (14, 32): every pass on the fma kernels with edges, all but the last on the K asked for
        assert len(fills[2]) == st2["passes"] and all(r["fma"] == 1 and r["edges"] == 1 and r["G"] == group for r in fills[2]), logs[2]
        assert [r["K"] for r in fills[2][:-1]] == [cols] * (st2["passes"] - 1), logs[2]
        assert fills[2][-1]["K"] == (st2["last_pass_cols"] or cols), logs[2]
        assert [(r["K"], r["G"], r["edges"]) for r in fills[1]] == [(r["K"], r["G"], r["edges"]) for r in fills[2]], (logs[1], logs[2])
