"""CPU: the matrix of tests/engine_instantiation_cases.py -- every fixed-stream and every systolic fill instantiation -- is
complete, the planner answers every one of its cases as the case intends (swg_debug_plan_streams, swg_debug_plan_systolic),
and the inputs have the properties the GPU test (tests/test_gpu_engine_instantiations.py) relies on: every local column and
every edge hand-over decides a score the main fill reports.  All against the int32 oracle, no device involved."""
import collections

import numpy as np
import pytest

import engine_instantiation_cases as ec
import instantiation_cases as ic
import swg_loader


@pytest.fixture(scope="module")
def swg():
    return swg_loader.load()


@pytest.fixture(scope="module")
def db(swg):
    flat, off = ec.database()
    d = swg.Database(flat, off)
    yield d
    d.close()


def test_every_instantiation_has_a_case(swg):
    """An entry added to SWG_DIAG_VARIANTS, or a systolic strip width added to the library, fails here until it has cases."""
    ks = sorted(k for k, _ in ic.variant_ks())
    assert ks == list(ic.KS), "SWG_DIAG_VARIANTS changed: extend instantiation_cases.KS and the matrices"
    have = collections.defaultdict(list)
    for c in ec.cases():
        have[c["family"]].append(c)
    # the fixed streams: every (K, form), the passes that select the kernel, every K at a group width and every width often
    for fam in ("streams_single", "streams_multi", "streams_wide"):
        assert sorted(c["K"] for c in have[fam]) == ks, fam
    assert all(c["passes"] == 1 and c["form"] == 0 for c in have["streams_single"])
    assert all(c["passes"] in (2, 3) and c["form"] == 0 for c in have["streams_multi"])
    assert all(c["form"] == 1 and c["lq"] >= ec.WIDE_MIN_LQ for c in have["streams_wide"])
    assert {c["passes"] == 1 for c in have["streams_wide"]} == {True, False}        # (the wide kernel "also runs one pass")
    widths = collections.Counter(c["G"] for c in have["streams_single"])
    assert set(widths) == set(ic.WIDTHS) and min(widths.values()) >= 10, widths
    assert len(have["streams_single"]) + len(have["streams_multi"]) + len(have["streams_wide"]) == 3 * len(ks) == 93
    # the systolic engine: the library's own list of strips
    v16, v32 = dict(swg.debug_systolic_variants(16)), dict(swg.debug_systolic_variants(32))
    assert set(v16) == {32, 16, 48, 24} and tuple(v32) == ec.I32_KS, (v16, v32)
    for fam, form in (("systolic_i16", 0), ("systolic_f16", 2)):
        for K, maxw in v16.items():
            assert sorted(c["W"] for c in have[fam] if c["K"] == K) == sorted((1, 2, maxw)), (fam, K)
        assert all(c["passes"] == 1 and c["form"] == form and c["bits"] == 16 for c in have[fam]), fam
    for K in v16:
        assert sorted(c["passes"] for c in have["systolic_multi"] if c["K"] == K) == [2, 3], K
    assert all(c["form"] == 0 and c["bits"] == 16 for c in have["systolic_multi"])
    for K in v32:
        assert sorted(c["passes"] for c in have["systolic_i32"] if c["K"] == K) == [1, 2], K
    assert all(c["bits"] == 32 for c in have["systolic_i32"]) and {c["K"] for c in have["systolic_i32"]} == set(v32)
    assert sorted(c["passes"] > 1 for c in have["systolic_hot"]) == [False, True] and all(c["rescore"] for c in have["systolic_hot"])
    # every W and every K legal, the last strip (the group's last lane) partly filled, no multiple of 4 in a systolic case
    for c in ec.cases():
        if c["engine"] == 1:
            assert 1 <= c["W"] <= (v32 if c["bits"] == 32 else v16)[c["K"]] and c["lq"] % 4 != 0 and c["lq"] % c["K"] != 0, c["id"]
            assert c["K"] * (c["W"] * c["passes"] - 1) < c["lq"] < c["K"] * c["W"] * c["passes"], c["id"]
        else:
            assert c["lq"] % c["K"] != 0 and c["G"] * c["K"] * (c["passes"] - 1) < c["lq"] < c["G"] * c["K"] * c["passes"], c["id"]
            if c["passes"] == 1:
                assert c["lq"] > (c["G"] - 1) * c["K"], c["id"]


def test_planner_answers_every_case_as_intended(swg, db):
    q = ec.query()
    for c in ec.cases():
        o, sub, qc = c["options"], ec.table(swg, c["scoring"]), q[:c["lq"]]
        if c["engine"] == 2:
            p = db.debug_plan_streams(sub, qc, cols=o["cols_per_wave"], group=o["group_lanes"], waves=o["max_waves"], workgroups=o["workgroups"])
            assert p["planned"], (c["id"], p)
            assert (p["classes"], p["K"], p["G"], p["W"], p["passes"], p["wide"]) == (1, c["K"], c["G"], c["W"], c["passes"], int(c["form"] == 1)), (c["id"], p)
            # one workgroup: 4 * (64 / G) streams for 134 pairs, so every lane group runs several pairs back to back
            assert p["workgroups"] == 1 and p["streams"] == ec.STREAM_W * (64 // c["G"]) <= (ec.DB_COUNT + 1) // 2 // 4, (c["id"], p)
        else:
            p = db.debug_plan_systolic(sub, qc, c["gaps"][0], c["gaps"][1], force_bits=o.get("force_bits", 0), cols=o["cols_per_wave"],
                                       max_waves=o.get("max_waves", 0), f16=o.get("f16", 1))
            assert p["planned"], (c["id"], p)
            assert (p["K"], p["W"], p["passes"], p["bits"], p["f16"]) == (c["K"], c["W"], c["passes"], c["bits"], int(c["form"] == 2)), (c["id"], p)
            assert p["workgroups"] >= 2, (c["id"], p)          # (several bins in flight)
            assert p["rescore"] == int(bool(c["rescore"])), (c["id"], p)
            if c["rescore"]:
                assert (p["rescore_K"], p["rescore_W"], p["rescore_passes"]) == c["rescore"], (c["id"], p)
    # a strip width the library does not build is no plan, for either arithmetic
    assert not db.debug_plan_systolic(ec.table(swg, "b62"), q[:100], -11, -1, cols=20)["planned"]
    assert not db.debug_plan_systolic(ec.table(swg, "b62"), q[:100], -11, -1, force_bits=32, cols=48)["planned"]


def test_inputs_have_what_the_cases_rely_on(db):
    flat, off = ec.database()
    lens = np.diff(off).astype(np.int64)
    assert len(lens) == ec.DB_COUNT and len(lens) % 2 == 1 and lens.max() == ec.MAX_LEN and ec.MAX_LEN * 11 < ic.F16_CEILING
    assert set(range(0, 10)) <= set(lens.tolist())                 # an empty record, lengths 1 .. 9
    # three bins of 128 by length: the last one is the sequences of at most 4 residues, one block of rows -- fewer than the W
    # of every multi-pass systolic case, whose passes must then stay W blocks apart (nb = W)
    by_rank = lens[db.order()]
    assert np.all(np.diff(by_rank) <= 0) and 256 < ec.DB_COUNT <= 384
    assert by_rank[256] <= 4 < by_rank[255] and ec.DB_COUNT - 256 == ec.N_SHORT
    assert all(c["W"] >= 2 for c in ec.cases() if c["engine"] == 1 and c["passes"] > 1)
    for c in ec.cases():
        t = ec.truth(c)
        assert t.shape == (ec.DB_COUNT,) and t[lens == 0].max() == 0 and t[(lens >= 1) & (lens <= 4)].max() > 0, c["id"]
        if c["form"] == 1:
            assert ((t >= ic.I16_CEILING) & (t < ic.WIDE_CEILING)).any() and t.max() < ic.WIDE_CEILING, (c["id"], int(t.max()))
        elif c["rescore"]:
            assert (t >= ic.I16_CEILING).sum() >= 1 and (t < ic.I16_CEILING).sum() > 100, c["id"]
        elif c["form"] == 2:
            assert t.max() < ic.F16_CEILING, c["id"]
        elif c["bits"] == 16:
            assert t.max() < ic.I16_CEILING, c["id"]                # plain int16 cells: nothing saturates, nothing is run again


def test_every_local_column_decides_a_score():
    """An instantiation that computed one of its K local columns wrongly must change a score the main fill reports: for
    every case and every local column -- col % K of a systolic strip, (col % (G * K)) % K of a lane -- some sequence below
    the cells' ceiling has all its best cells in that column.  The column-resolved truth is numpy's, held against the oracle
    here for every case."""
    for c in ec.cases():
        assert np.array_equal(ec.case_column_best(c).max(axis=1), ec.truth(c)), c["id"]
        classes = set(np.unique(ec.column_classes(c)).tolist())
        assert classes == set(range(min(c["K"], c["lq"]))), c["id"]
        missing = classes - ec.pinned_classes(c)
        assert not missing, (c["id"], sorted(missing))


def test_every_local_column_carries_a_gap(swg):
    """The match cells are not all of a column: a wrong gap register (the vertical gap's, or what a column hands to the
    horizontal gap of the next) changes no score of an exact copy.  In every case of GAP_SWEEP[1] columns or more, every
    local column is where the best alignment of some sequence below the ceiling opens a gap."""
    n = 0
    for c in ec.cases():
        if c["lq"] < ec.GAP_SWEEP[1]:
            continue
        missing = set(range(c["K"])) - ec.gap_pinned_classes(c, swg)
        assert not missing, (c["id"], sorted(missing))
        n += 1
    # (the shorter prefixes: systolic strips at one or two wavefronts, two short multi-pass ones, the fixed streams at K = 3:
    # every family has every K in a longer case beside them, but for the 16 x 3 columns of the single-pass fixed streams)
    assert n == sum(c["lq"] >= ec.GAP_SWEEP[1] for c in ec.cases()) >= len(ec.cases()) - 24, n
    for fam in ("streams_single", "streams_multi", "streams_wide", "systolic_i16", "systolic_f16", "systolic_multi", "systolic_hot", "systolic_i32"):
        for K in {c["K"] for c in ec.cases() if c["family"] == fam}:
            assert any(c["lq"] >= ec.GAP_SWEEP[1] for c in ec.cases() if c["family"] == fam and c["K"] == K) or (fam, K) == ("streams_single", 3), (fam, K)


def test_every_boundary_decides_a_score():
    """A wrong or stale edge where a pass or a systolic strip ends must change a reported score: for every such column b of
    every case, some sequence below the ceiling scores strictly more against the whole prefix than against q[:b] and
    against q[b:lq], each by the oracle."""
    n = 0
    for c in ec.cases():
        bs = ec.boundaries(c)
        assert bool(bs) == (c["passes"] > 1 or (c["engine"] == 1 and c["W"] > 1)), c["id"]
        whole, ok = ec.truth(c), ec.counted(c)
        for b in bs:
            left, right = ec.window_truth(0, b, c["scoring"], *c["gaps"]), ec.window_truth(b, c["lq"], c["scoring"], *c["gaps"])
            assert (ok & (whole > left) & (whole > right)).any(), (c["id"], b)
            n += 1
    assert n > 200
