"""CPU: the instantiation matrix of tests/instantiation_cases.py is complete, the planner answers every one of its cases as
the case intends, option f16_pair = 2 plans wherever f16_pair = 1 does, and the inputs have the properties the GPU test
(tests/test_gpu_instantiations.py) relies on -- all against the int32 oracle and the host-side planner hook
(swg_debug_plan_forced), no device involved."""
import collections

import numpy as np
import pytest

import instantiation_cases as ic
import swg_loader


@pytest.fixture(scope="module")
def swg():
    return swg_loader.load()


@pytest.fixture(scope="module")
def db(swg):
    flat, off = ic.database()
    d = swg.Database(flat, off)
    yield d
    d.close()


def _plan(db, c, **kw):
    o = c["options"]
    args = dict(cols=c["K"], group=c["G"], waves=c["W"], form=0 if c["form"] == 1 else c["form"], f16_pair=o.get("f16_pair", 0),
                last_pass=o.get("last_pass", 1))
    args.update(kw)
    return db.debug_plan_forced(c["lq"], **args)


def test_every_instantiation_has_a_case():
    """An entry added to SWG_DIAG_VARIANTS without a case in the matrix fails here."""
    ks = sorted(k for k, _ in ic.variant_ks())
    assert ks == list(ic.KS), "SWG_DIAG_VARIANTS changed: extend instantiation_cases.KS and the matrix"
    missing = ic.required(ks) - ic.held()
    assert not missing, sorted(missing)
    # the reduced int32 cells at the K the other deterministic tests leave out, the fallback triples, the fma last passes
    have = collections.defaultdict(set)
    for c in ic.cases():
        have[c["family"]].add((c["K"], c["G"], c["W"], c["last_k"], c["last_pass"]))
    assert {k for k, *_ in have["q32_single"]} == {k for k, *_ in have["q32_edges"]} == set(ic.Q32_KS)
    assert {(g, w, k) for k, g, w, *_ in have["f16_fallback"]} == {(g, w, k) for g, w, ks_ in ic.FALLBACK for k in ks_}
    assert have["f16_fma_last"] == {(32, g, 0, lk, 1) for g in (16, 32) for lk in ic.FMA_LAST_KS} | {(32, g, 0, 0, 0) for g in (16, 32)}
    # every K meets a group width in the rotated families, every width ten K or more
    for fam in ("i16_single", "f16_perm_single", "gapless"):
        widths = collections.Counter(g for _, g, *_ in have[fam])
        assert set(widths) == set(ic.WIDTHS) and min(widths.values()) >= 10, (fam, widths)


def test_query_lengths_leave_the_last_lane_partly_filled():
    for c in ic.cases():
        r = c["lq"] - c["G"] * c["K"] * (c["passes"] - 1)
        k_last = c["last_k"] or c["K"]
        assert 0 < r <= c["G"] * k_last and r % k_last != 0, c["id"]
        # (with last_pass = 0 the last pass keeps the others' K: some lane inside the group is the partly filled one)
        assert r > (c["G"] - 1) * k_last or not c["last_pass"], c["id"]


def test_planner_answers_every_case_as_intended(db):
    """The lane-group families whose geometry the int16 planner decides (the int32 families' is decided by plan_search on top
    of it, and asserted from the launch log on the GPU)."""
    n = 0
    for c in ic.cases():
        if c["launcher"] != "dyn":
            continue
        p = _plan(db, c)
        assert p["planned"], (c["id"], p)
        assert (p["K"], p["G"], p["passes"], p["classes"]) == (c["K"], c["G"], c["passes"], 1), (c["id"], p)
        assert p["fma"] == c["fma"], (c["id"], p)
        assert p["last_pass_cols"] == c["last_k"], (c["id"], p)
        assert p["lds_bytes"] <= ic.LDS, (c["id"], p)
        if c["W"]:
            assert p["W"] == c["W"], (c["id"], p)
        if c["family"] == "f16_fallback":
            # the same geometry with the perm pairing asked for is the same plan
            q = _plan(db, c, f16_pair=1)
            assert {k: v for k, v in p.items() if k != "est_us"} == {k: v for k, v in q.items() if k != "est_us"}, (c["id"], p, q)
        n += 1
    assert n > 300


def test_int32_cases_ask_for_what_the_int32_cells_hold():
    """The int32 families' geometry is decided by the search itself (asserted from the launch log on the GPU); here, that each
    case asks for an instantiation that exists and fits: K of the macro, at most SWG_X32_MAX_K for the exact cells unless
    the case expects a replacement, a profile of 128 bytes per (even-padded) column and the records within LDS."""
    ks = {k for k, _ in ic.variant_ks()}
    n = 0
    for c in ic.cases():
        if c["launcher"] == "dyn":
            continue
        assert c["K"] in ks and c["G"] in ic.WIDTHS and c["bits"] == 32 and c["W"] == 0 and not c["last_k"], c["id"]
        assert c["replaced"] == (c["exact"] == 1 and c["K"] > ic.X32_MAX_K), c["id"]
        assert c["passes"] == -(-c["lq"] // (c["G"] * c["K"])) <= 64, c["id"]
        if not c["replaced"]:
            assert c["G"] * ((c["K"] + 1) // 2 * 2) * 128 + 4 * (64 // c["G"]) * 512 <= ic.LDS, c["id"]
        n += 1
    assert n == sum(c["family"] in ("x32_single", "x32_edges", "q32_single", "q32_edges") for c in ic.cases()) > 60


def test_f16_pair_2_plans_wherever_f16_pair_1_does(db):
    """Option f16_pair = 2 is "v_pk_fma_f16 wherever it fits, v_perm_b32 elsewhere": every forced geometry the perm pairing
    plans, it plans too (with the fma pairing or without), and an fma plan fits LDS."""
    max_waves = dict(ic.variant_ks())
    no_plan, planned, fma_plans = [], 0, 0
    for K in ic.KS:
        for G in ic.WIDTHS:
            for W in (0, 4, 8, 12, 16):
                if W > max_waves[K]:
                    continue
                for passes in (1, 2):
                    lq = ic.single_lq(K, G) if passes == 1 else ic.multi_lq(K, G, 2, K)
                    p1, p0, p2 = (db.debug_plan_forced(lq, K, G, W, form=2, f16_pair=fp) for fp in (1, 0, 2))
                    if not p1["planned"]:
                        assert not p2["planned"] and not p0["planned"], (K, G, W, passes)
                        continue
                    planned += 1
                    if not p2["planned"]:
                        no_plan.append((K, G, W, passes))
                        continue
                    assert (p2["K"], p2["G"], p2["passes"]) == (K, G, passes) and (W == 0 or p2["W"] == W), (K, G, W, passes, p2)
                    assert p2["lds_bytes"] <= ic.LDS and p0["lds_bytes"] <= ic.LDS, (K, G, W, passes, p2, p0)
                    fma_plans += p2["fma"]
                    # (f16_pair = 1 is untouched by any of this: never the fma pairing)
                    assert p1["fma"] == 0 and p1["lds_bytes"] <= ic.LDS, (K, G, W, passes, p1)
                    # where the model ranks both pairings and picks fma, asking for fma gives that plan
                    if p0["fma"]:
                        assert p2["fma"] == 1, (K, G, W, passes, p0, p2)
    assert not no_plan, "f16_pair = 2 leaves %d of %d forced geometries without a plan: %s ..." % (len(no_plan), planned, no_plan[:12])
    # (at least: every K at every width in one pass and in two with the workgroup size left free; the fma pairing at least
    # where the matrix's single-pass fma cases have it)
    assert planned >= 2 * len(ic.KS) * len(ic.WIDTHS), planned
    assert fma_plans >= sum(c["family"] == "f16_fma_single" for c in ic.cases()), fma_plans


def test_inputs_have_what_the_cases_rely_on(db):
    flat, off = ic.database()
    lens = np.diff(off).astype(np.int64)
    assert len(lens) == ic.DB_COUNT and len(lens) % 2 == 1 and lens.max() <= ic.MAX_LEN
    assert set(range(0, 10)) <= set(lens.tolist())                 # an empty record, lengths 1 .. 9
    short = np.nonzero((lens >= 1) & (lens <= 4))[0]
    pairs = [p for p in ic.pairs_by_rank(db.order()) if len(p) == 2]
    assert len(pairs) == ic.DB_COUNT // 2
    for c in ic.cases():
        t = ic.truth(c)
        assert t.shape == (ic.DB_COUNT,) and t[lens == 0].max() == 0, c["id"]
        assert t[short].max() > 0, c["id"]
        if c["form"] in (2, 3) and c["lq"] >= 40:
            flagged = t >= ic.F16_CEILING
            assert flagged.any() and (~flagged).any(), c["id"]
            assert any(flagged[a] != flagged[b] for a, b in pairs), c["id"]
        if c["form"] == 1:
            assert ((t >= ic.I16_CEILING) & (t <= ic.WIDE_CEILING)).any(), (c["id"], int(t.max()))
        if c["form"] == 0 and c["bits"] == 16:
            assert t.max() < ic.I16_CEILING, c["id"]                # plain int16 cells: nothing saturates, nothing is run again


def test_every_lane_local_column_decides_a_score():
    """An instantiation that computed one of its K columns per lane wrongly (say, left the odd K's last column out of the
    running best) must change a score the main fill reports: for every case and every lane-local column -- k = 0 .. K - 1 of
    the passes on K columns, and those of a last pass on a K of its own -- some sequence below the cells' ceiling has all its
    best cells in that column.  The column-resolved truth is numpy's (instantiation_cases.column_best), held against the
    oracle here for every case.

    Not the exact int32 cases: their gap scores are positive (that is what selects those cells), so every alignment gains
    by running on and each sequence's best cell lies in the query's last few columns, whatever the sequences are."""
    n = 0
    for c in ic.cases():
        if c["exact"]:
            continue
        assert np.array_equal(ic.case_column_best(c).max(axis=1), ic.truth(c)), c["id"]
        classes = set(range(c["K"] + c["last_k"]))
        assert set(np.unique(ic.column_classes(c)).tolist()) == classes, c["id"]
        missing = classes - ic.pinned_classes(c)
        assert not missing, (c["id"], sorted(missing))
        n += 1
    assert n > 350
