"""CPU: the batch instantiation matrix of tests/batch_instantiation_cases.py is complete, the batch planners answer every
one of its cases as the case intends (hooks swg_debug_plan_batch / swg_debug_plan_lists: the geometry rules plan_batch and
plan_lists themselves run), and the inputs have the properties tests/test_gpu_batch_instantiations.py relies on -- all
against the int32 oracle, no device involved."""
import collections

import numpy as np
import pytest

import batch_instantiation_cases as bc
import instantiation_cases as ic
import swg_loader

HALVES_DISAGREE = 0.5      # the two halves of the first pair differ on more than this share of the sequences


@pytest.fixture(scope="module")
def swg():
    return swg_loader.load()


@pytest.fixture(scope="module")
def db(swg):
    flat, off = ic.database()
    d = swg.Database(flat, off)
    yield d
    d.close()


def _plan(db, c, batch_geometry=1):
    if c["lists"]:
        return db.debug_plan_lists(bc.lists(c), c["lq"], form=c["form"], cols=c["K"], group=c["G"], batch_geometry=batch_geometry)
    return db.debug_plan_batch(c["lq"], bc.N_QUERIES, form=c["form"], qq=bool(c["options"]["qq"]), cols=c["K"], group=c["G"],
                               batch_geometry=batch_geometry)


def test_every_batch_instantiation_has_a_case():
    """An entry added to SWG_DIAG_VARIANTS without batch cases fails here, and so does a K taken out of the matrix."""
    ks = sorted(k for k, _ in ic.variant_ks())
    assert ks == list(bc.KS), "SWG_DIAG_VARIANTS changed: extend the batch matrix"
    missing = bc.required(ks) - bc.held()
    assert not missing, sorted(missing)
    have = collections.defaultdict(set)
    for c in bc.cases():
        have[c["family"]].add((c["K"], c["G"]))
    # two queries per lane: every K at 16 and at 32 lanes; at 64 lanes every K is a case of one family or the other
    for G in (16, 32):
        assert {k for k, g in have["qq"] if g == G} == set(ks), G
    assert {k for k, g in have["qq"] | have["qq_fallback"] if g == 64} == set(ks)
    assert all(g == 64 for _, g in have["qq_fallback"])
    # every K meets a width in the rotated families, every width ten K or more
    for fam in ("batch_f16", "batch_i16", "lists_f16", "lists_i16"):
        assert {k for k, _ in have[fam]} == set(ks), fam
        widths = collections.Counter(g for _, g in have[fam])
        assert set(widths) == set(ic.WIDTHS) and min(widths.values()) >= 10, (fam, widths)


def test_no_score_bound_reaches_the_f16_ceiling(swg):
    """The cells of a batch are the options' choice only where no query's score bound reaches the f16 cells' 4096: the
    bound is at most (rows of the longest sequence, in whole 4-row blocks) x (the table's largest entry)."""
    _, off = ic.database()
    lens = np.diff(off).astype(np.int64)
    assert len(lens) == ic.DB_COUNT == 151 and lens.max() <= ic.MAX_LEN == 300
    sub = np.asarray(ic.table(swg, bc.SCORING), dtype=np.int64)
    rows = (int(lens.max()) + 3) // 4 * 4
    assert rows * int(sub[1:, 1:].max()) < ic.F16_CEILING, (rows, int(sub.max()))
    assert bc.GAPS == (-11, -1)
    for c in bc.cases():
        assert bc.truth(c).max() < ic.F16_CEILING, c["id"]


def test_batches_have_the_queries_the_cases_rely_on():
    for c in bc.cases():
        qs = bc.queries(c)
        K, G, lq, n = c["K"], c["G"], c["lq"], c["n2"]
        assert len(qs) == bc.N_QUERIES >= 5 and len(qs) % 2 == 1, c["id"]
        # one pass, the group's last lane partly filled
        assert (G - 1) * K < lq < G * K and lq % K != 0 and len(qs[0]) == lq, c["id"]
        assert np.array_equal(qs[0], ic.query()[:lq]) and np.array_equal(qs[1], ic.query()[bc.SHIFT:bc.SHIFT + n]), c["id"]
        # query 1: shorter, ends inside a lane, the second longest -- the other half of the first pair
        assert n < lq and n % K != 0 and len(qs[1]) == n > max(len(x) for x in qs[2:]), c["id"]
        assert len(qs[2]) == 1 and len(qs[3]) != len(qs[4]) and min(len(qs[3]), len(qs[4])) > 1, c["id"]
        pairs = bc.pairs_of(c)
        assert pairs[0] == (0, 1) and set(pairs[1]) == {3, 4} and pairs[2] == (2, 2), (c["id"], pairs)
        assert all(len(qs[a]) != len(qs[b]) for a, b in pairs[:2]), c["id"]
        if c["lists"]:
            ls = bc.lists(c)
            assert len(ls) == len(qs) and len(set(x.tobytes() for x in ls)) == len(ls), c["id"]
            assert np.array_equal(np.sort(ls[0]), np.arange(ic.DB_COUNT)), c["id"]
            assert len(ls[1]) % 2 == 1 and len(ls[2]) == 1 and len(ls[3]) == 0, c["id"]
            pins = set(bc.sweep_indices())
            assert pins <= set(ls[1].tolist()) and pins <= set(ls[4].tolist()), c["id"]
            assert set(ls[1].tolist()) != set(ls[4].tolist()) and all(len(np.unique(x)) == len(x) for x in ls), c["id"]


def test_batch_planners_answer_every_case_as_intended(db):
    """With batch_geometry = 1 the forced (K, lanes) is what the batch launches, on two queries per lane exactly where
    the case says so; with batch_geometry = 0 the same options send every case one by one, as they always did."""
    n, counts, refused = 0, collections.Counter(), []
    for c in bc.cases():
        p = _plan(db, c)
        assert p["batch"] and p["classes"] == 1, (c["id"], p)
        assert (p["K"], p["G"], p["qq"]) == (c["K"], c["G"], c["qq"]), (c["id"], p)
        assert 0 < p["lds_bytes"] <= ic.LDS and p["per_cu"] >= 1 and p["W"] in (4, 8, 12, 16), (c["id"], p)
        assert not _plan(db, c, batch_geometry=0)["batch"], c["id"]
        if c["family"] == "qq_fallback":
            refused.append(c["K"])
            # with the pairs switched off it is the same launch
            q = db.debug_plan_batch(c["lq"], bc.N_QUERIES, form=2, qq=False, cols=c["K"], group=c["G"], batch_geometry=1)
            assert q == p, (c["id"], p, q)
        counts[c["family"]] += 1
        n += 1
    # the hook decides which K the pairs' profile refuses at 64 lanes; this is what it answers today
    assert sorted(refused) == [k for k in bc.KS if k > bc.QQ_LDS_MAX_K_AT_64], refused
    assert counts == {"qq": 2 * len(bc.KS) + len(bc.KS) - len(refused), "qq_fallback": len(refused), "batch_f16": len(bc.KS),
                      "batch_i16": len(bc.KS), "lists_f16": len(bc.KS), "lists_i16": len(bc.KS)}, counts
    assert n == len(bc.cases()) == 7 * len(bc.KS)


def test_batch_geometry_keeps_the_planners_other_rules(db):
    """A forced geometry the rules refuse ends on the one-by-one route: a query that needs two passes of it, a batch of
    one query, a geometry that does not exist; and a geometry left free is planned as without the option."""
    K, G = 5, 32
    assert not db.debug_plan_batch(G * K + 1, 5, cols=K, group=G, batch_geometry=1)["batch"]
    assert db.debug_plan_batch(G * K, 5, cols=K, group=G, batch_geometry=1)["batch"]
    assert not db.debug_plan_batch(G * K - 1, 1, cols=K, group=G, batch_geometry=1)["batch"]
    assert not db.debug_plan_batch(30, 5, cols=33, group=G, batch_geometry=1)["batch"]
    ls = [np.arange(ic.DB_COUNT), np.arange(3)]
    assert not db.debug_plan_lists(ls, G * K + 1, cols=K, group=G, batch_geometry=1)["batch"]
    assert not db.debug_plan_lists([[], []], 20, cols=K, group=G, batch_geometry=1)["batch"]
    for lq in (1, 64, 65, 200, 367, 1152, 1153):
        assert db.debug_plan_batch(lq, 5, batch_geometry=1) == db.debug_plan_batch(lq, 5, batch_geometry=0), lq
        assert db.debug_plan_lists(ls, lq, batch_geometry=1) == db.debug_plan_lists(ls, lq, batch_geometry=0), lq
    # one lane or the other forced alone is a forced geometry too
    assert db.debug_plan_batch(100, 5, group=16, batch_geometry=1)["G"] == 16
    assert not db.debug_plan_batch(100, 5, group=16, batch_geometry=0)["batch"]


def test_every_lane_local_column_of_both_halves_decides_a_score():
    """What makes the GPU test able to fail.  An instantiation that computed one of its K columns per lane wrongly -- in
    one half of the lanes' registers only, say -- must change a score the batch reports: for every case, for each of the
    two QUERY-derived queries (the two halves of the qq cases' first pair) and every lane-local column k = 0 .. K - 1, some
    sequence has all its best cells in that column of that query; for the lists cases, some sequence of that query's own
    list.  The column-resolved truth is numpy's (instantiation_cases.column_best, per query), held against the oracle bit
    for bit.  (The other three queries are one residue and random residues: they check the pairing and the hand-over of
    unequal lengths, no planted copy pins their columns.)"""
    n = 0
    for c in bc.cases():
        t = bc.truth(c)
        for i in (0, 1):
            best = bc.query_column_best(c, i)
            assert best.shape == (ic.DB_COUNT, len(bc.queries(c)[i])), c["id"]
            assert np.array_equal(best.max(axis=1), t[i]), (c["id"], i)
            among = bc.lists(c)[i] if c["lists"] else None
            missing = set(range(c["K"])) - bc.pinned_columns(c, i, among)
            assert not missing, (c["id"], i, sorted(missing))
            n += 1
    assert n == 2 * len(bc.cases())


def test_the_halves_of_the_first_pair_disagree():
    """A kernel that swapped or merged the two queries of a lane would report one half's scores for the other: the two
    halves of the first pair (queries 0 and 1) differ on more than half of the sequences in every case, by the oracle
    alone; the least share over the matrix is 0.53 (K = 2 at 16 lanes, where the window is half the prefix)."""
    least = 1.0
    for c in bc.cases():
        t = bc.truth(c)
        share = float((t[0] != t[1]).mean())
        assert share > HALVES_DISAGREE, (c["id"], share)
        least = min(least, share)
        # ... and the second pair's too, and the hits differ
        assert float((t[3] != t[4]).mean()) > HALVES_DISAGREE, c["id"]
    assert least > HALVES_DISAGREE


def test_an_empty_list_gets_no_workgroup(db):
    for c in bc.cases():
        if not c["lists"] or c["K"] % 8:
            continue
        p = _plan(db, c)
        deal = db.debug_list_deal(bc.lists(c), p["W"] * (64 // p["G"]), 256 * p["per_cu"])
        rows = set(int(r) for r in deal[:, 0])
        assert rows == {0, 1, 2, 4}, (c["id"], rows)
