"""CPU: the inputs of tests/above_multi_cases.py are what the GPU tests of swg_search_above_multi rely on.  Every
condition is re-proved from the oracle: the thresholds, how many hits they leave, that no two rows or thresholds of the
batch can be swapped unnoticed, that one chunk holds more keys than a single search's key buffer starts with, that a pruned
search skips pairs for every query, and that the batch is admitted to the one launch."""
import numpy as np
import pytest

import above_multi_cases as amc
import gapless_cases as gc


@pytest.fixture(scope="module")
def case(swg, orc):
    sub = amc.table(swg)
    flat, off, qA = amc.database(swg)
    qs = amc.queries(swg, qA)
    truths = [orc.score_db(q, flat, off, sub, amc.GO, amc.GE) for q in qs]
    return dict(sub=sub, flat=flat, off=off, qs=qs, truths=truths, T=amc.level_table(truths))


def test_the_batch(case):
    qs = case["qs"]
    assert [len(q) for q in qs] == [200, 81, 1, 77, 150] and len(qs) % 2 == 1
    assert np.array_equal(qs[1], qs[0][60:141]) and np.array_equal(qs[2], qs[0][:1])
    assert len(case["off"]) - 1 == amc.N and len(amc.LEVELS) == 5


def test_tenth_best_thresholds_and_their_hits(case):
    tenth = [t[2] for t in case["T"]]
    assert tenth == [985, 393, 5, 89, 142] and len(set(tenth)) == 5
    hits = [len(amc.above(tr, t)) for tr, t in zip(case["truths"], tenth)]
    assert hits == [10, 10, 3795, 10, 10]             # (the one-residue query ties massively: the index order decides)
    one = amc.above(case["truths"][2], 5)
    assert len({s for s, _ in one}) <= 2 and [i for _, i in one[:50]] == sorted(i for _, i in one[:50])


def test_levels(case):
    for tr, t in zip(case["truths"], case["T"]):
        assert len(amc.above(tr, t[0])) == 0 and len(amc.above(tr, t[1])) >= 1
        assert len(amc.above(tr, t[3])) >= amc.N // 2 and t[4] == 1 and min(t) >= 1
    assert amc.mixed(case["T"]) == [case["T"][i][i] for i in range(5)]


def test_no_swap_of_rows_or_thresholds_can_pass(case):
    truths, tenth = case["truths"], [t[2] for t in case["T"]]
    for i in range(5):
        own = amc.above(truths[i], tenth[i])
        for j in range(5):
            if i == j:
                continue
            assert amc.above(truths[i], tenth[j]) != own, (i, j)      # query i under query j's threshold
            assert amc.above(truths[j], tenth[i]) != own, (i, j)      # query j's row under query i's threshold
    mixed = amc.mixed(case["T"])
    answers = [amc.above(truths[i], mixed[i]) for i in range(5)]
    assert all(answers[i] != answers[j] for i in range(5) for j in range(i))


def test_one_chunk_holds_more_keys_than_a_searchs_buffer_starts_with(case):
    total = sum(len(amc.above(tr, 1)) for tr in case["truths"])
    assert total == 19995 and total > 8192


def test_a_pruned_search_skips_pairs_for_every_query(swg, case):
    order = amc.sorted_order(case["off"])
    skipped = []
    for q, t in zip(case["qs"], case["T"]):
        b = amc.pair_order_bounds(swg, case["sub"], q, case["flat"], case["off"], order)
        assert len(b) == amc.N // 2
        skipped.append(int((b < t[2]).sum()))
    assert skipped == [1861, 1233, 2, 1, 272]


def test_gapless_thresholds(orc, case):
    g = [gc.oracle_gapless(orc, q, case["flat"], case["off"], case["sub"]) for q in case["qs"]]
    T = amc.level_table(g)
    assert [t[2] for t in T] == [985, 393, 5, 37, 38]
    assert [len(amc.above(tr, t[2])) for tr, t in zip(g, T)] == [10, 10, 3795, 10, 11]


def test_the_batch_is_admitted_to_one_launch(swg, case):
    db = swg.Database(case["flat"], case["off"])
    for form in (2, 0):
        plan = db.debug_plan_batch(200, 5, form=form)
        assert plan["batch"] and plan["classes"] in (1, 2), plan
    assert db.debug_plan_batch(200, 5, form=2)["qq"]                  # two queries per lane: the fifth is paired with itself
    assert not db.debug_plan_batch(200, 1)["batch"]                   # (a batch of one is a single search)
    db.close()
