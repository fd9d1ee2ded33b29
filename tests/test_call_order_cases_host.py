"""CPU: the cases of tests/call_order_cases.py are what they claim to be (no device anywhere here)."""
import numpy as np
import pytest

import above_multi_cases as amc
import call_order_cases as co
import db_kinds_cases as dk


@pytest.fixture(scope="module")
def c(swg, orc):
    return co.cases()


@pytest.fixture(scope="module")
def tunable(swg, c):
    db = swg.Database(*c["tunable"])
    yield db
    db.close()


def test_tunable_is_the_least_the_tuner_takes_and_its_lengths_plan_apart(swg, c, tunable):
    """plan_search tunes a handle of 4096 to 4 M sequences.  The three query lengths get three different geometries, so
    db->tuned holds three different entries per cell form.

    The cost model offers ONE class at all three lengths, the 600-column query included: a long class pays where the
    bulk's work per SIMD is of the order of the longest chain (1500 rows x 130 instructions: 0.9 M cycles), which at 600
    columns takes some 12 M residues -- 2900 a sequence at this count, where tunable's are mostly 8 to 90 and hold 0.2 M.
    A tuned entry of two classes is `tailed`'s (test_tailed_gets_two_classes_from_the_cost_model); on tunable and the
    world the two-class route is the forced mover's (long_split 1000)."""
    assert tunable.count == co.N_TUNABLE == 4096 + 37
    lens = np.diff(c["tunable"][1].astype(np.int64))
    assert int((lens >= 700).sum()) == co.N_LONG and lens.max() <= 1500 and lens.min() >= 8
    assert int(((lens >= 8) & (lens <= 90)).sum()) == co.N_TUNABLE - co.N_LONG
    for pair in (None, 0):
        plans = [tunable.debug_plan(lq, f16_pair=pair) for lq in co.LENS]
        assert all(p["classes"] == 1 and p["long_pairs"] == 0 and p["passes"] == 1 for p in plans), plans
        assert len({(p["K"], p["G"]) for p in plans}) == 3, plans


def test_tailed_gets_two_classes_from_the_cost_model(swg, c):
    """At 130 columns, on the int16 and on the f16 cells: the entry the tuner stores for it holds a bulk and a long class."""
    db = swg.Database(*c["tailed"])
    try:
        assert db.count == co.N_TAILED >= 4096
        for pair in (None, 0):
            p = db.debug_plan(130, f16_pair=pair)
            assert p["classes"] == 2 and p["long_pairs"] > 100 and p["passes"] == 1, p
    finally:
        db.close()


def test_no_score_on_tunable_reaches_the_f16_ceiling(c):
    """So neither hint (sat_hint, f16_veto_epoch) ever moves on it: what test_plan_does_not_depend_on_history relies on."""
    for li in range(3):
        for ci in range(2):
            for si in range(2):
                assert 0 < co.truth("tunable", li, ci, si).max() < dk.f16_ceiling(), (li, ci, si)


def test_the_second_scoring_keeps_the_f16_cells_off(c):
    """swg_f16_gaps_ok: both gap magnitudes at most 2048; the packed int16 cells take a first gap position up to 32767."""
    go, ge = co.SCORINGS[1]
    assert 2048 < -(go + ge) <= 32767 and -(co.SCORINGS[0][0] + co.SCORINGS[0][1]) <= 2048


def test_relatives_cross_the_veto_rule_and_both_ceilings(c):
    """f16 cells flag a pair when one of its two sequences reaches 4096 (tests/test_f16_cells_model.py: flagged exactly
    then); the veto rule of swg_search_end's bookkeeping: the flagged pairs' rows are more than 1/16 of all pair rows."""
    t, off = co.relatives_truth(False), c["relatives"][1]
    assert len(t) == co.N_RELATIVES and (t >= dk.f16_ceiling()).all() and t.max() < 32767
    lens = np.diff(off.astype(np.int64))
    order = amc.sorted_order(off)
    pairs = [order[i:i + 2] for i in range(0, len(order), 2)]        # two sequences of neighbouring ranks share a lane
    rows = np.array([2 + lens[p].max() for p in pairs])
    flagged = np.array([(t[p] >= dk.f16_ceiling()).any() for p in pairs])
    assert rows[flagged].sum() * 16 > rows.sum()
    heavy = co.relatives_truth(True)
    assert heavy.max() >= 32767 and heavy.max() < 65535 and int(c["heavy"].max()) == 55 and int(c["heavy"].min()) == -20


@pytest.mark.parametrize("si", [0, 1])
def test_the_hits_only_probes_prune(swg, c, tunable, si):
    """prune 2, hits and no scores, one class off the work queue: swg_prune_plan says pruned, and the head it runs unpruned
    is shorter than the range, so there is something left to cut."""
    go, ge = co.SCORINGS[si]
    for name, n in (("tunable", co.N_TUNABLE), ("world", dk.N)):
        pairs = (n + 1) // 2
        pruned, head = swg.debug_prune_plan(mode=2, k=co.K, want_scores=0, gap_open=go, gap_extend=ge, n_classes=1, range_pairs=pairs, groups=64,
                                            n_segments=1)
        assert pruned and 0 < head < pairs, (name, pruned, head)
        assert not swg.debug_prune_plan(mode=1, k=co.K, want_scores=0, gap_open=go, gap_extend=ge, range_pairs=pairs, groups=64, n_segments=1)[0]


def test_a_stale_kmer_table_would_cut_true_hits(swg, c):
    """What makes hits_only_kmer[tunable] notice a k-mer table that outlived its query.  A pruned search of one segment
    fills its longest pairs unpruned -- 256 or 516 of them here, by the lane groups resident -- and cuts the rest by the
    K-th best score of that head.  At 40 columns the head holds N_HEAD relatives, so the threshold is high; the N_DEEP
    near-copies lie far behind it, belong to the K best, and the OTHER content's table bounds each of them below the
    threshold, where the query's own table bounds every sequence at or above its score."""
    flat, off = c["tunable"]
    order = amc.sorted_order(off)
    rank = np.empty(len(order), dtype=np.int64)
    rank[order] = np.arange(len(order))
    for ci in range(2):
        for si in range(2):
            t = co.truth("tunable", 0, ci, si)
            best = np.array([i for _, i in co.top("tunable", 0, ci, si, k=co.K)])
            deep = best[rank[best] >= 2 * 516]
            assert len(deep) == co.N_DEEP and (rank[best[rank[best] < 2 * 516]] < 2 * 256).all(), rank[best]
            T = min(int(np.sort(t[order[:2 * pairs]])[-co.K]) for pairs in (256, 516))
            own = swg.debug_prune_kmer(c["sub"], c["queries"][0][ci], *co.SCORINGS[si], 4, flat, off, table=False)[1]
            stale = swg.debug_prune_kmer(c["sub"], c["queries"][0][1 - ci], *co.SCORINGS[si], 4, flat, off, table=False)[1]
            assert (own.astype(np.int64) >= t).all()
            assert T > 100 and (stale[deep].astype(np.int64) < T).all(), (ci, si, T, stale[deep], t[deep])


def test_the_two_contents_of_a_length_differ(c):
    for name in co.DBS:
        for li in range(3):
            assert len(c["queries"][li][0]) == len(c["queries"][li][1]) == co.LENS[li]
            assert c["pssms"][li][0].shape == c["pssms"][li][1].shape == (co.LENS[li], 32)
            for si in range(2):
                a, b = co.truth(name, li, 0, si), co.truth(name, li, 1, si)
                assert not np.array_equal(a, b)
                assert co.top(name, li, 0, si)[0][1] != co.top(name, li, 1, si)[0][1], (name, li, si)
            assert not np.array_equal(co.truth(name, li, 0, 0, True), co.truth(name, li, 1, 0, True))
    for li in range(3):                                               # the two scorings tell apart too, and the mask
        assert not np.array_equal(co.truth("world", li, 0, 0), co.truth("world", li, 0, 1))
    assert not np.array_equal(co.truth("world", 1, 0, 0), co.truth("masked", 1, 0, 0))


def _misplaced(accepted, named, excluded):
    """-> (names a mover uses that swg_set_option does not take, accepted options placed nowhere, excluded ones that are
    not options or are moved all the same)."""
    accepted, named = set(accepted), set(named)
    return sorted(named - accepted), sorted(accepted - named - set(excluded)), sorted((set(excluded) - accepted) | (set(excluded) & named))


def test_every_option_is_placed():
    accepted = co.accepted_options()
    assert _misplaced(accepted, co.option_names(), co.EXCLUDED) == ([], [], [])
    assert all(isinstance(r, str) and r and "\n" not in r for r in co.EXCLUDED.values())
    # the check bites: a misspelt mover, an option nobody placed, an exclusion that is no option
    assert _misplaced(accepted, co.option_names() + ["work_que"], co.EXCLUDED)[0] == ["work_que"]
    assert _misplaced(accepted + ["a_new_option"], co.option_names(), co.EXCLUDED)[1] == ["a_new_option"]
    assert _misplaced(accepted, co.option_names(), dict(co.EXCLUDED, batch="moved"))[2] == ["batch"]
    listed = ("work_queue", "last_pass", "wide16", "f16", "f16_pair", "qq", "long_helps", "batch", "batch_blocks", "batch_geometry", "force_bits",
              "prune", "prune_kmer", "prune_segments", "prune_table_bits", "prune_cut", "above_batch", "side_readout", "prio_share", "q32_waves",
              "long_cols", "long_group", "cols_per_wave", "group_lanes", "long_split", "engine", "calib_seed")
    assert set(listed) <= set(co.option_names())
    for key, away, default in [m[:3] for m in co.OPTION_MOVES] + list(co.PROCESS_WIDE):
        assert away != default, key
    # each option's mover runs a call that reads it: the pruning's options a pruned search, the batch planners' a batch,
    # the int32 launches' an int32 search, the multi-pass fill's several passes, the long class's two classes
    readers = {m[:2]: m[3] for m in co.OPTION_MOVES}
    assert all(r == "pruned" for (key, _), r in readers.items() if key.startswith("prune_")) and set(readers.values()) <= set(co.READERS)
    assert [readers[k] for k in (("qq", 0), ("batch_geometry", 1), ("above_batch", 1), ("above_batch", 2))] == ["multi", "multi", "above_multi", "above_multi"]
    assert (readers["q32_waves", 8], readers["last_pass", 0], readers["segment_blocks", 4096], readers["long_helps", 1], readers["wide16", 0]) == \
        ("int32", "several_pass", "several_pass", "two_class", "heavy")
    assert all(set(m[4]) <= set(co.accepted_options()) for m in co.OPTION_MOVES)


def test_the_tables():
    assert set(co.PROBES) <= set(co.MOVERS) and set(co.STATE_MOVERS) <= set(co.MOVERS)
    assert set(co.IN_FLIGHT_OK) == {"search[tunable]", "search[world]", "search[masked]", "hits_only[tunable]", "hits_only[world]", "hits_only_kmer[tunable]",
                                    "hits_only_kmer[world]"}
    for family in ("search[", "hits_only[", "search_above[", "search_gapless[", "search_multi[", "search_lists["):
        assert {family + n + "]" for n in co.DBS} <= set(co.PROBES)
    assert {"align_hits", "align_bounds", "align_stats", "align_hsps", "pssm_build", "calibrate"} <= set(co.PROBES)


def test_the_truths_take_seconds(swg, orc, c):
    """Every truth the GPU module compares a search with, computed anew: about 0.7 s with the oracle's OpenMP build; the
    bound leaves room for a busy machine and still tells a truth set that has grown out of a test's reach."""
    import time
    co._TRUTH.clear()
    co.relatives_truth.cache_clear()
    t0 = time.perf_counter()
    co.all_truths()
    took = time.perf_counter() - t0
    print("all_truths: %.2f s" % took)
    assert took < 30.0, took


def test_the_alignment_probes_have_something_to_align(c):
    for li in range(3):
        for ci in range(2):
            for si in range(2):
                row = co.hit_row(li, ci, si)
                assert len(row) == co.ROWS == len(set(row))
                assert all(co.trace(li, ci, si, i)["score"] == co.truth("world", li, ci, si)[i] > 0 for i in row)
    assert any(len(co.hsps(1, 0, 0, i)) > 1 for i in co.hit_row(1, 0, 0))      # (db_kinds' repeat: two alignments of one pair)
