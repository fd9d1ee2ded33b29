"""GPU (-m gpu): no call's answer depends on the calls made before it (tests/call_order_cases.py: PROBES, MOVERS, Session).

include/swg.h promises that a call's answer is a function of its arguments and of the context's scoring, query and
options.  Between calls a context keeps eight profile slots, the colmax and k-mer tables, a calibration database, the
batches16 cache, staging buffers and search slots; a handle keeps its tuned geometries, plans, layouts, the bin image, two
hints and the both-forms cut; two switches are process-wide.  Each is dropped by a key written by hand, and a key that
misses something shows up as a wrong answer only after the right call before it.

Everything here runs on a context of its own at default options, autotune ON, with the handles resident for the module:
never on the session's ctx, which the movers would leave in a state other modules do not expect.  Every probe's answer
is the CPU's truth exactly (outputs pre-filled: what a call must not write is part of it); the only tolerances are
test_gpu_pssm_build._assert_same's for a built PSSM and evalue_cases.REL for lambda, mu and K, both imported.  A failure
names the pair and lists every call since the context was made."""
import numpy as np
import pytest

import call_order_cases as co
import db_kinds_cases as dk
from test_gpu_pssm_build import _assert_same

pytestmark = pytest.mark.gpu

WALK_STEPS = 150


@pytest.fixture(scope="module")
def session(swg, orc):
    co.all_truths()
    s = co.Session(swg, _assert_same)
    try:
        yield s
    finally:
        try:
            s.close()
        finally:
            co.reset_process_wide(swg)


@pytest.mark.parametrize("mover", list(co.MOVERS))
def test_probe_after(session, mover):
    """mover, probe for every probe: every ordered pair adjacent once.  A mover that changes what the context holds (the
    query, the scoring) has the probe in front of it as well, so that what the probe remembered is there to go stale."""
    s = session
    for probe in co.PROBES:
        if mover in co.STATE_MOVERS:
            s.run_probe(probe)
        s.run_mover(mover)
        s.run_probe(probe)


def test_the_movers_moved_what_they_claim(session):
    """Every mover that is named after a route or an option runs once more here, at 130 columns under -11 / -1, and what
    swg_stats, swg_prune_last and the pruning's test hooks report must be the route it is named for: an option whose
    reader does not read it moves nothing."""
    s = session
    s.set_state(1, 0, False, 0)
    for mover in ["two-class search", "several-pass search", "systolic search", "search relatives", "fixed-streams search"] + list(co.OPTION_MOVERS):
        s.run_mover(mover)
    ev = s.evidence
    assert any(e["long_pairs"] > 0 and e["engine"] == 2 for e in ev["two_class"]), ev["two_class"]
    assert all(e["passes"] > 1 and e["engine"] == 2 for e in ev["several_pass"]), ev["several_pass"]
    assert all(e["engine"] == 1 for e in ev["systolic"]), ev["systolic"]
    assert all(e["work_queue"] == 0 for e in ev["fixed streams"]), ev["fixed streams"]
    # the first search on the f16 cells alone flags all 64; the second, under the veto, runs on the int16 cells
    first, second = ev["relatives"]
    assert first == (2, co.N_RELATIVES) and second[0] in (0, 1), ev["relatives"]
    assert ev["relatives, heavy"][1] > 0 or ev["relatives, heavy"][0] == 1, ev["relatives, heavy"]     # past 32767: the wide form, or a re-score
    # the options of a plain search
    assert ev["work_queue", 0]["work_queue"] == 0 and ev["force_bits", 32]["path_bits"] == 32 and ev["force_bits", 16]["path_bits"] == 16, ev
    assert ev["f16", 0]["cell_form"] == 0 and ev["f16", 2]["cell_form"] == 2 and ev["q32_waves", 8]["path_bits"] == 32, ev
    assert ev["last_pass", 0]["passes"] > 1 and ev["last_pass", 0]["last_pass_cols"] == 0, ev["last_pass", 0]
    assert ev["segment_blocks", 4096]["fill_launches"] > ev["segment_blocks", 4096]["passes"] > 1, ev["segment_blocks", 4096]
    assert ev["long_helps", 1]["long_pairs"] > 0 and ev["wide16", 0]["cell_form"] not in (1, 4), (ev["long_helps", 1], ev["wide16", 0])
    # the options of a pruned search: each one's reader was pruned, by the table, segments, width, gate and levels asked for
    pruned = {m[:2]: ev[m[:2]] for m in co.OPTION_MOVES if m[3] == "pruned"}
    assert len(pruned) == 13 and all(e["pruned"] and e["passes"] == 1 for e in pruned.values()), pruned
    assert pruned["prune_kmer", 4]["k"] == 4 and pruned["prune_kmer", 5]["k"] == 5, pruned
    assert (pruned["prune_segments", 8]["k"], pruned["prune_segments", 8]["segments"]) == (4, 8), pruned["prune_segments", 8]
    assert pruned["prune_table_bits", 16]["bits"]["first4"] == 16, pruned["prune_table_bits", 16]
    assert pruned["prune_gate", 2]["gate"] and not pruned["prune_gate", 1]["gate"], (pruned["prune_gate", 2], pruned["prune_gate", 1])
    assert pruned["prune_refine", 64]["refine"] == 64 and pruned["prune_refine", 1]["refine"] == 0, (pruned["prune_refine", 64], pruned["prune_refine", 1])
    assert pruned["prune_refine3", 256]["refine3"] == 256 and pruned["prune_refine3", 256]["refine"] == 128, pruned["prune_refine3", 256]
    for level in ("refine4", "refine5"):                             # (1.32 GB tables: a context that cannot have one searches without)
        e = pruned["prune_" + level, 5256][level]
        assert e[level] == 256 or e["refused"], (level, e)
    assert pruned["prune_cut", 1]["refine"] == 0, pruned["prune_cut", 1]
    s.set_state(0, 0, False, 0)                                      # 40 columns: the near-copies lie behind the unpruned head
    for probe in ("hits_only[tunable]", "hits_only_kmer[tunable]"):
        s.run_probe(probe)
    for key in ("hits_only", "hits_only_kmer"):                      # (the sum of the residues' best scores is too loose to cut here)
        last = s.stats[key, "tunable"]
        assert last["pruned"] and last["threshold"] >= co.truth("tunable", 0, 0, 0).max() // 2, (key, last)
        assert last["pairs_skipped"] > 0 or key == "hits_only", (key, last)


def _tuned_search(s, what):
    st = s.search("tunable", what)
    return tuple(st[k] for k in co.PLAN_FIELDS)


def test_a_tuned_handle_under_changed_options(swg, orc):
    """A default search of tunable at each length fills db->tuned; then every option of the mover list is changed in turn
    with the entries in place, then the scoring and the query's content, and every search must give the oracle's scores
    and top-K.  (The entries are keyed by length, cell form, pairing and gapless alone.)"""
    co.all_truths()
    s = co.Session(swg, _assert_same)
    try:
        tuned = {}
        for li in range(3):
            s.set_state(li, 0, False, 0)
            s.log.append("default search at %d columns" % co.LENS[li])
            tuned[li] = _tuned_search(s, "the tuning search")
            assert _tuned_search(s, "the search after it") == tuned[li]          # the tuned plan is kept
        for key, away, default in [m[:3] for m in co.OPTION_MOVES] + list(co.PROCESS_WIDE):
            s.option(key, away)                                      # the option alone, the entries replayed under it
            try:
                for li in range(3):
                    s.set_state(li, 0, False, 0)
                    s.log.append("%s = %d, %d columns" % (key, away, co.LENS[li]))
                    s.search("tunable", "a tuned handle under %s = %d" % (key, away))
            finally:
                s.option(key, default)
            name = "%s = %d" % (key, away)                              # then the call that reads it, and the entries again
            s.run_mover(name)
            for li in range(3):
                s.set_state(li, 0, False, 0)
                s.log.append("after %s, %d columns" % (name, co.LENS[li]))
                assert _tuned_search(s, "a tuned handle after %s" % name) == tuned[li], s.where("the tuned plan after %s" % name)
        for li, ci, pssm, si in ((0, 1, False, 0), (1, 1, False, 0), (2, 1, False, 0), (2, 1, True, 0), (2, 1, True, 1), (2, 0, False, 1),
                                 (1, 0, True, 1), (0, 0, False, 1), (0, 0, False, 0), (2, 0, False, 0)):
            s.set_state(li, ci, pssm, si)
            s.log.append("state %r" % ((li, ci, pssm, si),))
            s.search("tunable", "a tuned handle after set_query / set_scoring")
        for li in range(3):                                                       # and the entries are what they were
            s.set_state(li, 0, False, 0)
            assert _tuned_search(s, "back at the defaults") == tuned[li], s.where("the tuned plan at %d columns" % co.LENS[li])
    finally:
        s.close()
        co.reset_process_wide(swg)


def test_a_tuned_two_class_entry_under_changed_options(swg, orc):
    """tunable's tuned entries have one class (the cost model offers it nothing else); `tailed` gets a bulk and a long
    class at 130 columns.  Its entry is tuned by a default search and then replayed under the options a two-class plan is
    measured with -- long_helps, work_queue, the pairing, the cells, the batch -- beside a forced split, which goes past
    the entry, and under another content and a PSSM.  The oracle's scores and top-K every time, and
    the tuned plan again once everything is back."""
    s = co.Session(swg, _assert_same)
    try:
        db = swg.Database(*s.c["tailed"]).upload(s.ctx)
        s.db["tailed"] = db
        s.set_state(1, 0, False, 0)
        s.ctx.set_option("autotune", 0)
        s.log.append("the model's plan")
        model = s.search("tailed", "autotune 0")
        assert model["long_pairs"] > 0 and model["engine"] == 2, model      # (what the tuner's first candidate is)
        s.ctx.set_option("autotune", 1)
        s.log.append("the tuning search")
        tuned = tuple(s.search("tailed", "the tuning search")[k] for k in co.PLAN_FIELDS)
        print("tuned plan of tailed:", dict(zip(co.PLAN_FIELDS, tuned)))
        for key, away, default in (("long_helps", 1, 0), ("work_queue", 0, 1), ("long_split", -1, 0), ("long_split", 1500, 0), ("f16", 0, 1),
                                   ("f16_pair", 1, 0), ("f16_pair", 2, 0), ("batch", 1, 8), ("prio_share", 50, 150), ("last_pass", 0, 1),
                                   ("side_readout", 0, 1)):
            s.option(key, away)
            try:
                s.log.append("%s = %d" % (key, away))
                s.search("tailed", "a tuned two-class entry under %s = %d" % (key, away))
            finally:
                s.option(key, default)
            s.log.append("defaults again")
            assert tuple(s.search("tailed", "defaults after %s" % key)[k] for k in co.PLAN_FIELDS) == tuned, s.where("the tuned plan after %s" % key)
        for li, ci, pssm, si in ((1, 1, False, 0), (1, 1, True, 0), (1, 0, True, 0), (1, 0, False, 0)):
            s.set_state(li, ci, pssm, si)
            s.log.append("state %r" % ((li, ci, pssm, si),))
            st = s.search("tailed", "a tuned two-class entry after set_query / set_scoring")
        assert tuple(st[k] for k in co.PLAN_FIELDS) == tuned, s.where("the tuned plan at the end")
    finally:
        s.close()
        co.reset_process_wide(swg)


def _plans(s):
    """The plan fields of every probe that reports stats, at every length, on both handles."""
    out = {}
    for li in range(3):
        s.set_state(li, 0, False, 0)
        for probe in ("search[tunable]", "hits_only[tunable]", "search_gapless[tunable]"):
            s.run_probe(probe)
        for key in (("search", "tunable"), ("hits_only", "tunable"), ("search_gapless", "tunable")):
            out[key + (co.LENS[li],)] = {k: s.stats[key][k] for k in co.PLAN_FIELDS}
    return out


def test_plan_does_not_depend_on_history(swg, orc):
    """autotune 0, on tunable, where no score reaches 4096 and so neither hint moves: after every mover has run once, the
    plan of every probe is the plan a fresh context makes on a freshly packed and uploaded handle."""
    co.all_truths()
    old, fresh = co.Session(swg, _assert_same, autotune=0), None
    try:
        for mover in co.MOVERS:
            old.run_mover(mover)
        after = _plans(old)
        fresh = co.Session(swg, _assert_same, autotune=0)
        first = _plans(fresh)
        assert sorted(after) == sorted(first)
        for key in first:
            assert after[key] == first[key], old.where("the plan of %s at %d columns after every mover: %r, fresh: %r" % (
                key[0], key[2], after[key], first[key]))
    finally:
        old.close()
        if fresh:
            fresh.close()
        co.reset_process_wide(swg)


def test_the_veto_goes_with_the_epoch(swg, orc):
    """The two hints swg_host_internal.h documents as "plans of later searches only" are the only history a plan reads:
    on relatives the second search of a query runs under the veto, and set_query -- the same bytes -- ends it."""
    s = co.Session(swg, _assert_same, autotune=0)
    try:
        db, want = s.db["relatives"], dk.ByIndex(co.relatives_truth(False).astype(np.int32))
        s.ctx.set_query(s.c["qrel"])
        forms = []
        for n in range(4):
            if n == 2:
                s.ctx.set_query(s.c["qrel"])
            got, st = dk._search_raw(s.e, db, s.lib.swg_search, co.K)
            dk.same(got["scores"], want, "relatives, search %d" % n, None)
            forms.append(st["cell_form"])
        assert forms[0] == 2 and forms[1] != 2 and forms[2] == 2 and forms[3] != 2, forms
    finally:
        s.close()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_walks(swg, orc, seed):
    """150 calls drawn from the movers and the probes; the message of a failure holds the walk so far, and the seed
    repeats it."""
    co.all_truths()
    s = co.Session(swg, _assert_same)
    try:
        co.walk(s, np.random.default_rng(seed), WALK_STEPS)
    finally:
        s.close()
        co.reset_process_wide(swg)
