"""CPU: the world of tests/db_kinds_cases.py is what tests/test_gpu_db_kinds.py relies on.  Conditions, not measurements:
the seed and the planted ranks are chosen so that every one of them holds.  The kinds that need no device (everything
but views and masked copies) are packed here and their count, total_count and order() compared with the cases' member
sets; a view's and a masked copy's members follow from their base's by definition and are pinned on the device."""
import os
import re

import numpy as np
import pytest

import db_kinds_cases as dk
from test_gpu_stats import consensus

REQUIRED_KINDS = ["whole", "rank0of3", "rank1of3", "rank2of3", "rank2of7", "rank5of7", "rank6of7", "cut_elsewhere", "view_of_rank1of3",
                  "masked_rank1of3", "view_of_masked_rank1of3", "loaded_rank2of3"]
REQUIRED_FAMILIES = ["search", "search_begin / search_end", "search_multi", "search_multi_pssm", "search_gapless", "search_gapless_multi",
                     "search_gapless_multi_pssm", "search_above", "search_gapless_above", "search_above_multi", "search_above_multi_pssm",
                     "search_gapless_above_multi", "search_gapless_above_multi_pssm", "search_lists", "composition", "align_hits",
                     "align_hits_multi", "align_hits_multi_pssm", "align_bounds", "align_bounds_multi", "align_bounds_multi_pssm", "align_stats",
                     "align_stats_multi", "align_stats_multi_pssm", "align_hsps, max_hsps 1", "align_hsps", "align_hsps_multi",
                     "align_hsps_multi_pssm", "pssm_build", "pssm_build_multi", "pssm_build_multi_pssm", "sequence"]
RANKS_OF_3 = ("rank0of3", "rank1of3", "rank2of3")


@pytest.fixture(scope="module")
def w(swg, orc):
    return dk.world()


def test_the_world(w):
    assert dk.N == 677 and len(w["lens"]) == 677 and dk.GAPS == (-11, -1)
    assert [len(q) for q in w["queries"]] == [40, 130, 600]
    lens = w["lens"]
    assert int(lens.min()) == 1 and sorted(lens.tolist())[-3:] == [1500, 2200, 3000] and int(np.sort(lens)[-4]) <= 615
    by_rank = lens[w["order"]]
    assert (np.diff(by_rank) <= 0).all()
    bins = [by_rank[b * 128:(b + 1) * 128] for b in range(6)]
    assert [len(b) for b in bins] == [128] * 5 + [37]
    assert bins[0].min() >= 600 and bins[1][5:].max() <= 300           # the first bin is far longer than the rest
    assert bins[5].max() <= 12 and bins[4].min() <= 12                 # the last bins are a tail of lengths 1 .. 12
    assert 90000 <= int(lens.sum()) <= 140000
    for q, p in zip(w["queries"], w["pssms"]):                         # the PSSM twin: the same scores, the query its own consensus
        assert np.array_equal(p, w["sub"][q.astype(np.int64)]) and np.array_equal(consensus(p), q)


def test_the_tables_hold_every_kind_and_family():
    assert list(dk.KINDS) == REQUIRED_KINDS
    names = [f.name for f in dk.FAMILIES]
    assert len(set(names)) == len(names) and not set(REQUIRED_FAMILIES) - set(names)
    for f in dk.FAMILIES:
        assert f.takes_hits == f.name.startswith(("align_", "pssm_build")), f.name
    assert dk.KINDS["cut_elsewhere"].n_total == 100000 and int(dk.elsewhere(3)) == 7 + 131 * 3


def test_no_case_is_left_out_or_skipped():
    import test_gpu_db_kinds as gpu
    here = os.path.dirname(os.path.abspath(__file__))
    for name in ("db_kinds_cases.py", "test_db_kinds_cases_host.py", "test_gpu_db_kinds.py"):
        text = open(os.path.join(here, name)).read()
        assert not re.search(r"pytest\.(skip|xfail|importorskip)|mark\.(skip|xfail)", text), name
    marks = [m for m in gpu.test_every_family_on.pytestmark if m.name == "parametrize"]
    assert len(marks) == 1 and marks[0].args[0] == "kind" and list(marks[0].args[1]) == REQUIRED_KINDS
    assert "FAMILIES" in gpu.test_every_family_on.__code__.co_names
    # the merge takes every family with a search result: nothing is named twice, a new row joins by itself
    assert list(dk.MERGED) == [f.name for f in dk.FAMILIES if not f.takes_hits and f.name != "sequence"]
    assert not {n for n in REQUIRED_FAMILIES if n.startswith("search")} - set(dk.MERGED) and "composition" in dk.MERGED


def test_the_top_lists_order_ties_as_the_oracle_does(w, orc):
    everyone = np.arange(dk.N)
    for truths in w["truth"] + w["gapless"]:
        for t in truths:
            for k in (dk.K, dk.TOP, dk.N):
                assert dk._top(t, everyone, k) == [dk.H(*h) for h in orc.topk(t, k)]
    assert any(len(set(s for s, _ in orc.topk(t, dk.N))) < dk.N for t in w["truth"][0])     # (there are ties to order)


@pytest.mark.parametrize("count", [3, 7])
def test_the_merge_of_the_expected_answers_is_the_whole(swg, w, count):
    """The merge of tests/test_gpu_db_kinds.py, fed with what the ranks must answer: it gives the whole database's answer for
    every merged family, and it notices a rank that is missing."""
    import test_gpu_db_kinds as gpu
    kinds = [dk.Kind("rank%dof%d" % (r, count), (r, count)) for r in range(count)]
    whole = dk.KINDS["whole"]
    for f in dk.FAMILIES:
        if f.name in dk.MERGED:
            parts = [dk.expected(f, k) for k in kinds]
            gpu._merge(swg, parts, dk.expected(f, whole), f.name)
            with pytest.raises(AssertionError):
                gpu._merge(swg, parts[1:], dk.expected(f, whole), f.name)


@pytest.mark.parametrize("name", REQUIRED_KINDS)
def test_a_kinds_handle_holds_the_cases_members(swg, w, name, tmp_path):
    kind = dk.KINDS[name]
    db = kind.pack(swg, w, tmp_path)                                  # (the base: a view or a masked copy is made of it on a device)
    base = kind.base_members(w)
    assert db.count == len(base) and db.total_count == kind.n_total
    assert np.array_equal(np.sort(db.order().astype(np.int64)), kind.g(base))
    assert db.residues == int(w["lens"][base].sum())
    members = kind.members(w)
    assert set(members.tolist()) <= set(base.tolist())
    if kind.view:
        assert np.array_equal(members, np.intersect1d(base, dk.NOT_DIVISIBLE_BY_3)) and 0 < len(members) < len(base)
        assert kind.unselected(w) in kind.g(base).tolist() and kind.unselected(w) not in kind.g(members).tolist()
    else:
        assert np.array_equal(members, base) and kind.unselected(w) is None
    assert kind.outside(w) not in kind.g(base).tolist()
    for i in (members[:3].tolist() + members[-3:].tolist()):
        assert np.array_equal(db.sequence(int(kind.g(i))), w["seqs"][0][i])
    db.close()


def test_the_ranks(w):
    m = {name: kind.members(w) for name, kind in dk.KINDS.items()}
    assert len(m["whole"]) == 677 and len(m["rank5of7"]) == 37 and len(m["rank6of7"]) == 0 and len(m["rank2of7"]) == 128
    assert [len(m[r]) for r in RANKS_OF_3] == [256, 256, 165]
    for count in (3, 7):
        parts = [dk.members_of_rank(w, r, count) for r in range(count)]
        assert np.array_equal(np.sort(np.concatenate(parts)), np.arange(677))
    assert np.array_equal(m["cut_elsewhere"], m["rank1of3"]) and np.array_equal(m["loaded_rank2of3"], m["rank2of3"])
    g = dk.KINDS["cut_elsewhere"].g(m["cut_elsewhere"])
    assert g.max() > 100 * len(g) and (np.diff(g) > 0).all() and g.max() < 100000
    shuffled = m["rank1of3"][w["elsewhere_shuffle"]]                  # no positional link: neither the index nor the length order
    assert (np.diff(shuffled) < 0).any() and (np.diff(w["lens"][shuffled]) > 0).any()


def _rank_of_three(w, i):
    return [n for n, r in enumerate(RANKS_OF_3) if i in set(dk.KINDS[r].members(w).tolist())][0]


@pytest.mark.parametrize("masked", [0, 1])
def test_top_lists_and_thresholds_reach_every_rank(w, masked):
    for tops, levels, truths in ((w["top"][masked], w["levels"][masked], w["truth"][masked]),
                                 (w["gapless_top"][masked], w["gapless_levels"][masked], w["gapless"][masked])):
        for qi in range(3):
            assert len({_rank_of_three(w, i) for _, i in tops[qi][:12]}) >= 2, qi
            above_best, tenth, one = levels[qi]
            assert one == 1 and above_best > tenth > 1
            for r in RANKS_OF_3:
                m = dk.KINDS[r].members(w)
                assert len(dk.amc.above(truths[qi], tenth, m)) >= 1, (qi, r)
                assert len(dk.amc.above(truths[qi], above_best, m)) == 0
                assert len(dk.amc.above(truths[qi], 1, m)) > len(m) // 2


def test_every_kind_but_the_empty_one_has_hits_for_every_query(w):
    for name, kind in dk.KINDS.items():
        rows = dk.hit_rows(w, kind)
        if name in ("rank6of7", "rank5of7"):                          # (nothing, and nothing but the tail of lengths 1 .. 12)
            assert rows == [[], [], []]
        elif name != "rank2of7":
            assert all(len(r) >= 1 for r in rows), (name, rows)
    assert sum(len(r) for r in dk.hit_rows(w, dk.KINDS["rank2of7"])) >= 1


def test_near_copies_reach_the_f16_ceiling_in_two_ranks(w):
    ceiling = dk.f16_ceiling()
    assert ceiling == 4096
    at = np.nonzero(w["truth"][0][2] >= ceiling)[0]
    assert sorted(at.tolist()) == sorted(int(w["order"][r]) for r in dk.NEAR_COPIES)
    assert {_rank_of_three(w, int(i)) for i in at} == {0, 1}
    assert (w["truth"][0][0] < ceiling).all() and (w["truth"][0][1] < ceiling).all()
    holds = {name for name, kind in dk.KINDS.items() if (w["truth"][int(kind.masked)][2][kind.members(w)] >= ceiling).any()}
    assert {"whole", "rank0of3", "rank1of3", "cut_elsewhere", "view_of_rank1of3"} <= holds


def test_paths_with_both_gap_kinds_and_a_pair_of_two_alignments(w):
    for qi in range(3):
        paths = [dk.trace(0, qi, i)["ops"] for _, i in w["top"][0][qi]]
        assert any("I" in p and "D" in p for p in paths), qi
    assert any(len(dk.hsps(0, 1, i, 3)) >= 2 for _, i in w["top"][0][1])
    repeat = int(w["order"][135])
    assert repeat in [i for _, i in w["top"][0][1]] and len(dk.hsps(0, 1, repeat, 3)) >= 2


def test_masking_changes_scores_of_rank_1_of_3(w):
    m = dk.KINDS["rank1of3"].members(w)
    changed = [int((w["truth"][1][qi][m] != w["truth"][0][qi][m]).sum()) for qi in range(3)]
    assert changed[1] >= 3, changed
    assert any(int(i) in m.tolist() for _, i in w["top"][0][1] if w["truth"][1][1][i] != w["truth"][0][1][i])
    assert int(w["masked_residues"][m].sum()) > 0
    assert int(w["masked_residues"].sum()) == w["mask_totals"]["residues_masked"]
    assert int((w["masked_residues"] > 0).sum()) == w["mask_totals"]["sequences_masked"]
    assert int(w["mask_segments"].sum()) == w["mask_totals"]["segments"]


def test_expected_answers_of_the_cut_elsewhere_shard_are_rank_1_of_3_remapped(w):
    cut, rank1 = dk.KINDS["cut_elsewhere"], dk.KINDS["rank1of3"]
    for family in dk.FAMILIES:
        if family.name.startswith("pssm_build"):
            continue                                                  # (arrays of values: compared on the device)
        dk.same(dk.expected(family, cut), dk.remap(dk.expected(family, rank1), cut), family.name, None)
    s = dk.expected(dk.FAMILIES[0], cut)["f16=1"][0]
    assert s["scores"].arr.shape == (100000,) and int((s["scores"].arr != dk.FILL32).sum()) == 256


def test_the_comparison_notices_one_wrong_entry(w):
    """What the GPU test's verdict rests on: one score, one stray write, one hit, one touched slot, one path letter."""
    import copy
    kind = dk.KINDS["rank1of3"]
    by_name = {f.name: f for f in dk.FAMILIES}
    want = dk.expected(by_name["search_multi"], kind)
    dk.same(copy.deepcopy(want), want, "equal", None)
    member, other = int(kind.members(w)[0]), int(dk.KINDS["rank0of3"].members(w)[0])

    def spoiled(change):
        got = copy.deepcopy(want)
        change(got)
        with pytest.raises(AssertionError):
            dk.same(got, want, "spoiled", None)

    def score(got):
        got["scores"].arr[1, member] += 1

    def stray(got):
        got["scores"].arr[2, other] = 0

    def hit(got):
        got["hits"][0][3] = dk.H(got["hits"][0][3].score, got["hits"][0][3].index + 1)

    def tail(got):
        got["tail"] = False

    for change in (score, stray, hit, tail):
        spoiled(change)
    want = dk.expected(by_name["align_hsps_multi"], kind)
    got = copy.deepcopy(want)
    a = got["rows"][1][0][0]
    a["ops"] = a["ops"].replace("I", "D", 1)
    with pytest.raises(AssertionError):
        dk.same(got, want, "spoiled", None)
    got = copy.deepcopy(want)
    got["rows"][1][0].pop()
    with pytest.raises(AssertionError):
        dk.same(got, want, "spoiled", None)
