"""CPU: the generator of the pruned-search fuzz (tests/prune_fuzz_cases.py) -- the slice is pinned byte for byte, holds
every value of every dimension, says "pruned" exactly where swg_prune_plan does, forces only levels a context builds, and
on a sample of every case's sequences every level's host mirror is at least the oracle's score, so a device search built on
those bounds may cut nothing the oracle would report.

Measured on 16 CPUs: the whole file 13 s, of which the mirrors against the oracle (MIRROR_CASES: every case of the slice,
MIRROR_SEQUENCES sequences of each, every level it runs) 10 s, the slowest case 1.7 s."""
import numpy as np
import pytest

import prune_fuzz_cases as pc

SEED, COUNT = pc.SLICE
SLICE_DIGEST = "c825b918a17c29f69ee35b78dc8e8fd63d2079120c7388becb16e98bcf87d54e"
MIRROR_CASES = tuple(range(COUNT))
MIRROR_SEQUENCES = 400


@pytest.fixture(scope="module")
def cases(swg):
    return [pc.case(SEED, i) for i in range(COUNT)]


def test_the_slice_is_pinned(cases):
    for i in (0, 7, COUNT - 1):
        again = pc.case(SEED, i)
        assert pc.digest(again) == pc.digest(cases[i]), i
        assert np.array_equal(again["flat"], cases[i]["flat"]) and again["options"] == cases[i]["options"]
    assert pc.digest(pc.case(SEED + 1, 0)) != pc.digest(cases[0])
    assert pc.slice_digest() == SLICE_DIGEST


def test_every_value_of_every_dimension_occurs(cases):
    seen = {
        "table": ({c["table_name"] for c in cases}, pc.TABLES),
        "gaps": ({(c["gap_open"], c["gap_extend"]) for c in cases}, pc.GAPS),
        "query kind": ({c["query_kind"] for c in cases}, pc.QUERY_KINDS),
        "lq": ({len(c["query"]) for c in cases}, pc.LQS),
        "family": ({c["family"] for c in cases}, pc.FAMILIES),
        "segments": ({c["segments"] for c in cases}, pc.SEGMENTS),
        "f16": ({c["options"]["f16"] for c in cases}, pc.F16),
        "k": ({a for c in cases for a in c["k_asks"]}, pc.K_ASKS),
    }
    for key, vals in pc.LEVELS.items():
        seen[key] = ({c["options"][key] for c in cases}, vals)
    for name, (got, want) in seen.items():
        assert got == set(want), (name, sorted(set(want) - got, key=str))
    # the fourth level's table is 1.32 GB per new query: at most one case in eight forces it
    assert 1 <= sum(c["options"]["prune_refine4"] == 5256 for c in cases) <= COUNT // 8


def test_cases_stay_within_their_limits(cases):
    for c in cases:
        n, lq = len(c["off"]) - 1, len(c["query"])
        assert 600 <= n <= 4000 and lq * len(c["flat"]) <= pc.MAX_CELLS, pc.describe(c)
        assert pc.query_bound(c["table"], c["query"]) <= pc.I16_CEILING        # one cell form
        assert c["flat"].min() >= 1 and c["flat"].max() <= 31 and c["query"].min() >= 1 and c["query"].max() <= 31
        assert pc.lengths(c).min() >= 1
        if c["pssm"] is not None:
            assert np.array_equal(c["pssm"], c["table"][c["query"].astype(np.int64)])
        got = pc.n_segments(pc.lengths(c), lq, c["options"]["segment_blocks"])
        if lq > pc.PASS_COLUMNS:
            assert {"one": got == 1, "two": got == 2, "many": got >= 5}[c["segments"]], (pc.describe(c), got)
        else:
            assert got == 1
    # the families are what they say
    by = {f: [c for c in cases if c["family"] == f] for f in pc.FAMILIES}
    assert all(len(set(pc.lengths(c))) == 1 for c in by["equal"])
    assert all(np.sum(pc.lengths(c) >= 900) == 60 and np.sum(pc.lengths(c) <= 4) == len(c["off"]) - 61 for c in by["long_short"])
    assert all(set(pc.lengths(c)) <= {4 * nb - 3 for nb in pc.EDGE_BLOCKS} for c in by["chunk_edges"])
    assert all(c["flat"].max() > 20 for c in by["odd_residues"])
    for c in by["copies"]:
        o = c["off"].astype(np.int64)
        first = c["flat"][o[0]:o[1]]
        same = sum(np.array_equal(c["flat"][o[j]:o[j + 1]], first) for j in range(len(o) - 1))
        assert same >= (len(o) - 1) // 3
    assert any(len(set(pc.lengths(c))) == 1 and c["family"] == "copies" for c in cases)


def _members(c):
    """The whole database, the random view and the two halves a sharding could make: (lengths of the members)"""
    lens = pc.lengths(c)
    yield lens
    yield lens[pc.view_members(c).astype(np.int64)]
    yield lens[0::2]
    yield lens[1::2]


def test_expect_pruned_is_the_planners_answer(swg, cases):
    n_true = n_false = 0
    for c in cases:
        lq, seg = len(c["query"]), c["options"]["segment_blocks"]
        for lens in _members(c):
            whole = len(lens) == len(c["off"]) - 1
            ask = dict(mode=2, gap_open=c["gap_open"], gap_extend=c["gap_extend"], bits=16 if pc.structural(c) else 32,
                       range_pairs=(len(lens) + 1) // 2, n_segments=pc.n_segments(lens, lq, seg))
            ks = list(c["ks"]) + [len(lens) - 1, len(lens), len(lens) + 5]
            for k in ks:
                for groups in (64, 1024, 8192):
                    for want_scores in (0, 1):
                        got = swg.debug_prune_plan(k=k, want_scores=want_scores, groups=groups, prune_head=4, **ask)[0]
                        assert got == pc.pruned_topk(c, lens, k), (pc.describe(c), len(lens), k, groups)
                if whole and k in c["expect_pruned"]["topk"]:
                    assert c["expect_pruned"]["topk"][k] == pc.pruned_topk(c, lens, k)
                    n_true += c["expect_pruned"]["topk"][k]
                    n_false += not c["expect_pruned"]["topk"][k]
            for groups in (64, 8192):
                assert swg.debug_prune_plan_above(groups=groups, **ask)[0] == pc.pruned_above(c, lens), pc.describe(c)
            if whole:
                assert c["expect_pruned"]["above"] == pc.pruned_above(c, lens)
    # both answers occur, and "not pruned" for both reasons: the positive gap point, and a k that leaves no rest
    assert n_true > COUNT and n_false >= 3
    assert any(not pc.structural(c) for c in cases)
    assert any(pc.structural(c) and not all(c["expect_pruned"]["topk"].values()) for c in cases)


def test_forced_levels_are_ones_a_context_builds(swg, cases):
    ran = set()
    for c in cases:
        o = c["options"]
        for route in ("topk", "above"):
            r = pc.realised(swg, c, route)
            assert r["admitted"], pc.describe(c)
            if o["prune_kmer"] in (1, 4, 5):
                assert r["k"] == o["prune_kmer"]
            if r["k"] > 1 and o["prune_segments"] >= 1:
                assert r["S"] == o["prune_segments"]
            cut = route == "topk" and o["prune_cut"] == 1
            assert r["S2"] == (o["prune_refine"] if o["prune_refine"] in (64, 128) and not cut else 0)
            assert r["S3"] == (256 if o["prune_refine3"] == 256 and not cut else 0)
            assert r["gate"] == (o["prune_gate"] == 2 and r["k"] > 1 and r["S"] > 1 and not cut)
            if pc.structural(c):
                ran |= {("k", r["k"]), ("S", r["S"]), ("S2", r["S2"]), ("S3", r["S3"]), ("S4", r["S4"]), ("gate", r["gate"])}
    # every level the slice forces is run by some case that is pruned
    assert ran >= {("k", 1), ("k", 4), ("k", 5), ("S", 8), ("S", 16), ("S", 32), ("S2", 64), ("S2", 128), ("S3", 256), ("S4", 256),
                   ("gate", True)}, ran


def _mirrors(swg, c, flat, off):
    """(name, bound per sequence) of every level the case's searches run, from the host mirrors"""
    rows, q = (c["pssm"], None) if c["pssm"] is not None else (c["table"], c["query"])
    go, ge = c["gap_open"], c["gap_extend"]
    out = [("colmax", swg.debug_prune_bound(rows, q, flat, off)[1])]
    r = pc.realised(swg, c, "above")
    if r["k"] > 1 and r["S"] == 1:
        out.append(("kmer %d" % r["k"], swg.debug_prune_kmer(rows, q, go, ge, r["k"], flat, off, table=False)[1]))
    elif r["k"] > 1:
        out.append(("kmer %d in %d" % (r["k"], r["S"]), swg.debug_prune_kmer_seg(rows, q, go, ge, r["k"], r["S"], flat, off, table=False)[1]))
    for S in (r["S2"], r["S3"]):
        if S:
            out.append(("refine %d" % S, swg.debug_prune_kmer_refine(rows, q, go, ge, S, flat, off, table=False)[1]))
    if r["S4"]:
        out.append(("refine4", swg.debug_prune_kmer_refine4(rows, q, go, ge, r["S4"], flat, off)))
    return out


@pytest.mark.parametrize("i", MIRROR_CASES)
def test_every_forced_mirror_is_at_least_the_oracle(swg, orc, cases, i):
    c = cases[i]
    if not pc.structural(c):
        return   # (positive gap scores: no bound holds, and nothing is pruned)
    n = len(c["off"]) - 1
    rng = np.random.default_rng([SEED, i, 1])
    pick = np.sort(rng.choice(n, size=min(n, MIRROR_SEQUENCES), replace=False))
    o = c["off"].astype(np.int64)
    flat = np.concatenate([c["flat"][o[j]:o[j + 1]] for j in pick]).astype(np.int8)
    off = np.concatenate([[0], np.cumsum(np.diff(o)[pick])]).astype(np.uint64)
    want = orc.score_db(c["query"], flat, off, c["table"], c["gap_open"], c["gap_extend"]).astype(np.int64)
    levels = _mirrors(swg, c, flat, off)
    for name, u in levels:
        u = u.astype(np.int64)
        bad = np.flatnonzero(u < want)
        assert len(bad) == 0, (pc.describe(c), name, pick[bad[:5]], u[bad[:5]], want[bad[:5]])
    print(i, c["table_name"], (c["gap_open"], c["gap_extend"]), len(c["query"]), [name for name, _ in levels], "best", int(want.max()))
