"""GPU (-m gpu): align_bounds* and align_stats* on sequences of 2^19 to 2^20 residues (swg_bounds.hip).

swg_bounds_kernel and swg_stats_kernel keep every position -- a state's origin, a lane's best cell and its origin, lane
0's border hand-overs -- as row << 12 | column in one 32-bit register that goes through DPP moves and shuffles as an int.
From row 2^19 on that register's sign bit is set; the host hands a sequence of SWG_BOUNDS_LEN = 2^20 residues or more to
the traceback's kernel.  The cases of long_rows_cases.py (proved by test_long_rows_cases_host.py) put best cells, origins,
ties, step counts and scores above 2^19 and a pair on either side of 2^20.

Every comparison is on all seven bounds fields and all eleven stats fields against the int32 oracle's traceback
(orc.pair_trace), computed once per case and shared; nothing is filtered or tolerated."""
import numpy as np
import pytest

import long_rows_cases as lc
from long_rows_cases import HALF, LIMIT

pytestmark = pytest.mark.gpu

BOUNDS = ("score", "index", "q_begin", "q_end", "d_begin", "d_end", "n_ops")
COUNTS = ("n_ident", "n_match", "n_gap_open", "n_gap")
FIELDS = BOUNDS + COUNTS
TRACED = [n for n in lc.NAMES if max(len(q) for q in lc.case(n)["queries"]) <= 129]   # also run through the traceback
PATHS = ["limit", "every_row_path_gaps_2_1", "every_row_path_gaps_0_1"]


@pytest.fixture(scope="module")
def lctx(swg):
    c = swg.Context(0)
    c.set_option("autotune", 0)
    yield c
    c.close()


_truth = {}


def truth(orc, name):
    """What the oracle says of a case, computed once: per query, per hit, (the eleven fields as a dict, the path)."""
    if name not in _truth:
        c = lc.case(name)
        rows = []
        for q, row in zip(c["queries"], c["hits"]):
            out = []
            for i in row:
                d = c["seqs"][i]
                sc, co, ops = orc.pair_trace(q, d, c["sub"], c["gap_open"], c["gap_extend"])
                want = (sc, i, co[0], co[1], co[2], co[3], len(ops)) + lc.counts_of(q, d, co[0], co[2], ops)
                out.append((dict(zip(FIELDS, want)), ops))
            rows.append(out)
        _truth[name] = rows
    return _truth[name]


def want_stats(orc, name):
    return [[a for a, _ in row] for row in truth(orc, name)]


def want_bounds(orc, name):
    return [[{f: a[f] for f in BOUNDS} for a, _ in row] for row in truth(orc, name)]


class Resident:
    """A case's sequences as a resident database under the case's scoring."""

    def __init__(self, swg, ctx, c):
        self.c, self.ctx = c, ctx
        ctx.set_scoring(c["sub"], c["gap_open"], c["gap_extend"])
        self.db = swg.Database(*lc.packed(c)).upload(ctx)
        self.hits = [[(0, i) for i in row] for row in c["hits"]]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.db.close()


def routed(last):
    return last["kernel_pairs"], last["fallback_pairs"], last["launches"]


# ---- 1. every case through the two batch calls, against the oracle --------------------------------------------------------
@pytest.mark.parametrize("name", lc.NAMES)
def test_bounds_and_stats_of_every_case(swg, orc, lctx, name):
    c = lc.case(name)
    pairs = sum(len(r) for r in c["hits"])
    with Resident(swg, lctx, c) as r:
        got_b = lctx.align_bounds_multi(r.db, c["queries"], r.hits)
        last_b = lctx.debug_bounds_last()
        got_s = lctx.align_stats_multi(r.db, c["queries"], r.hits)
        last_s = lctx.debug_bounds_last()
    assert all(tuple(a) == BOUNDS for row in got_b for a in row) and all(tuple(a) == FIELDS for row in got_s for a in row)
    assert got_b == want_bounds(orc, name)
    assert got_s == want_stats(orc, name)
    # one launch per geometry used and no pair on the fallback -- but the limit case's second sequence, of SWG_BOUNDS_LEN
    # residues, which is the fallback's first
    want = (1, 1, 1) if name == "limit" else (pairs, 0, len(set(c["geometries"])))
    assert routed(last_b) == want and routed(last_s) == want, (last_b, last_s)
    flat = [a for row in got_s for a in row]
    if c["rows"] == "high":
        assert all(a["d_begin"] >= HALF and a["n_gap_open"] >= 1 and a["n_ident"] < a["n_match"] for a in flat)
    if c["rows"] == "straddle":
        assert all(a["d_begin"] < HALF <= a["d_end"] for a in flat)
    if c["rows"] == "tie":
        assert all(a["d_end"] < HALF for a in flat)                        # the low copy, not the high one
    if c["rows"] == "every":
        assert all(min(a["score"], a["n_ops"], a["d_end"], a["n_gap"]) > HALF for a in flat)
    if c["rows"] == "limit":
        assert [a["d_end"] for a in flat] == [LIMIT - 1, LIMIT]


# ---- 2. the traceback's kernel on the same pairs --------------------------------------------------------------------------
@pytest.mark.parametrize("name", TRACED)
def test_bounds_equal_the_traceback_without_paths(swg, orc, lctx, name):
    c = lc.case(name)
    with Resident(swg, lctx, c) as r:
        walked = lctx.align_hits_multi(r.db, c["queries"], r.hits, want_ops=False)
        assert lctx.align_bounds_multi(r.db, c["queries"], r.hits) == walked
        lctx.set_query(c["queries"][0])
        assert lctx.align_bounds(r.db, r.hits[0]) == lctx.align_hits(r.db, r.hits[0], want_ops=False) == walked[0]
    assert walked == want_bounds(orc, name)


@pytest.mark.parametrize("name", PATHS)
def test_traceback_spells_the_oracle_s_path(swg, orc, lctx, name):
    """swg_trace_kernel over 2^19 to 2^20 anti-diagonals, best cells with bj >= 2^19, paths of more than 2^19 steps."""
    c = lc.case(name)
    with Resident(swg, lctx, c) as r:
        lctx.set_query(c["queries"][0])
        got = lctx.align_hits(r.db, r.hits[0])
    want = [dict({f: a[f] for f in BOUNDS}, ops=ops) for a, ops in truth(orc, name)[0]]
    assert got == want
    assert all(a["d_end"] >= HALF and len(a["ops"]) == a["n_ops"] for a in got)


# ---- 3. the PSSM instantiations ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["high_16x4", "high_64x16", "tie_across_sign_32x8"])
def test_pssm_of_the_table_s_rows_gives_the_index_results(swg, orc, lctx, name):
    c = lc.case(name)
    pssms = [lc.pssm_of(c, i) for i in range(len(c["queries"]))]
    # the table's diagonal is each row's strict maximum, so the PSSM's consensus is the query: the identity counts agree
    assert all(np.array_equal(np.argmax(p[:, 1:32], axis=1) + 1, q) for p, q in zip(pssms, c["queries"]))
    with Resident(swg, lctx, c) as r:
        got_b = lctx.align_bounds_multi_pssm(r.db, pssms, r.hits)
        last_b = lctx.debug_bounds_last()
        got_s = lctx.align_stats_multi_pssm(r.db, pssms, r.hits)
        last_s = lctx.debug_bounds_last()
    assert got_b == want_bounds(orc, name) and got_s == want_stats(orc, name)
    assert routed(last_b) == routed(last_s) == (1, 0, 1)


# ---- 4. a long pair, then a one-residue pair, then a score-0 pair, through one lane group ------------------------------------
def test_after_a_long_pair_in_one_group(swg, orc, lctx):
    name = "after_a_long_pair"
    c = lc.case(name)
    with Resident(swg, lctx, c) as r:
        lctx.set_query(c["queries"][0])
        lctx.set_option("bounds_groups", 1)
        try:
            got_b = lctx.align_bounds(r.db, r.hits[0])
            last_b = lctx.debug_bounds_last()
            got_s = lctx.align_stats(r.db, r.hits[0])
            last_s = lctx.debug_bounds_last()
        finally:
            lctx.set_option("bounds_groups", 0)
    assert [got_b] == want_bounds(orc, name) and [got_s] == want_stats(orc, name)
    assert routed(last_b) == routed(last_s) == (3, 0, 1)
    assert got_s[0]["d_begin"] >= HALF
    assert tuple(got_s[1][f] for f in FIELDS) == (3, 1, got_s[1]["q_begin"], got_s[1]["q_begin"] + 1, 0, 1, 1, 1, 1, 0, 0)
    assert tuple(got_s[2][f] for f in FIELDS if f != "index") == (0,) * 10


# ---- 5. several alignments of a long pair --------------------------------------------------------------------------------
def test_hsps_of_a_long_pair(swg, orc, lctx):
    """high_16x4's pair with max_hsps 3 and min_score 1: the oracle's alignment at the high rows, then the decoy at the
    low rows; the whole answer is the host twin's, field for field, with paths and counts."""
    name = "high_16x4"
    c = lc.case(name)
    q, d = c["queries"][0], c["seqs"][0]
    twin = swg.align_hsps_host(c["sub"], c["gap_open"], c["gap_extend"], d, 3, 1, query=q, want_counts=True)
    with Resident(swg, lctx, c) as r:
        lctx.set_query(q)
        got = lctx.align_hsps(r.db, r.hits[0], 3, 1, want_counts=True)
    assert got == [twin] and len(twin) == 3
    first, ops = truth(orc, name)[0][0]
    assert got[0][0] == dict(first, ops=ops) and got[0][0]["d_begin"] >= HALF
    row, piece = c["decoy"]
    second = got[0][1]
    assert (second["score"], second["q_begin"], second["q_end"], second["d_begin"], second["d_end"], second["ops"]) == \
        (3 * len(piece), 0, len(piece), row, row + len(piece), "M" * len(piece))


# ---- 6. a view -----------------------------------------------------------------------------------------------------------
def test_limit_pair_through_a_view_in_swapped_order(swg, orc, lctx):
    name = "limit"
    c = lc.case(name)
    with Resident(swg, lctx, c) as r:
        view = r.db.view(lctx, [1, 0])
        swapped = [[(0, 1), (0, 0)]]
        got_b = lctx.align_bounds_multi(view, c["queries"], swapped)
        last = lctx.debug_bounds_last()
        got_s = lctx.align_stats_multi(view, c["queries"], swapped)
        view.close()
    assert got_b == [want_bounds(orc, name)[0][::-1]] and got_s == [want_stats(orc, name)[0][::-1]]
    assert [a["index"] for a in got_b[0]] == [1, 0] and routed(last) == (1, 1, 1)
