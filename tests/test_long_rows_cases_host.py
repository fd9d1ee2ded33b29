"""CPU: every case of long_rows_cases.py is what it claims, by the int32 oracle's traceback (orc.pair_trace); the GPU half
(test_gpu_long_rows.py) then runs them on the device.  Also here, without a device: the kernels' best-cell reduction
restated, which shows that the tie cases tell an unsigned compare of the packed positions from a signed one."""
import os

import numpy as np
import pytest

import long_rows_cases as lc
from conftest import ROOT
from long_rows_cases import HALF, LIMIT


def trace(orc, c, q, d):
    return orc.pair_trace(q, d, c["sub"], c["gap_open"], c["gap_extend"])


def without(d, piece):
    """The sequence with a planted piece overwritten by junk."""
    row, residues = piece
    out = d.copy()
    out[row:row + len(residues)] = lc.JUNK
    return out


def test_the_constants_are_the_library_s():
    text = open(os.path.join(ROOT, "seq-align-gpu_amd", "csrc", "swg_host_internal.h")).read()
    assert "#define SWG_BOUNDS_LEN (1u << 20)" in text and LIMIT == 1 << 20 and HALF == LIMIT // 2
    assert (HALF << 12) & 0xFFFFFFFF == 1 << 31 and ((HALF - 1) << 12 | 0xFFF) < 1 << 31       # the first row with bit 31 set
    assert [c["name"] for c in lc.all_cases()] == lc.NAMES


@pytest.mark.parametrize("name", lc.NAMES)
def test_query_lengths_select_the_geometry_named(name):
    c = lc.case(name)
    for q, g in zip(c["queries"], c["geometries"]):
        assert g == next((G, K) for G, K in [(16, 4), (16, 8), (32, 8), (64, 8), (64, 16)] if len(q) <= G * K)
        assert all(1 <= int(r) <= 20 for r in q)
    assert all(lc.geometry_of(lq) == g and lc.geometry_of(lq - 1) != g for g, lq in lc.SMALLEST_LQ.items() if lq != 60)
    assert lc.geometry_of(60) == (16, 4) and lc.geometry_of(1025) is None
    if name.startswith(("high_", "tie_")):
        G, K = (int(x) for x in name.rsplit("_", 1)[1].split("x"))
        assert c["geometries"] == [(G, K)] and len(c["queries"][0]) == lc.SMALLEST_LQ[(G, K)]
    assert all(HALF <= len(s) <= LIMIT for s in c["seqs"] if len(s) > 1)


@pytest.mark.parametrize("G,K", lc.GEOMETRIES)
def test_high_cases(orc, G, K):
    c = lc.case("high_%dx%d" % (G, K))
    q, d = c["queries"][0], c["seqs"][0]
    assert len(d) == HALF + 300 + len(q) and c["copy"][0] == HALF + 200
    sc, co, ops = trace(orc, c, q, d)
    ident, n_match, n_gap_open, n_gap = lc.counts_of(q, d, co[0], co[2], ops)
    assert co[2] >= HALF and co[2] == c["copy"][0] and co[3] == c["copy"][0] + len(q) - 1       # bpos and borg: bit 31 set
    assert (co[0], co[1]) == (0, len(q)) and n_gap_open >= 1 and ident < n_match and len(ops) == len(q)
    assert sc == 3 * (len(q) - 2) - 2 - 5                    # a mismatch, and one deleted residue at (-4, -1)
    lsc, lco, _ = trace(orc, c, q, without(d, c["copy"]))    # the decoy alone
    assert 0 < lsc < sc and lsc == 3 * (len(q) // 2) and lco[2] == 100 and lco[3] < HALF


def test_straddle_case(orc):
    c = lc.case("straddle")
    q, d = c["queries"][0], c["seqs"][0]
    sc, co, ops = trace(orc, c, q, d)
    assert co[2] < HALF <= co[3] and co == (0, len(q), HALF - 30, HALF - 30 + len(q)) and sc == 3 * len(q) and ops == "M" * len(q)
    assert (co[2] + 1) << 12 < 1 << 31 <= co[3] << 12        # the origin's word has bit 31 clear, the best cell's has it set


@pytest.mark.parametrize("G,K", [(16, 4), (32, 8), (64, 16)])
def test_tie_cases(orc, G, K):
    c = lc.case("tie_across_sign_%dx%d" % (G, K))
    q, d = c["queries"][0], c["seqs"][0]
    S = 3 * lc.TIE_STRETCH
    low, high = c["low"], c["high"]
    assert len(low[1]) == len(high[1]) == lc.TIE_STRETCH and not np.array_equal(low[1], high[1])
    assert low[0] + lc.TIE_STRETCH < HALF < high[0]
    for piece in (low, high):                                # each stretch alone scores S
        assert trace(orc, c, q, lc.planted(64, [(20, piece[1])]))[0] == S
    (la, lb), (ha, hb) = c["low_columns"], c["high_columns"]
    sc, co, ops = trace(orc, c, q, d)                        # the pair: S, at the low coordinates
    assert (sc, co, ops) == (S, (la, lb, low[0], low[0] + lc.TIE_STRETCH), "M" * lc.TIE_STRETCH)
    sc, co, ops = trace(orc, c, q, without(d, low))          # without the low copy: S, at the high coordinates
    assert (sc, co, ops) == (S, (ha, hb, high[0], high[0] + lc.TIE_STRETCH), "M" * lc.TIE_STRETCH)
    assert (lb - 1) // K != (hb - 1) // K and lb > hb        # end columns of different lanes; the low copy's is the higher


def test_every_row_path_cases(orc):
    a, b = lc.case("every_row_path_gaps_2_1"), lc.case("every_row_path_gaps_0_1")
    for c in (a, b):
        assert len(c["queries"][0]) == 8 and len(c["seqs"][0]) == HALF + 77 and len(set(c["seqs"][0].tolist())) == 1
    assert (a["sub"] == -100).all() and (a["gap_open"], a["gap_extend"]) == (2, 1)
    sc, co, ops = trace(orc, a, a["queries"][0], a["seqs"][0])
    assert (sc, len(ops)) == (524298, 524371) == (a["score"], a["n_ops"]) and ops.startswith("DIDIDI")
    assert co[3] == HALF + 77 and co[2] <= 1 and co[0] == 0          # in from the border, through every row
    assert np.array_equal(b["sub"], lc.simple_table(3, -2)) and (b["gap_open"], b["gap_extend"]) == (0, 1)
    sc, co, ops = trace(orc, b, b["queries"][0], b["seqs"][0])
    assert (sc, len(ops)) == (524381, 524365) == (b["score"], b["n_ops"]) and ops.startswith("MIII")
    assert co == (0, 8, 0, HALF + 77)
    assert min(a["score"], a["n_ops"], b["score"], b["n_ops"]) > HALF


def test_limit_case(orc):
    c = lc.case("limit")
    q = c["queries"][0]
    assert [len(s) for s in c["seqs"]] == [LIMIT - 1, LIMIT] and len(q) == 8
    for d in c["seqs"]:
        sc, co, ops = trace(orc, c, q, d)
        assert (sc, co, ops) == (24, (0, 8, len(d) - 8, len(d)), "M" * 8)          # d_end == len: the last row and column
        lsc, lco, _ = trace(orc, c, q, without(d, (len(d) - 8, q)))                # the decoy alone
        assert 0 < lsc < sc and lco[2] == 10


def test_after_a_long_pair_case(orc):
    c = lc.case("after_a_long_pair")
    h = lc.case("high_16x4")
    q = c["queries"][0]
    assert np.array_equal(q, h["queries"][0]) and np.array_equal(c["seqs"][0], h["seqs"][0])
    assert [len(s) for s in c["seqs"][1:]] == [1, 1] and c["hits"] == [[0, 1, 2]]
    assert trace(orc, c, q, c["seqs"][1])[0] == 3 and trace(orc, c, q, c["seqs"][2]) == (0, (0, 0, 0, 0), "")


# ---- the fault the tie cases are aimed at, shown without a device --------------------------------------------------------
@pytest.mark.parametrize("G,K", [(16, 4), (32, 8), (64, 16)])
def test_a_signed_compare_would_pick_the_high_copy(G, K):
    """The two candidates of a tie case as the lanes hold them (score, end row, end column; from 1) through the kernels'
    reduction restated in long_rows_cases.best_cell: compared as uint32 the low copy wins, as the rule and the oracle say;
    compared as int32 the high one would, and the GPU test of the case would fail."""
    c = lc.case("tie_across_sign_%dx%d" % (G, K))
    S = 3 * lc.TIE_STRETCH
    low = (S, c["low"][0] + lc.TIE_STRETCH, c["low_columns"][1])
    high = (S, c["high"][0] + lc.TIE_STRETCH, c["high_columns"][1])
    for order in ([low, high], [high, low]):
        assert lc.best_cell(order, signed=False) == low
        assert lc.best_cell(order, signed=True) == high
    # an arithmetic shift in the unpacking would turn a high row negative
    word = np.array([high[1] << 12 | high[2]], dtype=np.uint32)
    assert int(word[0] >> 12) == high[1] and int(word.view(np.int32)[0] >> 12) < 0
