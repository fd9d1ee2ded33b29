"""CPU: the host twin with the two options of the PSSM construction, swg_pssm_from_paths_ex(blocks, purge) -- per-column
alignment blocks and the purge of near-identical hits -- against the numpy restatement of pssm_blocks_cases with the
oracle's paths: every case of the whole-query model's host tests under blocks = 1, and the cases that model cannot tell
apart (staggered extents, two domains, a gap inside an extent, columns only the query covers)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import pssm_blocks_cases as bc
import pssm_build_cases as pc
from conftest import ROOT
from test_pssm_build_host import CASES as OLD_CASES

NEW_CASES = ("staggered", "two_domains", "gap_row")
COINCIDE = ("nohits_BLOSUM62", "nohits_BLOSUM45", "nohits_PAM250", "lq1", "family_1", "score0", "query_x")
B62, GAPS = "BLOSUM62", pc.MATRICES["BLOSUM62"]


@functools.lru_cache(maxsize=None)
def _cases():
    import swg_loader
    cases = dict(pc.host_cases(swg_loader.oracle()))
    cases.update(bc.blocks_cases(swg_loader.oracle()))
    return cases


@functools.lru_cache(maxsize=None)
def _twin(name, blocks, purge):
    import swg_loader
    c = _cases()[name]
    return swg_loader.load().pssm_from_paths(c["sub"], c["q"], c["flat"], c["off"], c["al"], freq=c["freq"], pseudocount=c["beta"],
                                             want_values=True, blocks=blocks, purge=purge)


@functools.lru_cache(maxsize=None)
def _restated(name, blocks, purge):
    c = _cases()[name]
    return bc.model_numpy(c["sub"], c["q"], c["flat"], c["off"], c["al"], freq=c["freq"], beta=c["beta"], blocks=blocks, purge=purge)


def _assert_same(got, want, what):
    pssm, values, info = got
    margin = pc.half_integer_margin(want["values"], want["have"])
    worst = float(np.abs(values - want["values"]).max())
    print(what, "rows", info["n_rows"], "purged", info["n_purged"], "Nbar", info["n_distinct"], "worst", worst, "margin", margin)
    assert margin >= 1e-6, "a value within 1e-6 of a half-integer: re-seed this case"
    assert worst <= 1e-9, what
    assert np.array_equal(pssm, want["pssm"]), what
    assert abs(info["lambda"] - want["info"]["lambda"]) <= 1e-9 and abs(info["n_distinct"] - want["info"]["n_distinct"]) <= 1e-12, what
    for key in ("n_rows", "n_observed", "n_clamped", "n_purged"):
        assert info[key] == want["info"][key], (what, key)


def test_abi_and_binding(swg):
    text = open(os.path.join(ROOT, "include", "swg.h")).read() + open(os.path.join(ROOT, "include", "swg_host.h")).read()
    assert "swg_pssm_from_paths_ex" in swg.ABI_SYMBOLS and hasattr(swg.lib, "swg_pssm_from_paths_ex")
    assert " swg_pssm_from_paths_ex(" in text and "n_purged" in text
    assert C.sizeof(swg.PssmInfo) == 32 and swg.PssmInfo.n_purged.offset == 28 and swg.PssmInfo.n_purged.size == 4
    assert swg.lib.swg_abi_version() == 3          # a function was added; the struct's reserved word took a name


# ---- the twin against the restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", OLD_CASES + NEW_CASES)
def test_blocks_against_numpy(swg, name):
    _assert_same(_twin(name, True, 0), _restated(name, True, 0), name)


@pytest.mark.parametrize("name", NEW_CASES + ("duplicate", "partial"))
@pytest.mark.parametrize("blocks", [False, True])
def test_purge_against_numpy(swg, name, blocks):
    _assert_same(_twin(name, blocks, 94), _restated(name, blocks, 94), "%s blocks %d purge 94" % (name, blocks))


@pytest.mark.parametrize("name", NEW_CASES)
def test_the_new_cases_under_the_whole_query_model(swg, name):
    c = _cases()[name]
    want = pc.model_numpy(c["sub"], c["q"], c["flat"], c["off"], c["al"])
    want["info"]["n_purged"] = 0
    _assert_same(_twin(name, False, 0), want, name)


@pytest.mark.parametrize("name", COINCIDE)
def test_the_models_coincide_where_every_row_spans_the_query(swg, name):
    (p1, v1, i1), (p0, v0, i0) = _twin(name, True, 0), _twin(name, False, 0)
    assert np.array_equal(p1, p0)
    assert float(np.abs(v1 - v0).max()) <= 1e-12
    assert abs(i1["n_distinct"] - i0["n_distinct"]) <= 1e-12 and {k: v for k, v in i1.items() if k != "n_distinct"} == \
        {k: v for k, v in i0.items() if k != "n_distinct"}


def test_partial_differs_under_blocks(swg):
    """Six hits on the middle third of 90 columns: their block is that third, not the query, so the rows' weights, Nbar
    and with them the scores change."""
    (p1, v1, _), (p0, v0, _) = _twin("partial", True, 0), _twin("partial", False, 0)
    differing = int((p1 != p0).sum())
    print("partial: entries that differ", differing, "largest move", float(np.abs(v1 - v0).max()))
    assert differing >= 1


def test_the_old_symbol_is_ex_with_both_options_off(swg):
    for name in ("partial", "gaps", "clamp", "staggered"):
        c = _cases()[name]
        q = np.ascontiguousarray(c["q"], dtype=np.int8)
        flat = np.ascontiguousarray(c["flat"], dtype=np.int8)
        off = np.ascontiguousarray(c["off"], dtype=np.uint64)
        sub = np.ascontiguousarray(c["sub"], dtype=np.int8)
        n = len(c["al"])
        stride = max(a["n_ops"] for a in c["al"]) + 1
        al = (swg.Alignment * n)()
        ops = C.create_string_buffer(n * stride)
        for i, a in enumerate(c["al"]):
            for field, _ in swg.Alignment._fields_:
                if field != "reserved":
                    setattr(al[i], field, int(a[field]))
            ops[i * stride:i * stride + len(a["ops"])] = a["ops"].encode()
        vp = lambda x: x.ctypes.data_as(C.c_void_p)
        freq = None if c["freq"] is None else np.ascontiguousarray(c["freq"], dtype=np.float64)
        head = (vp(sub), None if freq is None else vp(freq), float(c["beta"]), vp(q), q.size, vp(flat), vp(off), C.cast(al, C.c_void_p),
                C.cast(ops, C.c_void_p), stride, n)
        outs = []
        for ex in (False, True):
            pssm, values, info = np.full((q.size, 32), 99, dtype=np.int8), np.full((q.size, 32), 9.0), swg.PssmInfo()
            tail = (vp(pssm), vp(values), C.byref(info))
            rc = swg.lib.swg_pssm_from_paths_ex(*head, 0, 0, *tail) if ex else swg.lib.swg_pssm_from_paths(*head, *tail)
            assert rc == swg.SWG_OK
            outs.append((pssm.tobytes(), values.tobytes(), bytes(info)))
        assert outs[0] == outs[1], name


# ---- what the generators promise ---------------------------------------------------------------------------------------
def test_the_generators_made_what_they_promise(swg):
    cs = _cases()
    st = _restated("staggered", True, 0)
    assert bc.segments_of(st["ext"]) == 2 * len(cs["staggered"]["al"]) + 1 > len(st["ext"])        # segments outnumber the rows
    td = _restated("two_domains", True, 0)["ext"]
    assert (td[1] == (5, 40)).all() and (td[2:] == (55, 95)).all() and len(td) == 22
    covered = np.zeros(100, dtype=bool)
    for b, e in td[1:]:
        covered[b:e] = True
    assert (~covered).sum() == 5 + 15 + 5                             # columns only row 0 covers
    gr = cs["gap_row"]["al"][0]
    assert "DD" in gr["ops"] and gr["q_begin"] <= 40 < 42 <= gr["q_end"]
    X = pc.rows_of(cs["gap_row"]["q"], cs["gap_row"]["flat"], cs["gap_row"]["off"], cs["gap_row"]["al"])
    assert (X[1, 40:42] == pc.GAP).all()                              # its extent contains the columns, it shows a gap


# ---- the purge ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _purge_family():
    import swg_loader
    q, flat, off = bc.purge_family()
    al = pc.align(swg_loader.oracle(), q, flat, off, range(5), pc.table(B62), GAPS)
    assert all(a["ops"] == "M" * 100 and a["q_begin"] == 0 for a in al)   # ungapped and spanning: c = 100 for every pair
    return q, flat, off, al


def _purged(swg, hits, T, blocks=False):
    q, flat, off, al = _purge_family()
    chosen = [al[h] for h in hits]
    got = swg.pssm_from_paths(pc.table(B62), q, flat, off, chosen, want_values=True, blocks=blocks, purge=T)
    want = bc.model_numpy(pc.table(B62), q, flat, off, chosen, blocks=blocks, purge=T)
    _assert_same(got, want, "purge family %r at %d" % (hits, T))
    return got[2]["n_purged"], want["purged"]


def test_duplicate_loses_exactly_its_two_repeats(swg):
    info = _twin("duplicate", False, 94)[2]
    assert info["n_purged"] == 2 and info["n_rows"] == 4
    assert _restated("duplicate", False, 94)["purged"] == [4, 5]      # the second and third listing of hit 1 (rows 4 and 5)
    c = _cases()["duplicate"]
    once = swg.pssm_from_paths(c["sub"], c["q"], c["flat"], c["off"], c["al"][:3], want_values=True)
    assert np.array_equal(once[1], _twin("duplicate", False, 94)[1])  # ... and the rest is the build without them


def test_a_copy_of_the_query_is_dropped_at_any_T(swg):
    for T in (50, 94, 100):
        assert _purged(swg, [3], T) == (1, [1])
        assert _purged(swg, [0, 3], T, blocks=True) == (1, [2])       # (A, 80 % identical to the query, stays at every T)


def test_exactly_T_percent_is_dropped_and_one_column_less_is_kept(swg):
    A, B94, B93 = 0, 1, 2
    assert _purged(swg, [A, B94], 94) == (1, [2])                     # 100 * 94 >= 94 * 100
    assert _purged(swg, [A, B93], 94) == (0, [])                      # 100 * 93 <  94 * 100
    assert _purged(swg, [A, B93], 93) == (1, [2])
    assert _purged(swg, [A, B94], 95) == (0, [])


def test_a_purged_row_purges_no_later_one(swg):
    A, B94, C = 0, 1, 4
    assert _purged(swg, [A, B94, C], 94) == (1, [2])                  # C is 95 % to B94, which is gone, and 89 % to A
    assert _purged(swg, [B94, C], 94) == (1, [2])                     # (with B94 kept, C goes)


def test_purge_values_outside_the_range_are_refused(swg):
    c = _cases()["partial"]
    for T in (49, 101, 1, -94):
        with pytest.raises(swg.SwgError) as e:
            swg.pssm_from_paths(c["sub"], c["q"], c["flat"], c["off"], c["al"], purge=T)
        assert e.value.code == swg.SWG_ERR_ARG and "purge" in str(e.value) and "swg_pssm_from_paths_ex" in str(e.value)
    with pytest.raises(swg.SwgError) as e:
        swg.pssm_from_paths(c["sub"], c["q"], c["flat"], c["off"], c["al"], blocks=2)
    assert e.value.code == swg.SWG_ERR_ARG and "blocks" in str(e.value)
    for T in (50, 100):
        swg.pssm_from_paths(c["sub"], c["q"], c["flat"], c["off"], c["al"], purge=T)
