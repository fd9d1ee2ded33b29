"""CPU: several non-overlapping alignments per hit, host side (swg_align_hsps_host, the twin of swg_align_hsps*).

The twin against the scalar model of hsps_model.py on every small case of hsps_cases.py -- scores, coordinates, paths,
counts and the number of alignments, all exactly --, alignment 0 against the int32 oracle's traceback, every path
re-scored by the oracle, and the invariants of the rule: scores never increase, no two alignments of a pair share an
aligned residue pair.  The width-edge cases are too slow for the model: there the invariants and alignment 0 are
checked, and from then on the twin is their judge (test_gpu_hsps.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import hsps_cases as hc
import hsps_model as hm
from conftest import ROOT

NEW = ("swg_align_hsps", "swg_align_hsps_multi", "swg_align_hsps_multi_pssm", "swg_align_hsps_host")
FIELDS = ("score", "q_begin", "q_end", "d_begin", "d_end", "n_ops", "ops", "n_ident", "n_match", "n_gap_open", "n_gap")


@pytest.fixture(scope="module")
def tables(swg):
    return swg.load_scoring("BLOSUM62").table(), swg.load_scoring("PAM250").table()


def twin(swg, case, pssm=None, **kw):
    args = dict(max_hsps=case["max_hsps"], min_score=case["min_score"], want_counts=True)
    args.update(kw)
    if pssm is not None:
        return swg.align_hsps_host(None, case["gap_open"], case["gap_extend"], case["seq"], pssm=pssm, **args)
    return swg.align_hsps_host(case["sub"], case["gap_open"], case["gap_extend"], case["seq"], query=case["query"], **args)


def model(case, pssm=None):
    return hm.align(case["sub"], case["gap_open"], case["gap_extend"], case["seq"], case["max_hsps"], case["min_score"],
                    query=None if pssm is not None else case["query"], pssm=pssm)


def strip(als):
    return [{f: a[f] for f in FIELDS} for a in als]


def m_cells(a):
    """The (database position, query column) pairs of an alignment's M steps, from 0."""
    i, j, out = a["q_begin"], a["d_begin"], set()
    for op in a["ops"]:
        if op == "M":
            out.add((j, i))
            i, j = i + 1, j + 1
        elif op == "I":
            j += 1
        else:
            i += 1
    assert (i, j) == (a["q_end"], a["d_end"])
    return out


def check_invariants(orc, case, als):
    """What holds for any pair: the oracle's alignment 0, additive path scores, scores that never increase, disjoint M
    cells, a cut respected and a cap respected."""
    q, d, sub, go, ge = case["query"], case["seq"], case["sub"], case["gap_open"], case["gap_extend"]
    assert len(als) <= case["max_hsps"]
    sc, coords, ops = orc.pair_trace(q, d, sub, go, ge)
    if sc >= case["min_score"]:
        a = als[0]
        assert (a["score"], (a["q_begin"], a["q_end"], a["d_begin"], a["d_end"]), a["ops"]) == (sc, coords, ops), case["name"]
    else:
        assert als == []
    seen = set()
    for r, a in enumerate(als):
        assert a["score"] >= case["min_score"] and a["index"] == 0
        assert orc.path_score(q, d, sub, go, ge, (a["q_begin"], a["q_end"], a["d_begin"], a["d_end"]), a["ops"]) == a["score"]
        assert r == 0 or a["score"] <= als[r - 1]["score"], case["name"]
        cells = m_cells(a)
        assert a["ops"][-1] == "M" and len(cells) == a["n_match"]      # (a gap that pays may open a path; H ends it)
        assert not (cells & seen), case["name"]
        seen |= cells


def test_abi_exports_and_header(swg):
    text = open(os.path.join(ROOT, "include", "swg.h")).read()
    for name in NEW:
        assert name in swg.ABI_SYMBOLS and hasattr(swg.lib, name), name
        assert " %s(" % name in text, name
    assert "#define SWG_MAX_HSPS 64" in text
    assert swg.lib.swg_abi_version() == 3            # functions were added, no struct changed
    for method in ("align_hsps", "align_hsps_multi", "align_hsps_multi_pssm"):
        assert callable(getattr(swg.Context, method, None)), method
    assert callable(swg.align_hsps_host)


def test_twin_equals_model_on_small_cases(swg, orc, tables):
    """... and the conditions on the case set itself: later paths do cross used cells in a gap state, and all three stop
    reasons occur (otherwise the random cases would not reach what they are for)."""
    crossings, stops = 0, set()
    for case in hc.small_cases(*tables):
        got = twin(swg, case)
        want, info = model(case)
        assert strip(got) == strip(want), case["name"]
        for a, w in zip(got, want):
            assert m_cells(a) == {(j - 1, i - 1) for j, i in w["cells"]}
        check_invariants(orc, case, got)
        if case["name"].startswith("random"):
            crossings += info["crossings"]
            stops.add(info["stop"])
    print("gap-state steps of later paths on used cells: %d; stop reasons: %s" % (crossings, sorted(stops)))
    assert crossings > 0
    assert stops == {"cap", "score", "exhausted"}


def test_repeat_case_is_the_table_worked_by_hand(swg):
    full, cap2, min43 = hc.repeat_cases()
    got = twin(swg, full)
    assert [(a["score"], a["q_begin"], a["q_end"], a["d_begin"], a["d_end"], a["n_ops"]) for a in got] == hc.REPEAT_EXPECTED
    assert all(a["ops"] == "M" * a["n_ops"] and a["n_ident"] == a["n_ops"] and a["n_gap"] == 0 for a in got)
    assert strip(twin(swg, cap2)) == strip(got[:2])          # stopped by the cap
    assert strip(twin(swg, min43)) == strip(got[:1])         # stopped by the score


def test_tiny_cases(swg):
    one, zero = hc.tiny_cases()
    got = twin(swg, one)
    assert len(got) == 1 and (got[0]["score"], got[0]["ops"], got[0]["q_end"], got[0]["d_end"]) == (3, "M", 1, 1)
    assert twin(swg, zero) == []


def test_domain_cases_have_the_outcomes_they_were_made_for(swg, tables):
    swapped, bridged, split = hc.domain_cases(tables[0])
    a = twin(swg, swapped)
    assert len(a) == 2 and (a[0]["q_end"] <= a[1]["q_begin"] or a[1]["q_end"] <= a[0]["q_begin"])
    assert a[0]["d_end"] <= a[1]["d_begin"] or a[1]["d_end"] <= a[0]["d_begin"]
    b = twin(swg, bridged)
    assert len(b) == 1 and "I" * 60 in b[0]["ops"]
    s = twin(swg, split)
    assert len(s) == 2 and all(x["n_gap"] == 0 or "I" * 30 not in x["ops"] for x in s)


def test_pssm_of_the_matrix_rows_gives_the_index_alignments(swg, tables):
    """Every field and path; identity alone is counted against another sequence (the PSSM's consensus, which a matrix
    row's best residue need not be the query's own), and there the model is the judge."""
    def but_ident(als):
        return [{k: v for k, v in a.items() if k != "n_ident"} for a in als]

    for case in hc.all_cases(*tables):
        p = hc.pssm_of(case)
        got = twin(swg, case, pssm=p)
        assert but_ident(got) == but_ident(twin(swg, case)), case["name"]
        if case["small"] and not case["name"].startswith("random"):
            assert strip(got) == strip(model(case, pssm=p)[0]), case["name"]


def test_free_pssm_equals_model(swg):
    f = hc.free_pssm_case()
    case = dict(f, sub=None, query=None)
    got = twin(swg, case, pssm=f["pssm"])
    want, _ = model(case, pssm=f["pssm"])
    assert len(got) >= 2 and strip(got) == strip(want)


def test_width_edges_invariants_and_at_least_three_rounds(swg, orc, tables):
    for case in hc.width_cases(tables[0]):
        got = twin(swg, case)
        assert len(got) >= 3, case["name"]
        check_invariants(orc, case, got)


def test_outputs_not_wanted_change_nothing_else(swg, tables):
    case = hc.matrix_cases(*tables)[0]
    full = twin(swg, case)
    bare = twin(swg, case, want_ops=False, want_counts=False)
    assert bare == [{k: v for k, v in a.items() if k in ("score", "index", "q_begin", "q_end", "d_begin", "d_end", "n_ops")} for a in full]


def test_argument_errors(swg):
    t = hc.simple_table()
    q = np.array([1, 2, 3], dtype=np.int8)
    ok = dict(max_hsps=2, min_score=1)
    for kw in (dict(ok, max_hsps=0), dict(ok, max_hsps=65), dict(ok, min_score=0), dict(ok, min_score=-3)):
        with pytest.raises(swg.SwgError) as e:
            swg.align_hsps_host(t, -4, -1, q, query=q, **kw)
        assert e.value.code == swg.SWG_ERR_ARG and "swg_align_hsps_host" in str(e.value)
    with pytest.raises(swg.SwgError) as e:                    # neither a query nor a PSSM
        swg.align_hsps_host(t, -4, -1, q, **ok)
    assert e.value.code == swg.SWG_ERR_ARG
    with pytest.raises(swg.SwgError) as e:                    # both
        swg.align_hsps_host(t, -4, -1, q, query=q, pssm=np.zeros((3, 32), dtype=np.int8), **ok)
    assert e.value.code == swg.SWG_ERR_ARG
    with pytest.raises(swg.SwgError) as e:
        swg.align_hsps_host(t, -4, -1, q, query=np.array([0, 1], dtype=np.int8), **ok)
    assert e.value.code == swg.SWG_ERR_RESIDUE
    out = (swg.Alignment * 2)()
    n = C.c_uint32(7)
    vp = C.c_void_p
    rc = swg.lib.swg_align_hsps_host(t.ctypes.data_as(vp), -4, -1, q.ctypes.data_as(vp), None, 3, q.ctypes.data_as(vp), 3, 2, 1,
                                     C.cast(out, vp), None, None, 0, None)
    assert rc == swg.SWG_ERR_ARG and n.value == 7


def test_device_calls_refuse_a_null_context(swg):
    q = np.ones(4, dtype=np.int8)
    off = np.array([0, 4], dtype=np.uint64)
    hits, nh, out, n = (swg.Hit * 1)(), (C.c_size_t * 1)(1), (swg.Alignment * 1)(), (C.c_uint32 * 1)()
    vp = C.c_void_p
    assert swg.lib.swg_align_hsps(None, None, C.cast(hits, vp), 1, 1, 1, C.cast(out, vp), C.cast(n, vp), None, None, 0) == swg.SWG_ERR_ARG
    assert b"swg_align_hsps: NULL context" in swg.lib.swg_global_error()
    for name in ("swg_align_hsps_multi", "swg_align_hsps_multi_pssm"):
        src = q if name.endswith("multi") else np.zeros((4, 32), dtype=np.int8)
        rc = getattr(swg.lib, name)(None, None, src.ctypes.data_as(vp), off.ctypes.data_as(vp), 1, C.cast(hits, vp), 1, C.cast(nh, vp),
                                    1, 1, C.cast(out, vp), C.cast(n, vp), None, None, 0)
        assert rc == swg.SWG_ERR_ARG and name.encode() + b": NULL context" in swg.lib.swg_global_error()
