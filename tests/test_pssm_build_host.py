"""CPU: the host half of the PSSM construction -- swg_matrix_lambda, swg_pssm_from_paths (the twin of the device's
kernels) against the numpy restatement of pssm_build_cases with the oracle's paths, swg_pssm_save, and the end-to-end
fixture of the GPU tests pinned with the oracle alone."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import pssm_build_cases as pc
from conftest import ROOT
from test_pssm_host import sw_numpy

NEW_SYMBOLS = ("swg_matrix_lambda", "swg_pssm_from_paths", "swg_pssm_save", "swg_pssm_build", "swg_pssm_build_multi",
               "swg_pssm_build_multi_pssm")
CASES = ("nohits_BLOSUM62", "nohits_BLOSUM45", "nohits_PAM250", "lq1", "partial", "gaps", "odd_residues", "query_x", "duplicate",
         "score0", "clamp", "family_1", "family_24", "family_300", "pam250")


@functools.lru_cache(maxsize=None)
def _cases():
    import swg_loader
    return pc.host_cases(swg_loader.oracle())


@functools.lru_cache(maxsize=None)
def _both(name):
    """(the twin's answer, the restatement's) for one case, computed once."""
    import swg_loader
    swg = swg_loader.load()
    c = _cases()[name]
    got = swg.pssm_from_paths(c["sub"], c["q"], c["flat"], c["off"], c["al"], freq=c["freq"], pseudocount=c["beta"], want_values=True)
    want = pc.model_numpy(c["sub"], c["q"], c["flat"], c["off"], c["al"], freq=c["freq"], beta=c["beta"])
    return got, want


def test_abi_and_binding(swg):
    text = open(os.path.join(ROOT, "include", "swg.h")).read() + open(os.path.join(ROOT, "include", "swg_host.h")).read()
    for name in NEW_SYMBOLS:
        assert name in swg.ABI_SYMBOLS and hasattr(swg.lib, name), name
        assert " %s(" % name in text, name
    assert swg.lib.swg_abi_version() == 3          # functions and a struct were added, no struct changed
    assert C.sizeof(swg.PssmInfo) == 32
    assert "SWG_PSSM_PSEUDOCOUNT_DEFAULT 10.0" in text and swg.PSSM_PSEUDOCOUNT_DEFAULT == 10.0
    for method in ("build_pssm", "build_pssm_multi", "build_pssm_multi_pssm"):
        assert callable(getattr(swg.Context, method, None)), method
    for fn in ("matrix_lambda", "pssm_from_paths", "write_pssm"):
        assert callable(getattr(swg, fn, None)), fn


# ---- lambda -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(pc.MATRICES))
def test_lambda_residual(swg, name):
    sub = pc.table(name).astype(np.float64)
    lam = swg.matrix_lambda(pc.table(name))
    P = pc.builtin_freq() / pc.builtin_freq().sum()
    residual = abs(float((np.outer(P, P) * np.exp(lam * sub))[np.ix_(P > 0, P > 0)].sum()) - 1.0)
    print(name, lam, residual)
    assert lam > 0 and residual <= 1e-12
    assert abs(lam - pc.lambda_numpy(sub)) <= 1e-9


def test_lambda_of_blosum62(swg):
    assert round(swg.matrix_lambda(pc.table("BLOSUM62")), 10) == 0.3172837580
    assert round(swg.matrix_lambda(pc.table("BLOSUM62"), pc.builtin_freq() * 7.0), 10) == 0.3172837580    # (the library normalises)


def test_lambda_refusals(swg):
    positive = np.ones((32, 32), dtype=np.int8)                       # expected score >= 0
    negative = -np.ones((32, 32), dtype=np.int8)                      # no positive entry
    zero_mean = np.zeros((32, 32), dtype=np.int8)
    for sub in (positive, negative, zero_mean):
        with pytest.raises(swg.SwgError) as e:
            swg.matrix_lambda(sub)
        assert e.value.code == swg.SWG_ERR_ARG and "swg_matrix_lambda" in str(e.value) and "lambda" in str(e.value)
    for bad in (np.full(32, np.nan), -pc.builtin_freq(), np.zeros(32), np.r_[1.0, pc.builtin_freq()[1:]]):
        with pytest.raises(swg.SwgError) as e:
            swg.matrix_lambda(pc.table("BLOSUM62"), bad)
        assert e.value.code == swg.SWG_ERR_ARG and "freq" in str(e.value)
    lam = C.c_double()
    assert swg.lib.swg_matrix_lambda(None, None, C.byref(lam)) == swg.SWG_ERR_ARG


# ---- the twin against the restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_twin_against_numpy(swg, name):
    (pssm, values, info), want = _both(name)
    margin = pc.half_integer_margin(want["values"], want["have"])
    worst = float(np.abs(values - want["values"]).max())
    print(name, "rows", info["n_rows"], "Nbar", info["n_distinct"], "worst", worst, "margin", margin, info)
    assert margin >= 1e-6, "a value within 1e-6 of a half-integer: re-seed this case"
    assert worst <= 1e-9
    assert np.array_equal(pssm, want["pssm"])
    assert abs(info["lambda"] - want["info"]["lambda"]) <= 1e-9 and abs(info["n_distinct"] - want["info"]["n_distinct"]) <= 1e-12
    for key in ("n_rows", "n_observed", "n_clamped"):
        assert info[key] == want["info"][key], key
    assert np.array_equal(pssm[:, 0], np.zeros(len(pssm), dtype=np.int8))


def test_every_case_is_listed(orc):
    assert sorted(_cases()) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(pc.MATRICES))
def test_no_hits_gives_the_matrix_rows(swg, name):
    c = _cases()["nohits_" + name]
    (pssm, values, info), _ = _both("nohits_" + name)
    rows = c["sub"][c["q"].astype(np.int64)].copy()
    rows[:, 0] = 0
    assert np.array_equal(pssm, rows)
    A = pc.builtin_freq() > 0
    assert np.abs(values[:, A] - rows[:, A]).max() <= 2e-14
    assert info["n_rows"] == 1 and info["n_observed"] == 0 and info["n_distinct"] == 1.0 and info["n_clamped"] == 0


def test_the_generators_made_what_they_promise(swg):
    cs = _cases()
    ops = "/".join(a["ops"] for a in cs["gaps"]["al"])
    assert "III" in ops and "DD" in ops                               # runs of both gap kinds
    part = cs["partial"]["al"]
    assert all(a["q_begin"] > 0 and a["q_end"] < 90 for a in part)    # hits covering part of the query
    odd = set(int(v) for v in cs["odd_residues"]["flat"]) & {pc.idx(c) for c in "XBZ*"}
    assert len(odd) == 4
    assert (_both("query_x")[1]["m"] == 0).sum() >= 2                 # the m_p = 0 fallback is taken
    assert [a["index"] for a in cs["duplicate"]["al"]].count(1) == 3
    assert cs["score0"]["al"][1]["score"] == 0 and cs["score0"]["al"][1]["ops"] == ""
    assert _both("score0")[0][2]["n_rows"] == 3
    assert _both("clamp")[0][2]["n_clamped"] > 0
    assert cs["lq1"]["q"].size == 1 and _both("lq1")[0][2]["n_rows"] == 5       # (Y against W scores 2)


def test_a_duplicate_counts_twice(swg):
    c = _cases()["duplicate"]
    once = swg.pssm_from_paths(c["sub"], c["q"], c["flat"], c["off"], c["al"][:3])[0]
    assert not np.array_equal(once, _both("duplicate")[0][0])


def test_a_score0_hit_contributes_nothing(swg):
    c = _cases()["score0"]
    without = swg.pssm_from_paths(c["sub"], c["q"], c["flat"], c["off"], [c["al"][0], c["al"][2]], want_values=True)
    assert np.array_equal(without[1], _both("score0")[0][1])


# ---- properties -------------------------------------------------------------------------------------------------------
def test_a_conserved_motif_gains_score(swg, orc):
    sub, gaps = pc.table("BLOSUM62"), pc.MATRICES["BLOSUM62"]
    motif = tuple(range(40, 52))
    q, flat, off, hits = pc.family(31, 100, 40, subst=(0.3, 0.7), keep=motif)
    pssm = swg.pssm_from_paths(sub, q, flat, off, pc.align(orc, q, flat, off, hits, sub, gaps))[0]
    for p in motif:
        assert pssm[p, q[p]] > sub[q[p], q[p]], p


def test_a_column_where_every_hit_differs_scores_the_hits_residue_higher(swg, orc):
    sub, gaps = pc.table("BLOSUM62"), pc.MATRICES["BLOSUM62"]
    rng = np.random.default_rng(32)
    q = pc.random_seq(rng, 80)
    q[30] = pc.idx("A")
    seqs = [pc.relative(rng, q, 0.2, odd={30: pc.idx("W")}) for _ in range(20)]
    flat, off = pc.pack(seqs)
    pssm = swg.pssm_from_paths(sub, q, flat, off, pc.align(orc, q, flat, off, range(20), sub, gaps))[0]
    assert pssm[30, pc.idx("W")] > pssm[30, pc.idx("A")]


# ---- refusals and the file ----------------------------------------------------------------------------------------------
def test_twin_refusals(swg):
    c = _cases()["gaps"]
    args = (c["sub"], c["q"], c["flat"], c["off"], c["al"])
    for kw in ({"pseudocount": 0.0}, {"pseudocount": -1.0}, {"pseudocount": float("inf")}, {"pseudocount": float("nan")},
               {"freq": np.full(32, -1.0)}):
        with pytest.raises(swg.SwgError) as e:
            swg.pssm_from_paths(*args, **kw)
        assert e.value.code == swg.SWG_ERR_ARG and "swg_pssm_from_paths" in str(e.value)
    with pytest.raises(swg.SwgError) as e:
        swg.pssm_from_paths(np.ones((32, 32), dtype=np.int8), *args[1:])
    assert e.value.code == swg.SWG_ERR_ARG and "lambda" in str(e.value)
    broken = [dict(c["al"][0])]
    broken[0]["ops"] = "M" * (len(c["q"]) + 400)                       # a path that leaves its pair
    broken[0]["n_ops"] = len(broken[0]["ops"])
    with pytest.raises(swg.SwgError) as e:
        swg.pssm_from_paths(c["sub"], c["q"], c["flat"], c["off"], broken)
    assert e.value.code == swg.SWG_ERR_ARG and "path" in str(e.value)


def test_save_and_load_return_the_same_bytes(swg, tmp_path):
    sc = swg.load_scoring("BLOSUM62")
    for name in ("gaps", "odd_residues", "query_x"):
        c = _cases()[name]
        pssm = _both(name)[0][0]
        path = tmp_path / (name + ".pssm")
        swg.write_pssm(str(path), pssm, c["q"])
        back, q = swg.read_pssm(str(path), sc)
        assert np.array_equal(back, pssm) and np.array_equal(q, c["q"])
    with pytest.raises(swg.SwgError) as e:
        swg.write_pssm(str(tmp_path / "no" / "such" / "dir.pssm"), pssm, c["q"])
    assert e.value.code == swg.SWG_ERR_IO


# ---- the end-to-end fixture ----------------------------------------------------------------------------------------------
E2E_PINNED = {"first": 26, "second": 29}          # family members among the top 30 of iteration 1 and of iteration 2


@functools.lru_cache(maxsize=None)
def e2e_cpu():
    """Iteration 1 by the oracle, the twin's PSSM of the hits at or above the inclusion score, iteration 2 by the numpy
    PSSM scorer -> dict(q, flat, off, is_family, scores1, included, pssm, scores2, first, second)."""
    import swg_loader
    swg, orc = swg_loader.load(), swg_loader.oracle()
    sub, gaps = pc.table("BLOSUM62"), pc.MATRICES["BLOSUM62"]
    q, flat, off, is_family = pc.e2e_database()
    scores1 = orc.score_db(q, flat, off, sub, *gaps)
    included = [i for i in np.lexsort((np.arange(len(scores1)), -scores1.astype(np.int64))) if scores1[i] >= pc.E2E["include_score"]]
    pssm = swg.pssm_from_paths(sub, q, flat, off, pc.align(orc, q, flat, off, included, sub, gaps))[0]
    scores2 = sw_numpy(pssm, flat, off, *gaps)
    return dict(q=q, flat=flat, off=off, is_family=is_family, scores1=scores1, included=[int(i) for i in included], pssm=pssm,
                scores2=scores2, first=pc.family_in_top(scores1, is_family, pc.E2E["top"]),
                second=pc.family_in_top(scores2, is_family, pc.E2E["top"]))


def test_the_second_iteration_finds_more_of_the_family(swg, orc):
    e = e2e_cpu()
    print("family members in the top %d: iteration 1 %d, iteration 2 %d; included %d" % (pc.E2E["top"], e["first"], e["second"], len(e["included"])))
    assert not (set(e["included"]) - set(np.flatnonzero(e["is_family"]).tolist())), "a random sequence was included"
    assert e["second"] > e["first"]
    assert (e["first"], e["second"]) == (E2E_PINNED["first"], E2E_PINNED["second"])
