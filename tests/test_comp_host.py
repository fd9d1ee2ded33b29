"""CPU: composition-based score adjustment, host side (swg_comp_adjust_host, the twin of swg_comp_adjust*).

The twin against the numpy model of comp_model.py on every case of comp_cases.py -- ratio16, status, scaled_score and
adj_score exactly, the two lambdas within 1e-9 relative (the bound tests/test_evalue_host.py holds the Gumbel twin to) --,
after the margin that makes exact equality of ratio16 a legitimate demand: the model's r x 65536 is at least 1e-6 away
from every half-integer in every case.  Then the invariants of the rule against the int32 oracle, lambda_std against
swg_matrix_lambda, the cases' own properties (what each expects, the pinned lane-local columns), the argument errors
and the exports (the option's range needs a context: test_gpu_comp.py)."""
import ctypes as C

import numpy as np
import pytest

import comp_cases as cc
import comp_model as cm
import pssm_build_cases as pc
import swg_loader

NEW = ("swg_comp_adjust", "swg_comp_adjust_multi", "swg_comp_adjust_multi_pssm", "swg_comp_adjust_host")
REL = 1e-9


def twin(swg, c, i, F=None):
    return swg.comp_adjust_host(c["sub"], c["gap_open"], c["gap_extend"], c["seqs"][i], query=c["query"], pssm=c["pssm"], freq=c["freq"],
                                scale=c["F"] if F is None else F)


@pytest.fixture(scope="module")
def models():
    """The model's answer for every (case, distinct hit), computed once."""
    out = {}
    for c in cc.all_cases():
        for i in sorted(set(c["hits"])):
            out[c["name"], i] = cm.adjust(c["sub"], c["gap_open"], c["gap_extend"], c["seqs"][i], query=c["query"], pssm=c["pssm"],
                                          freq=c["freq"], F=c["F"])
    return out


def close(a, b):
    return abs(a - b) <= REL * abs(b)


def test_the_case_list_holds_what_it_must():
    cases = cc.all_cases()
    names = {c["name"] for c in cases}
    assert {c["F"] for c in cases} == set(cc.SCALES)
    assert {(c["gap_open"], c["gap_extend"]) for c in cases} >= {(0, 1), (2, 3), (0, 0), (-11, -1)}
    assert any(len(c["hits"]) != len(set(c["hits"])) for c in cases)                        # a duplicate hit
    assert any(c["freq"] is not None and (np.asarray(c["freq"])[1:] == 0).any() and c["query"] is not None for c in cases)
    assert {"x_only_subject", "pssm_positive_against_subject", "pssm_no_positive_entry", "pssm_full_int8"} <= names
    full = next(c for c in cases if c["name"] == "pssm_full_int8")["pssm"]
    assert full.min() == -128 and full.max() == 127
    for c in cases:
        assert all(1 <= len(s) <= 400 for s in c["seqs"]) and len(c["hits"]) <= 64, c["name"]
        assert cc.lq_of(c) <= 400 or "G" in c or "over" in c, c["name"]
    # every class at its three edge lengths and at one column, subjects of 1, 2 and G + 3 residues
    held = {(c["G"], c["K"], cc.lq_of(c)) for c in cases if "G" in c}
    assert held == {(G, K, lq) for G, K in cc.CLASSES for lq in cc.class_lengths(G, K)} | {(16, 4, 1)}
    for c in cases:
        if "G" in c:
            assert [len(s) for s in c["seqs"][:3]] == [1, 2, c["G"] + 3] and cc.class_of(cc.lq_of(c)) == cc.CLASSES.index((c["G"], c["K"]))
    assert {(cc.lq_of(c), c["over"], c["pssm"] is None) for c in cases if "over" in c} == \
        {(cc.COLS, False, True), (cc.COLS, False, False), (cc.COLS + 1, True, True), (cc.COLS + 1, True, False)}
    assert all(len(c["seqs"][0]) == 64 for c in cases if "over" in c)


def test_the_models_ratio_is_clear_of_every_rounding_edge(models):
    """r x 65536 at least 1e-6 from every half-integer: the twin's and the device's lambdas, good to 1e-9 relative, then
    round to the model's ratio16."""
    n = 0
    for key, m in models.items():
        if m["status"] == 0:
            frac = m["r65536"] - np.floor(m["r65536"])
            assert abs(frac - 0.5) >= 1e-6, (key, m["r65536"])
            n += 1
    assert n > 300


def test_each_case_gives_what_it_expects(models):
    seen = set()
    for c in cc.all_cases():
        for i in set(c["hits"]):
            m = models[c["name"], i]
            if c["expect"] == "floor":
                assert (m["status"], m["ratio16"]) == (0, 32768), (c["name"], i, m["r65536"])
            elif c["expect"] == "cap":
                assert (m["status"], m["ratio16"]) == (0, 65536), (c["name"], i, m["r65536"])
            elif c["expect"] == "between":
                assert m["status"] == 0 and 32768 < m["ratio16"] < 65536, (c["name"], i, m["r65536"])
            elif c["expect"] == "none":
                assert (m["status"], m["ratio16"]) == (1, 65536), (c["name"], i)
        seen.add(c["expect"])
    assert seen == {"floor", "cap", "between", "none", None}
    # the three ways to status 1: nothing counted, no lambda_hit beside a lambda_std, no lambda_std
    assert models["pssm_positive_against_subject", 0]["lambda_std"] is not None
    assert models["pssm_no_positive_entry", 0]["lambda_std"] is None
    zero = next(c for c in cc.all_cases() if c["name"] == "freq_zero_weight")
    assert models["freq_zero_weight", len(zero["seqs"]) - 1]["status"] == 1             # all L, and L is not in A: n = 0


def test_every_lane_local_column_decides_a_score(models):
    """For every instantiation case and every lane-local column k some pair has all its best cells in columns = k mod K, so
    an instantiation that computed one of its K columns wrongly changes a score.  From the model's column-resolved bests."""
    n = 0
    for c in cc.all_cases():
        if "G" not in c:
            continue
        K, lq = c["K"], cc.lq_of(c)
        assert sorted(c["pinned"]) == list(range(min(K, lq))), c["name"]
        for k, i in c["pinned"].items():
            m = models[c["name"], i]
            at = np.nonzero(m["colbest"] == m["scaled_score"])[0]
            assert m["scaled_score"] > 0 and set((at % K).tolist()) == {k}, (c["name"], k, at)
            n += 1
        # (the last lane's single column at (G - 1) K + 1 is pinned by k = 0's subject)
        if lq == (c["G"] - 1) * K + 1 and lq > 1:
            m = models[c["name"], c["pinned"][0]]
            assert int(np.argmax(m["colbest"])) == lq - 1, c["name"]
    assert n == sum(min(c["K"], cc.lq_of(c)) for c in cc.all_cases() if "G" in c) > 200


def test_the_models_two_fills_agree():
    """The row-vectorised recurrence the larger cases use against the scalar int32 loop, on every small pair."""
    n = 0
    for c in cc.all_cases():
        if cc.lq_of(c) > 130:
            continue
        for i in sorted(set(c["hits"]))[:3]:
            if len(c["seqs"][i]) > 100:
                continue
            kw = dict(query=c["query"], pssm=c["pssm"], freq=c["freq"], F=c["F"])
            a = cm.adjust(c["sub"], c["gap_open"], c["gap_extend"], c["seqs"][i], **kw)
            b = cm.adjust(c["sub"], c["gap_open"], c["gap_extend"], c["seqs"][i], scalar=True, **kw)
            assert a["scaled_score"] == b["scaled_score"], (c["name"], i)
            n += 1
    assert n >= 40


def test_twin_equals_the_model_on_every_case(swg, models):
    for c in cc.all_cases():
        for i in sorted(set(c["hits"])):
            r, lam_std = twin(swg, c, i)
            m = models[c["name"], i]
            got = (int(r["ratio16"]), int(r["status"]), int(r["scaled_score"]), int(r["adj_score"]))
            assert got == (m["ratio16"], m["status"], m["scaled_score"], m["adj_score"]), (c["name"], i, got, m["r65536"])
            if m["lambda_std"] is None:
                assert lam_std == 0.0
            else:
                assert close(lam_std, m["lambda_std"]), (c["name"], lam_std, m["lambda_std"])
            if m["lambda_hit"] is None:
                assert r["lambda_hit"] == 0.0
            else:
                assert close(float(r["lambda_hit"]), m["lambda_hit"]), (c["name"], i)


def _index_form(c):
    """(q, sub) under which the oracle scores the case's query, or None (a PSSM of free columns)."""
    if c["query"] is not None:
        return c["query"], c["sub"]
    return c.get("index_form")


def test_no_adjustment_is_the_exact_score_at_every_scale(swg, orc, models):
    """ratio16 == 65536 gives T[s] = F s: scaled_score = F x the pair's exact score and adj_score = that score, whatever F."""
    n = 0
    for c in cc.all_cases():
        form = _index_form(c)
        if form is None or cc.lq_of(c) > 400:
            continue
        for i in sorted(set(c["hits"])):
            if models[c["name"], i]["ratio16"] != 65536:
                continue
            exact = orc.pair(form[0], c["seqs"][i], form[1], c["gap_open"], c["gap_extend"])
            for F in cc.SCALES:
                r, _ = twin(swg, c, i, F=F)
                assert (int(r["adj_score"]), int(r["scaled_score"])) == (exact, F * exact), (c["name"], i, F)
            n += 1
    assert n >= 30


def test_scale_one_is_the_oracle_under_the_rescaled_table(swg, orc):
    """F = 1 makes T an int8 table: the int32 oracle scores the pair under T o sub, built here from the twin's own ratio16."""
    n = adjusted = 0
    for c in cc.all_cases():
        form = _index_form(c)
        if form is None or cc.lq_of(c) > 400:
            continue
        for i in sorted(set(c["hits"])):
            r, _ = twin(swg, c, i, F=1)
            T = cm.table(1, int(r["ratio16"]))
            tsub = T[np.asarray(form[1], dtype=np.int64) + 128].astype(np.int8)
            want = orc.pair(form[0], c["seqs"][i], tsub, c["gap_open"], c["gap_extend"])
            assert int(r["scaled_score"]) == int(r["adj_score"]) == want, (c["name"], i)
            n += 1
            adjusted += int(r["ratio16"]) < 65536
    assert n >= 100 and adjusted >= 30


def test_lambda_std_is_the_matrix_lambda_for_a_query_in_proportion(swg):
    """A query that holds every residue of A in proportion to P has hP = sum_ab P_a P_b [sub_ab = s] x lq: the two
    distributions coincide, and so do the roots."""
    b62 = pc.table("BLOSUM62")
    for per in (200, 1000):
        counts = np.rint(pc.builtin_freq() / pc.builtin_freq().sum() * per).astype(np.int64)
        assert (counts[pc.builtin_freq() > 0] >= 1).all()
        q = np.repeat(np.arange(32), counts).astype(np.int8)
        fq = counts.astype(np.float64)              # the background IS the query's composition
        _, lam_std = swg.comp_adjust_host(b62, -11, -1, q[:5], query=q, freq=fq)
        want = swg.matrix_lambda(b62, fq)
        assert 0.2 < want < 0.4 and close(lam_std, want), (per, lam_std, want)


def test_the_argument_errors(swg):
    b62 = pc.table("BLOSUM62")
    q, d = cc.background_seq(np.random.default_rng(1), 30), cc.background_seq(np.random.default_rng(2), 40)
    ok = dict(query=q)
    swg.comp_adjust_host(b62, -11, -1, d, **ok)
    for kw in (dict(scale=0), dict(scale=65), dict(scale=-1)):
        with pytest.raises(swg.SwgError) as e:
            swg.comp_adjust_host(b62, -11, -1, d, query=q, **kw)
        assert e.value.code == swg.SWG_ERR_ARG
    for bad in (np.full(32, np.nan), -pc.builtin_freq(), np.zeros(32), np.r_[1.0, pc.builtin_freq()[1:]]):
        with pytest.raises(swg.SwgError) as e:
            swg.comp_adjust_host(b62, -11, -1, d, query=q, freq=bad)
        assert e.value.code == swg.SWG_ERR_ARG
    for kw in (dict(), dict(query=q, pssm=b62[q.astype(np.int64)]), dict(query=q[:0])):
        with pytest.raises(swg.SwgError) as e:
            swg.comp_adjust_host(b62, -11, -1, d, **kw)
        assert e.value.code == swg.SWG_ERR_ARG
    with pytest.raises(swg.SwgError) as e:
        swg.comp_adjust_host(b62, -11, -1, d, query=np.r_[q, 0].astype(np.int8))
    assert e.value.code == swg.SWG_ERR_RESIDUE
    with pytest.raises(swg.SwgError) as e:
        swg.comp_adjust_host(b62, -11, -1, np.r_[d, 32].astype(np.int8), query=q)
    assert e.value.code == swg.SWG_ERR_RESIDUE
    with pytest.raises(swg.SwgError) as e:                      # a pair whose int32 cells could wrap
        swg.comp_adjust_host(b62, 30000, 2000, np.tile(d, 30), query=q, scale=64)
    assert e.value.code == swg.SWG_ERR_ARG
    # an empty sequence counts nothing and scores nothing
    r, lam = swg.comp_adjust_host(b62, -11, -1, d[:0], query=q)
    assert (int(r["status"]), int(r["ratio16"]), int(r["scaled_score"]), int(r["adj_score"])) == (1, 65536, 0, 0) and lam > 0
    assert lib_null_out(swg) == swg.SWG_ERR_ARG


def lib_null_out(swg):
    q = np.ones(4, dtype=np.int8)
    t = np.ascontiguousarray(pc.table("BLOSUM62"))
    return swg.lib.swg_comp_adjust_host(t.ctypes.data_as(C.c_void_p), -11, -1, q.ctypes.data_as(C.c_void_p), None, 4, q.ctypes.data_as(C.c_void_p), 4,
                                        None, 32, None, None)


def test_the_symbols_are_exported_and_declared(swg):
    import os
    header = open(os.path.join(swg_loader.ROOT, "include", "swg.h")).read()
    for name in NEW:
        assert hasattr(swg.lib, name) and name in swg.ABI_SYMBOLS and ("int %s(" % name) in header, name
    assert "typedef struct swg_comp_result" in header and swg.COMP_DTYPE.itemsize == 24
    assert swg.COMP_CLASSES == cc.CLASSES and swg.COMP_COLS == cc.COLS == cc.CLASSES[-1][0] * cc.CLASSES[-1][1]
