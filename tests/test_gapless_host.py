"""CPU: the gapless search's host side (swg_search_gapless and its batch forms): the ABI and the binding, the truth the
GPU tests compare against -- the oracle with the gaps priced out equals a direct restatement of the recurrence --, and
the plan hook: which queries take the gapless cells (route 1) and which the gapped machinery (route 0)."""
import ctypes as C

import numpy as np
import pytest

import gapless_cases as gc
import scoring_edges as se
from conftest import ROOT  # noqa: F401  (path set-up)

NEW_SYMBOLS = ("swg_search_gapless", "swg_search_gapless_multi", "swg_search_gapless_multi_pssm")


def test_gapless_abi_and_binding(swg):
    for name in NEW_SYMBOLS:
        assert hasattr(swg.lib, name), name
        assert name in swg.ABI_SYMBOLS, name
    for name in ("search_gapless", "search_gapless_multi", "search_gapless_multi_pssm"):
        assert callable(getattr(swg.Context, name, None)), name
    assert callable(getattr(swg.Database, "debug_plan_gapless", None))
    assert swg.lib.swg_abi_version() == 3
    # a NULL context: SWG_ERR_ARG and a message, from each of the three
    nh = C.c_size_t(0)
    calls = {
        "swg_search_gapless": lambda: swg.lib.swg_search_gapless(None, None, None, None, 0, C.byref(nh), None),
        "swg_search_gapless_multi": lambda: swg.lib.swg_search_gapless_multi(None, None, None, None, 0, None, None, 0, None, None),
        "swg_search_gapless_multi_pssm": lambda: swg.lib.swg_search_gapless_multi_pssm(None, None, None, None, 0, None, None, 0, None, None),
    }
    for name, call in calls.items():
        assert call() == swg.SWG_ERR_ARG, name
        assert name in swg.lib.swg_global_error().decode(), name


def _tables(swg):
    b62 = swg.load_scoring("BLOSUM62").table()
    return {"blosum62": np.array(b62, dtype=np.int8).reshape(32, 32), "diag127": se.diag127(), "full_range": se.full_range(),
            "all_127": se.all_127(), "all_m128": se.all_m128()}


def test_priced_out_oracle_is_the_gapless_recurrence(swg, orc):
    """300 random pairs over int8-extreme tables, with planted copies (whole, partial, shifted): 0 mismatches."""
    rng = np.random.default_rng(2025)
    tables = _tables(swg)
    names = sorted(tables)
    n_pairs = n_positive = n_big = 0
    for t in range(30):
        sub = tables[names[t % len(names)]]
        lq = int(rng.integers(1, 120))
        q = rng.integers(1, 32, size=lq).astype(np.int8)
        seqs = []
        for s in range(10):
            kind = s % 5
            if kind == 0:                     # a random sequence
                d = rng.integers(1, 32, size=int(rng.integers(1, 150))).astype(np.int8)
            elif kind == 1:                   # a planted copy of a stretch of the query between junk
                a = int(rng.integers(0, lq))
                b = int(rng.integers(a + 1, lq + 1))
                d = np.concatenate([rng.integers(1, 32, size=int(rng.integers(0, 9))), q[a:b], rng.integers(1, 32, size=int(rng.integers(0, 9)))]).astype(np.int8)
            elif kind == 2:                   # the whole query
                d = q.copy()
            elif kind == 3:                   # a copy with an indel in the middle: the gapless score sees one side only
                cut = lq // 2
                d = np.concatenate([q[:cut], rng.integers(1, 32, size=2), q[cut:]]).astype(np.int8)
            else:                             # a copy with substitutions
                d = q.copy()
                hit = rng.random(lq) < 0.2
                d[hit] = rng.integers(1, 32, size=int(hit.sum()))
            seqs.append(d)
        flat, off = gc.pack(seqs)
        want = gc.gapless_numpy(q, flat, off, sub)
        got = gc.oracle_gapless(orc, q, flat, off, sub)
        assert np.array_equal(got, want), (names[t % len(names)], lq)
        n_pairs += len(seqs)
        n_positive += int((want > 0).sum())
        n_big += int((want >= 4096).sum())
    assert n_pairs == 300 and n_positive >= 150 and n_big >= 10, (n_pairs, n_positive, n_big)


def test_gapless_is_not_the_gapped_score(swg, orc):
    """The restatement on a relative with one indel between two 40-residue flanks: strictly below the gapped score."""
    rng = np.random.default_rng(7)
    sub = _tables(swg)["blosum62"]
    q = rng.integers(1, 21, size=80).astype(np.int8)
    d = np.concatenate([q[:40], rng.integers(1, 21, size=1), q[40:]]).astype(np.int8)
    flat, off = gc.pack([d])
    gapped = int(orc.score_db(q, flat, off, sub, -11, -1)[0])
    gapless = int(gc.oracle_gapless(orc, q, flat, off, sub)[0])
    assert gapless == int(gc.gapless_numpy(q, flat, off, sub)[0]) and 0 < gapless < gapped


@pytest.fixture(scope="module")
def plan_db(swg):
    flat, off = swg.synth_db(0x6A9, 1000)
    db = swg.Database(flat, off)
    yield db
    db.close()


@pytest.mark.parametrize("lq", [1, 128, 367, 500, 2048])
def test_plan_route_1_covers_the_query_in_one_pass(plan_db, lq):
    p = plan_db.debug_plan_gapless(lq)
    assert p["route"] == 1 and p["passes"] == 1, p
    assert p["G"] in (16, 32, 64) and 2 <= p["K"] <= 32 and p["G"] * p["K"] >= lq, p
    assert p["W"] >= 1 and p["workgroups"] >= 1, p


@pytest.mark.parametrize("lq", [2049, 3000])
def test_plan_route_0_beyond_one_pass(plan_db, lq):
    p = plan_db.debug_plan_gapless(lq)
    assert p["route"] == 0 and p["G"] * p["K"] * p["passes"] >= lq, p


def test_plan_hooks_of_the_gapped_searches_keep_their_outputs(plan_db):
    """swg_debug_plan / swg_debug_plan_f16 answer as before a gapless plan was asked for (the planner's one-entry cache
    is keyed by the cells)."""
    before = (plan_db.debug_plan(367), plan_db.debug_plan(367, f16_pair=0))
    plan_db.debug_plan_gapless(367)
    assert (plan_db.debug_plan(367), plan_db.debug_plan(367, f16_pair=0)) == before
