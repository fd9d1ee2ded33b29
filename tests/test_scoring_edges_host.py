"""CPU: the builder of tests/scoring_edges.py and the oracle at the scoring-parameter edges.  What the GPU module
(test_gpu_scoring_edges.py) rests on, checked without a GPU: at every gap point the databases hold relatives whose
best alignment goes through a gap (so the gap magnitude shows in a score), the oracle's own paths add up to its scores
at magnitudes up to 65536, and the oracle equals the REFERENCE's alignment_fill_matrices (oracle/_ref, when built)
wherever the reference's int16 lanes can hold the scores."""
import numpy as np
import pytest

import scoring_edges as se
from conftest import ROOT  # noqa: F401  (path set-up)


def _db(p, n=49, salt=11, hi=31):
    rng = np.random.default_rng([p["g"], p["e"], salt])
    return se.split_db(p["g"], n, rng, hi=hi)


@pytest.mark.parametrize("p", se.GAP_POINTS, ids=se.point_id)
def test_builder_self_check(orc, p):
    """At least 5 of every 48 sequences are relatives whose oracle path holds an I or a D and whose oracle score is
    above what a flank scores alone; both kinds of gap occur; lengths 1 and 2 and an odd count are present; a copy
    scores 254 F."""
    sub = se.diag127()
    q, flat, off, kinds = _db(p)
    F = len(q) // 2
    assert F == se.flank_len(p["g"]) == max(8, p["g"] // 127 + 4)
    n_gap, n_i, n_d = se.gapped_relatives(orc, q, flat, off, kinds, sub, p["go"], p["ge"])
    assert n_gap >= 5 and n_i >= 1 and n_d >= 1, (n_gap, n_i, n_d)
    lens = np.diff(off.astype(np.int64))
    assert len(lens) % 2 == 1 and 1 in lens and 2 in lens
    want = orc.score_db(q, flat, off, sub, p["go"], p["ge"])
    assert (want[kinds == 0] == 254 * F).all()
    # a relative with one inserted residue scores 254 F - g exactly
    one = np.concatenate([q[:F], np.array([q[F - 1] % 31 + 1], dtype=np.int8), q[F:]])
    assert orc.pair(q, one, sub, p["go"], p["ge"]) == max(254 * F - p["g"], 127 * F)
    assert 254 * F - p["g"] > 127 * F


def test_builder_straddles_every_ceiling():
    f = se.flank_len
    assert 254 * f(2048) > 4096 > 254 * f(2048) - 2048                   # the f16 cells' ceiling
    assert 254 * f(16000) < 32767                                        # everything inside int16
    assert 254 * f(32767) >= 65535 > 254 * f(32767) - 32767 >= 32767     # beyond the wide form, and inside it only
    assert 254 * f(65536) - 65536 > 65535                                # int32 only
    assert se.payable(se.gap_point(-2047, -1), 4096) and se.payable(se.gap_point(-15999, -1), 32767)
    assert not se.payable(se.gap_point(-32766, -1), 32767) and se.payable(se.gap_point(-32766, -1), 65535)


def test_tables_are_what_they_say(swg):
    d = se.diag127()
    assert (np.diag(d) == 127).all() and d.min() == -128 and np.sort(d.ravel())[-33] == 126
    off_diag = d[~np.eye(32, dtype=bool)]
    assert ((off_diag <= -100) | (off_diag == 126)).all()
    z = se.diag127(zero0=True)
    assert not z[0].any() and not z[:, 0].any() and np.array_equal(z[1:, 1:], d[1:, 1:])
    f = se.full_range()
    assert f.min() == -128 and f.max() == 127 and f[0].any() and f[:, 0].any()
    assert (se.all_127() == 127).all() and (se.all_m128() == -128).all()
    b62 = swg.load_scoring("BLOSUM62").table()
    dirty = se.blosum62_dirty0(b62)
    assert np.array_equal(dirty[1:, 1:], b62[1:, 1:]) and not np.array_equal(dirty, b62)


@pytest.mark.parametrize("p", se.GAP_POINTS, ids=se.point_id)
def test_oracle_paths_add_up_at_every_gap_point(orc, p):
    """orc.path_score of every oracle path == its score, coordinates inside the pair, at every point."""
    sub = se.diag127()
    q, flat, off, kinds = _db(p, n=25, salt=12)
    want = orc.score_db(q, flat, off, sub, p["go"], p["ge"])
    for i, d in enumerate(se.seqs_of(flat, off)):
        sc, co, ops = orc.pair_trace(q, d, sub, p["go"], p["ge"])
        assert sc == int(want[i]) == orc.pair(q, d, sub, p["go"], p["ge"])
        assert orc.path_score(q, d, sub, p["go"], p["ge"], co, ops) == sc
        assert co[1] <= len(q) and co[3] <= len(d)


# (gap_open + gap_extend = -65536 is outside the reference's int16 score_t: its sum wraps to 0 there, so the last point
# has no reference to compare with -- the int32 oracle alone defines it)
@pytest.mark.parametrize("p", [p for p in se.GAP_POINTS if p["g"] <= 32768], ids=se.point_id)
def test_oracle_equals_the_reference_where_int16_holds(orc, p):
    """The reference's own alignment_fill_matrices on split_db, 16 lanes at a time, wherever every score of a batch
    stays at or below 32767 (its lanes wrap above).  Sequences are cut to 258 residues where they would
    score more (258 * 127 = 32766).  Residues 1 .. 26 only: the batches' filler is index 31, which must not match a
    query residue."""
    if not orc.have_ref():
        pytest.skip("oracle/_ref was not built (needs the reference sources at build time)")
    sub = se.diag127()
    q, flat, off, kinds = _db(p, n=49, salt=13, hi=26)
    seqs = [s[:258] if orc.pair(q, s, sub, p["go"], p["ge"]) > 32767 else s for s in se.seqs_of(flat, off)]
    seqs = seqs[:48]
    assert len(seqs) == 48
    n_checked = 0
    for b in range(0, 48, 16):
        batch = sorted(seqs[b:b + 16], key=len, reverse=True)
        want = np.array([orc.pair(q, s, sub, p["go"], p["ge"]) for s in batch])
        assert want.max() <= 32767
        ref = orc.ref_batch16(q, orc.make_batch16(batch), sub, p["go"], p["ge"])
        assert np.array_equal(ref.astype(np.int32), want), (se.point_id(p), b)
        n_checked += 16
    assert n_checked == 48


@pytest.mark.parametrize("name,go,ge", [("gapedge_2047_1", -2047, -1), ("gapedge_0_2048", 0, -2048), ("gapedge_2048_1", -2048, -1),
                                        ("gapedge_15999_1", -15999, -1), ("gapedge_32766_1", -32766, -1),
                                        ("gapedge_32767_1", -32767, -1)])
def test_gap_edge_fixtures_hold_what_they_are_for(orc, name, go, ge):
    """The reference-produced fixtures of make_golden.py --gap-edges: diag127 with row and column 0 zero, 48 records in
    batches of 16 with the first the longest, every score within the reference's int16 (ref_valid = 1, reference ==
    oracle), lengths 1 and 2 present -- and best paths through a gap wherever one can pay below 32767 (from g = 32767
    on none can: those two fixtures pin the hand-over to int32 on ungapped scores)."""
    from conftest import load_golden
    g = load_golden(name)
    assert (int(g["gaps"][0]), int(g["gaps"][1])) == (go, ge)
    assert np.array_equal(g["sub"], se.diag127(zero0=True))
    lens = np.diff(g["offsets"].astype(np.int64))
    assert len(lens) == 48 and all(lens[b] == lens[b:b + 16].max() for b in (0, 16, 32)) and 1 in lens and 2 in lens
    assert g["ref_valid"][0] == 1 and g["oracle32"].max() <= 32767
    assert np.array_equal(g["ref16"].astype(np.int32), g["oracle32"])
    assert np.array_equal(orc.score_db(g["query"], g["flat"], g["offsets"], g["sub"], go, ge), g["oracle32"])
    F = len(g["query"]) // 2
    gapped = 0
    for d in se.seqs_of(g["flat"], g["offsets"]):
        sc, _, ops = orc.pair_trace(g["query"], d, g["sub"], go, ge)
        gapped += sc > 127 * F and ("I" in ops or "D" in ops)
    assert gapped >= 5 if -(go + ge) <= 16000 else gapped == 0, gapped


def _lib_score_bound(swg, rows, idx, longest):
    """swg_debug_score_bound (csrc/swg_host_internal.h): (qbound, smax, bound) of a table + query indices, or of PSSM
    rows (idx None), against sequences of at most `longest` rows."""
    import ctypes as C
    fn = swg.lib.swg_debug_score_bound
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64, C.c_void_p]
    rows = np.ascontiguousarray(rows, dtype=np.int8)
    idx = None if idx is None else np.ascontiguousarray(idx, dtype=np.int8)
    out = np.zeros(3, dtype=np.uint64)
    lq = rows.shape[0] if idx is None else len(idx)
    assert fn(rows.ctypes.data, None if idx is None else idx.ctypes.data, lq, longest, out.ctypes.data) == 0
    return tuple(int(x) for x in out)


def _pssm_bound_model(pssm, longest):
    """A PSSM bounds by its own rows: each position's best entry over residues 1 .. 31 (never below 0), their sum, and
    the largest of them times min(lq, longest)."""
    best = np.asarray(pssm).astype(np.int64)[:, 1:].max(axis=1).clip(min=0)
    return int(best.sum()), int(best.max()), min(int(best.sum()), min(len(best), longest) * int(best.max()))


def test_score_bound_equals_the_python_model(swg):
    """The one bound every search and every batch plans by (swg_score_bound), against the model the GPU module's route
    expectations use (test_gpu_scoring_edges._score_bound), for a table query and for a PSSM, on both arms of the
    minimum: the query's best total, and min(lq, longest) x the largest entry."""
    from test_gpu_scoring_edges import _score_bound
    rng = np.random.default_rng(20261017)
    b62 = swg.load_scoring("BLOSUM62").table()
    arms = set()
    for sub in (b62, se.diag127(), se.full_range(), se.blosum62_dirty0(b62), se.all_m128()):
        for lq, max_len in ((1, 1), (37, 5), (37, 6), (300, 41), (300, 4000), (3000, 372), (3000, 35000)):
            q = rng.integers(1, 32, size=lq).astype(np.int8)
            lens = np.array([1, max_len])
            longest = (max_len + 3) // 4 * 4
            qbound, smax, bound = _lib_score_bound(swg, sub, q, longest)
            assert bound == _score_bound(sub, q, lens), (lq, max_len)
            assert smax == max(0, int(np.asarray(sub).max()))
            assert qbound == int(np.asarray(sub).astype(np.int64)[q.astype(np.int64)][:, 1:].max(axis=1).clip(min=0).sum())
            assert bound == min(qbound, min(lq, longest) * smax)
            arms.add("total" if qbound < min(lq, longest) * smax else "longest" if qbound > min(lq, longest) * smax else "tie")
            # the same query as a PSSM (its rows of the table): the same total; the largest entry is the rows' own
            pssm = np.asarray(sub)[q.astype(np.int64)]
            assert _lib_score_bound(swg, pssm, None, longest) == _pssm_bound_model(pssm, longest)
            assert _lib_score_bound(swg, pssm, None, longest)[0] == qbound
    assert {"total", "longest"} <= arms, arms
    # PSSMs of any int8, column 0 (never a database residue) holding the largest entries
    for lq, longest in ((1, 4), (50, 8), (50, 4000), (700, 64)):
        pssm = rng.integers(-128, 128, size=(lq, 32)).astype(np.int8)
        pssm[:, 0] = 127
        pssm[::3, 1:] = rng.integers(-128, 0, size=pssm[::3, 1:].shape)  # positions with no positive entry count 0
        got = _lib_score_bound(swg, pssm, None, longest)
        assert got == _pssm_bound_model(pssm, longest), (lq, longest)
    pssm = np.zeros((50, 32), dtype=np.int8)
    pssm[:, 5] = 100
    pssm[0, 7] = 127
    assert _lib_score_bound(swg, pssm, None, 8) == (5027, 127, 8 * 127)      # the min(lq, longest) * smax arm
    assert _lib_score_bound(swg, pssm, None, 4000) == (5027, 127, 5027)      # the query's best total
