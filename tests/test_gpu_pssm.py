"""GPU (-m gpu): position-specific queries (swg_set_query_pssm) through every layer -- search, streaming, the
multi-query fallback, the re-score ceilings, traceback, the reference-shaped batches, groups and the CLI.

The oracle takes index queries over one table.  A PSSM with at most 31 distinct columns is exactly such a query:
q'[i] = the id (1..31) of position i's column, sub'[id] = that column.  So every PSSM below that has at most 31
distinct columns is checked bit for bit against orc.score_db / orc.pair_trace on (q', sub'); fully general PSSMs
(every position its own column) against the numpy restatement of test_pssm_host.py, at small sizes."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, golden_names, load_golden
from test_pssm_host import PSIBLAST_COLS, letters, sw_numpy, write_ascii_pssm

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "seq-align-gpu_amd", "bin", "smith_waterman")
B62 = os.path.join(ROOT, "seq-align-gpu_amd", "data", "BLOSUM62.txt")
ENTRY_RX = re.compile(r"Entry\s+#(\d+):\s*score:\s*([+-]?\d+)", re.IGNORECASE)
PLAN_FIELDS = ("engine", "cell_form", "cols_per_wave", "group_lanes", "passes", "fill_launches", "n_rescored")


@pytest.fixture(scope="module")
def pctx(swg):
    c = swg.Context(0)
    yield c
    c.close()


def _options(c, **kw):
    base = dict(force_bits=0, engine=0, f16=1, autotune=0, wide16=1, last_pass=1, work_queue=1)
    base.update(kw)
    for k, v in base.items():
        c.set_option(k, v)


def _pssm31(rng, lq, lo=-128, hi=127):
    """A random position-specific query of at most 31 distinct columns -> (pssm[lq, 32], q', sub')."""
    subp = np.zeros((32, 32), dtype=np.int8)
    subp[1:, 1:] = rng.integers(lo, hi + 1, size=(31, 31))
    qp = rng.integers(1, 32, size=lq).astype(np.int8)
    return subp[qp.astype(np.int64)], qp, subp


def _path_score(pssm, d, go, ge, a):
    """An alignment's path score recomputed with the PSSM itself."""
    i, j, tot, prev = a["q_begin"], a["d_begin"], 0, ""
    for op in a["ops"]:
        if op == "M":
            tot += int(pssm[i, int(d[j])]); i += 1; j += 1
        elif op == "I":
            tot += ge if prev == "I" else go + ge; j += 1
        else:
            tot += ge if prev == "D" else go + ge; i += 1
        prev = op
    assert (i, j) == (a["q_end"], a["d_end"])
    return tot


# ---- 1. a PSSM equal to sub[q] is the index query q: same scores, top-K and plan -------------------------------
@pytest.mark.parametrize("opts", [{}, {"engine": 1}, {"f16": 0}, {"f16": 2}, {"force_bits": 32}],
                         ids=["default", "engine1", "f16_0", "f16_2", "int32"])
def test_pssm_equals_index_query_on_golden(swg, pctx, opts):
    for name in golden_names():
        g = load_golden(name)
        go, ge = int(g["gaps"][0]), int(g["gaps"][1])
        if opts.get("engine") == 1 and not (go <= 0 and ge <= 0):
            continue                              # (the systolic engine is int16 only: such rows run on int32)
        _options(pctx, **opts)
        pctx.set_scoring(g["sub"], go, ge)
        db = swg.Database(g["flat"], g["offsets"]).upload(pctx)
        pctx.set_query(g["query"])
        s_idx, h_idx, st_idx = pctx.search(db, k=10)
        pctx.set_query_pssm(g["sub"][g["query"].astype(np.int64)])
        s_p, h_p, st_p = pctx.search(db, k=10)
        assert np.array_equal(s_p, g["oracle32"]), (name, opts)
        assert np.array_equal(s_p, s_idx) and h_p == h_idx, (name, opts)
        assert {f: st_p[f] for f in PLAN_FIELDS} == {f: st_idx[f] for f in PLAN_FIELDS}, (name, opts, st_p, st_idx)
        db.close()
    _options(pctx)


# ---- 2. position-specific columns ------------------------------------------------------------------------------
def test_pssm_random_columns_against_oracle(swg, orc, pctx):
    rng = np.random.default_rng(2024)
    flat, off = swg.synth_db(0xC0FFEE, 3000, median=180.0, min_len=1, max_len=1500)
    _options(pctx)
    pctx.set_scoring(np.zeros((32, 32), dtype=np.int8), -11, -1)     # the table is not read while a PSSM is set
    db = swg.Database(flat, off).upload(pctx)
    for lq in (1, 128, 500, 3000):
        pssm, qp, subp = _pssm31(rng, lq)
        pctx.set_query_pssm(pssm)
        scores, hits, st = pctx.search(db, k=20)
        want = orc.score_db(qp, flat, off, subp, -11, -1)
        assert np.array_equal(scores, want), (lq, st)
        assert hits == orc.topk(want, 20)
        if lq == 3000:
            assert st["passes"] > 1, st
    db.close()


def test_pssm_general_columns_against_numpy(swg, pctx):
    """Every position its own column (more than 31 distinct ones): against the numpy restatement."""
    rng = np.random.default_rng(99)
    flat, off = swg.synth_db(0xBEEF, 200, median=50.0, sigma_ln=0.5, min_len=1, max_len=120)
    _options(pctx)
    pctx.set_scoring(np.zeros((32, 32), dtype=np.int8), -10, -1)
    db = swg.Database(flat, off).upload(pctx)
    for lq in (1, 17, 64):
        pssm = rng.integers(-128, 128, size=(lq, 32)).astype(np.int8)
        pctx.set_query_pssm(pssm)
        scores, _, _ = pctx.search(db)
        assert np.array_equal(scores, sw_numpy(pssm, flat, off, -10, -1)), lq
    db.close()


# ---- 3. every ceiling: f16 (4096), int16 (32767), wide (65535) -----------------------------------------------
@pytest.mark.parametrize("lq,least,opts", [(120, 4096, {"engine": 2}), (800, 32767, {"wide16": 0}), (1600, 65535, {})],
                         ids=["f16", "int16", "wide"])
def test_pssm_ceilings_rescored_exactly(swg, orc, pctx, lq, least, opts):
    """Columns boosted to ~10x BLOSUM62 and near-copies of the query planted: the best scores pass the ceiling of the
    cells they run on (the f16 cells' 4096; int16's 32767 with the wide form off; the wide form's 65535); the flagged
    sequences are re-scored and every score is exact.  The plan is the index query's over the same table."""
    rng = np.random.default_rng(lq)
    sub = swg.load_scoring("BLOSUM62").table().astype(np.int64)
    subp = np.clip(sub * 10 + rng.integers(-3, 4, size=(32, 32)), -128, 127).astype(np.int8)
    subp[:, 0] = 0
    q = swg.synth_query(lq, lq)
    flat, off, planted = swg.synth_db(lq, 1500, median=200.0, max_len=1700, query=q, fraction=0.01, subst=0.05)
    assert planted > 0
    _options(pctx, **opts)
    pctx.set_scoring(np.zeros((32, 32), dtype=np.int8), -11, -1)
    db = swg.Database(flat, off).upload(pctx)
    pctx.set_query_pssm(subp[q.astype(np.int64)])
    scores, hits, st = pctx.search(db, k=10)
    want = orc.score_db(q, flat, off, subp, -11, -1)
    assert np.array_equal(scores, want), st
    assert hits == orc.topk(want, 10)
    assert want.max() >= least and st["n_rescored"] > 0, (int(want.max()), st)
    if least == 4096:
        assert st["cell_form"] == 2, st
    # the same plan as the index query over the same table
    pctx.set_scoring(subp, -11, -1)
    pctx.set_query(q)
    s_idx, _, st_idx = pctx.search(db)
    assert np.array_equal(s_idx, want)
    assert {f: st[f] for f in PLAN_FIELDS} == {f: st_idx[f] for f in PLAN_FIELDS}, (st, st_idx)
    db.close()
    _options(pctx)


# ---- 4. streaming: PSSMs and index queries queued between search_begin calls ---------------------------------
def test_pssm_streamed_between_searches(swg, orc, pctx):
    rng = np.random.default_rng(4)
    flat, off = swg.synth_db(0x5EED4, 2000)
    sc = swg.load_scoring("BLOSUM62").table()
    _options(pctx)
    pctx.set_scoring(sc, -11, -1)
    db = swg.Database(flat, off).upload(pctx)
    p1, q1, s1 = _pssm31(rng, 300, -8, 8)
    q = swg.synth_query(44, 250)
    p2, q2, s2 = _pssm31(rng, 90, -20, 12)
    pctx.set_query_pssm(p1)
    t1 = pctx.search_begin(db, k=5, want_scores=True)
    pctx.set_query(q)
    t2 = pctx.search_begin(db, k=5, want_scores=True)
    pctx.set_query_pssm(p2)
    t3 = pctx.search_begin(db, k=5, want_scores=True)
    for t, (qq, ss) in zip((t1, t2, t3), ((q1, s1), (q, sc), (q2, s2))):
        scores, hits, _ = pctx.search_end(t)
        want = orc.score_db(qq, flat, off, ss, -11, -1)
        assert np.array_equal(scores, want)
        assert hits == orc.topk(want, 5)
    db.close()


# ---- 5. the one-query-at-a-time fallback of swg_search_multi puts the PSSM back ------------------------------
def test_search_multi_fallback_keeps_the_pssm(swg, orc, pctx):
    rng = np.random.default_rng(5)
    flat, off = swg.synth_db(0x5EED5, 1000)
    sc = swg.load_scoring("BLOSUM62").table()
    _options(pctx)
    pctx.set_scoring(sc, -11, -1)
    db = swg.Database(flat, off).upload(pctx)
    pssm, qp, subp = _pssm31(rng, 200, -10, 10)
    pctx.set_query_pssm(pssm)
    q = swg.synth_query(55, 150)
    ms, _, _ = pctx.search_multi(db, [q])
    assert np.array_equal(ms[0], orc.score_db(q, flat, off, sc, -11, -1))
    scores, _, _ = pctx.search(db)
    assert np.array_equal(scores, orc.score_db(qp, flat, off, subp, -11, -1))
    db.close()


# ---- 6. traceback ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lq", [200, 2000])        # the trace kernel's anti-diagonals in LDS, and in HBM beyond 1700
def test_pssm_alignments_of_hits(swg, orc, pctx, lq):
    rng = np.random.default_rng(lq + 6)
    flat, off = swg.synth_db(0x5EED6 + lq, 400, median=250.0)
    _options(pctx)
    go, ge = -10, -1
    pctx.set_scoring(np.zeros((32, 32), dtype=np.int8), go, ge)
    db = swg.Database(flat, off).upload(pctx)
    pssm, qp, subp = _pssm31(rng, lq, -12, 10)
    pctx.set_query_pssm(pssm)
    scores, hits, _ = pctx.search(db, k=8)
    assert swg.lib.swg_align_ops_bound(pctx.handle, db.handle) == lq + int(np.diff(off.astype(np.int64)).max()) + 1
    als = pctx.align_hits(db, hits)
    for (s, i), a in zip(hits, als):
        d = flat[int(off[i]):int(off[i + 1])]
        want_sc, co, ops = orc.pair_trace(qp, d, subp, go, ge)
        assert (a["score"], a["index"]) == (s, i) and want_sc == s
        assert (a["q_begin"], a["q_end"], a["d_begin"], a["d_end"]) == co and a["ops"] == ops
        assert _path_score(pssm, d, go, ge, a) == s
    db.close()


# ---- 7. the reference-shaped batches ---------------------------------------------------------------------------
def test_pssm_fill_batches16(swg, orc, pctx):
    """Padded rows ('*') are computed as real rows, like the reference does; scores saturate at 32767."""
    rng = np.random.default_rng(7)
    flat, off = swg.synth_db(0x5EED7, 128, median=300.0)
    _options(pctx)
    pctx.set_scoring(np.zeros((32, 32), dtype=np.int8), -11, -1)
    for lo, hi in ((-10, 10), (100, 127)):         # the second saturates (500 positions x >= 100 per residue)
        pssm, qp, subp = _pssm31(rng, 500, lo, hi)
        pctx.set_query_pssm(pssm)
        batches = orc.db_to_batches16(flat, off)
        lanes = [16] * len(batches)
        lanes[-1] = 11
        out, _ = pctx.fill_batches16(list(zip(batches, lanes)))
        for b, (o, vs) in enumerate(zip(out, lanes)):
            want = [min(orc.pair(qp, batches[b][:, l], subp, -11, -1), 32767) for l in range(vs)]
            assert o.tolist() == want, (lo, b)
        if lo > 0:
            assert max(max(o.tolist()) for o in out) == 32767


# ---- 8. a group ------------------------------------------------------------------------------------------------
def test_pssm_group_of_two_on_one_device(swg, pctx):
    rng = np.random.default_rng(8)
    flat, off = swg.synth_db(0x5EED8, 1500)
    pssm, _, _ = _pssm31(rng, 400, -10, 9)
    _options(pctx)
    pctx.set_scoring(np.zeros((32, 32), dtype=np.int8), -11, -1)
    pctx.set_query_pssm(pssm)
    db = swg.Database(flat, off).upload(pctx)
    want, want_hits, _ = pctx.search(db, k=10)
    db.close()
    grp = swg.Group([0, 0])
    try:
        grp.set_option("autotune", 0)
        grp.set_scoring(np.zeros((32, 32), dtype=np.int8), -11, -1)
        grp.set_query_pssm(pssm)
        grp.load(flat, off)
        scores, hits, _ = grp.search(k=10)
        assert np.array_equal(scores, want) and hits == want_hits
    finally:
        grp.close()


# ---- 9. argument errors ----------------------------------------------------------------------------------------
def test_pssm_argument_errors(swg):
    import ctypes as C
    c = swg.Context(0)
    try:
        buf = np.zeros(32, dtype=np.int8)
        bp = buf.ctypes.data_as(C.c_void_p)
        assert swg.lib.swg_set_query_pssm(None, bp, 1) == swg.SWG_ERR_ARG
        assert swg.lib.swg_set_query_pssm(c.handle, None, 1) == swg.SWG_ERR_ARG
        assert swg.lib.swg_set_query_pssm(c.handle, bp, 0) == swg.SWG_ERR_ARG
        # the length is refused before anything is read or allocated
        assert swg.lib.swg_set_query_pssm(c.handle, bp, (1 << 24) + 1) == swg.SWG_ERR_ARG
        assert swg.lib.swg_group_set_query_pssm(None, bp, 1) == swg.SWG_ERR_ARG
        # a PSSM search without scoring
        c.set_query_pssm(np.ones((8, 32), dtype=np.int8))
        flat, off = swg.synth_db(9, 64)
        db = swg.Database(flat, off).upload(c)
        with pytest.raises(swg.SwgError) as e:
            c.search(db)
        assert e.value.code == swg.SWG_ERR_STATE
        db.close()
    finally:
        c.close()


# ---- 10. the CLI ---------------------------------------------------------------------------------------------
def test_cli_pssm(swg, pctx, tmp_path):
    sc = swg.load_scoring("BLOSUM62")
    rng = np.random.default_rng(10)
    q = swg.synth_query(0x5EED10, 160)
    ql = letters(swg, q)
    scores20 = rng.integers(-6, 9, size=(len(ql), 20))
    flat, off = swg.synth_db(0x5EED10, 600)
    seqs = [letters(swg, flat[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)]
    qf, df, pf = tmp_path / "q.fa", tmp_path / "d.fa", tmp_path / "q.pssm"
    qf.write_text(">query\n" + ql.lower() + "\n")
    df.write_text("".join(">s%d\n%s\n" % (i, s) for i, s in enumerate(seqs)))
    write_ascii_pssm(pf, ql, scores20)
    pssm, pq = swg.read_pssm(str(pf), sc)
    assert np.array_equal(pq, q)
    _options(pctx)
    pctx.set_scoring(sc, -2, -1)
    pctx.set_query_pssm(pssm)
    db = swg.Database(flat, off).upload(pctx)
    want, want_hits, _ = pctx.search(db, k=5)
    db.close()
    assert not np.array_equal(want, np.zeros_like(want))
    for extra in ([], ["--gpus", "1"]):
        r = subprocess.run([CLI, "--substitution_matrix", B62, "--pssm", str(pf), "--topk", "5", "--align", *extra,
                            "--files", str(qf), str(df)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stderr
        got = {int(m.group(1)): int(m.group(2)) for m in ENTRY_RX.finditer(r.stdout)}
        assert got == {i: int(v) for i, v in enumerate(want)}, extra
        lines = r.stdout.splitlines()
        top = lines[lines.index("Top 5 hits (score, entry, name):") + 1:][:5]
        assert top == ["%d\t%d\ts%d" % (s, i, i) for s, i in want_hits], extra
        for k, (s, i) in enumerate(want_hits):
            assert any(l.startswith("Alignment #%d: entry %d score %d " % (k, i, s)) for l in lines), extra
    # the mismatch error, with a GPU present too
    other = tmp_path / "other.pssm"
    write_ascii_pssm(other, ("A" if ql[0] == "W" else "W") + ql[1:], scores20)
    r = subprocess.run([CLI, "--substitution_matrix", B62, "--pssm", str(other), "--files", str(qf), str(df)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode != 0 and "does not spell the query" in r.stderr
    r = subprocess.run([CLI, "--substitution_matrix", B62, "--pssm", str(pf), "--allqueries", "--files", str(qf), str(df)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert r.returncode != 0 and "--allqueries" in r.stderr
