"""GPU (-m gpu): alignments of a batch's hits in one call (swg_align_hits_multi, swg_align_hits_multi_pssm,
Context.align_hits_multi / align_hits_multi_pssm, the CLI's --allqueries --align).

Each batch must be, field for field and path for path, what the per-query loop gives: swg_set_query (or
swg_set_query_pssm) with that query, then swg_align_hits, on the same build.  Index queries are also checked against
the int32 oracle's traceback and path score, as test_gpu_align does; PSSM paths are re-scored with the PSSM itself."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, golden_names, load_golden
from test_gpu_align import _check
from test_gpu_pssm_multi import _blocks, _path_score
from test_pssm_host import letters, write_ascii_pssm

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "seq-align-gpu_amd", "bin", "smith_waterman")
B62 = os.path.join(ROOT, "seq-align-gpu_amd", "data", "BLOSUM62.txt")
DIR_BUDGET = 2 << 30   # predecessor bytes one launch of the trace kernel may use (swg_trace.hip)


@pytest.fixture(scope="module")
def actx(swg):
    c = swg.Context(0)
    c.set_option("autotune", 0)
    yield c
    c.close()


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _loop(c, db, queries, hits, want_ops=True, pssm=False):
    """The per-query loop the batch call replaces."""
    out = []
    for q, row in zip(queries, hits):
        (c.set_query_pssm if pssm else c.set_query)(q)
        out.append(c.align_hits(db, row, want_ops=want_ops))
    return out


def _oracle_check(orc, queries, flat, off, sub, go, ge, got):
    for q, row in zip(queries, got):
        _check(orc, q, flat, off, sub, go, ge, row)


def _other_lengths(lq):
    return [L if L != lq else L + 1 for L in (17, 150, 700)]


# ---- 1. every golden fixture: its query and three of other lengths ----------------------------------------------
@pytest.mark.parametrize("name", golden_names())
def test_batch_alignments_of_golden_hits(swg, orc, actx, name):
    g = load_golden(name)
    go, ge = int(g["gaps"][0]), int(g["gaps"][1])
    actx.set_scoring(g["sub"], go, ge)
    db = swg.Database(g["flat"], g["offsets"]).upload(actx)
    qs = [g["query"]] + [swg.synth_query(0xA11 + L, L) for L in _other_lengths(len(g["query"]))]
    _, hits, _ = actx.search_multi(db, qs, k=12, want_scores=False)
    got = actx.align_hits_multi(db, qs, hits)
    assert got == _loop(actx, db, qs, hits)
    for row, h in zip(got, hits):
        assert [a["index"] for a in row] == [i for _, i in h]
        assert [a["score"] for a in row] == [s for s, _ in h]
    ref = g["ref16"].astype(np.int32) if g["ref_valid"][0] else g["oracle32"]
    _check(orc, g["query"], g["flat"], g["offsets"], g["sub"], go, ge, got[0], ref)
    _oracle_check(orc, qs[1:], g["flat"], g["offsets"], g["sub"], go, ge, got[1:])
    db.close()


# ---- 2. LDS and non-LDS queries in one call --------------------------------------------------------------------
def test_batch_mixes_lds_and_global_diagonals(swg, orc, actx):
    sc = swg.load_scoring("PAM250").table()
    base = swg.synth_query(0xA12, 2500)
    flat, off, planted = swg.synth_db(0xA12, 160, query=base, fraction=0.1, subst=0.05, max_len=5000)
    assert planted > 0
    lens = np.diff(off.astype(np.int64))
    longest = int(np.argmax(lens))
    qs = [base[:60].copy(), base[:1700].copy(), base[300:2001].copy(), base]      # 60, 1700, 1701, 2500 columns
    assert [len(q) for q in qs] == [60, 1700, 1701, 2500]
    actx.set_scoring(sc, -2, -1)
    db = swg.Database(flat, off).upload(actx)
    scores, hits, _ = actx.search_multi(db, qs, k=5)
    hits = [h if any(i == longest for _, i in h) else h + [(int(scores[r][longest]), longest)] for r, h in enumerate(hits)]
    got = actx.align_hits_multi(db, qs, hits)
    assert got == _loop(actx, db, qs, hits)
    for r, row in enumerate(got):
        assert [a["score"] for a in row] == [int(scores[r][a["index"]]) for a in row]
    _oracle_check(orc, qs, flat, off, sc, -2, -1, got)
    db.close()


# ---- 3. more predecessor bytes than one launch takes -----------------------------------------------------------
def test_batch_cut_into_several_launches(swg, actx):
    """8 queries of 3000 columns x 16 sequences of about 5000 residues: about 3 GB of predecessor bytes, so the call
    cuts more than one launch.  Compared with the loop only (the CPU oracle at this size would dominate the suite)."""
    sc = swg.load_scoring("BLOSUM62").table()
    flat, off = swg.synth_db(0xA13, 16, median=5000.0, sigma_ln=0.01, min_len=4900, max_len=5100)
    lens = np.diff(off.astype(np.int64))
    qs = [swg.synth_query(0xA130 + i, 3000) for i in range(8)]
    actx.set_scoring(sc, -11, -1)
    db = swg.Database(flat, off).upload(actx)
    _, hits, _ = actx.search_multi(db, qs, k=16, want_scores=False)
    assert all(len(h) == 16 for h in hits)
    need = sum((len(q) + int(lens[i]) - 1) * len(q) for q, h in zip(qs, hits) for _, i in h)
    print("predecessor bytes %d, budget per launch %d" % (need, DIR_BUDGET))
    assert need > DIR_BUDGET
    got = actx.align_hits_multi(db, qs, hits)
    assert got == _loop(actx, db, qs, hits)
    assert all(a["score"] == s for row, h in zip(got, hits) for a, (s, _) in zip(row, h))
    db.close()


# ---- 4. PSSMs -----------------------------------------------------------------------------------------------------
def test_batch_pssm_equal_to_table_is_the_index_batch(swg, orc, actx):
    sc = swg.load_scoring("BLOSUM62").table()
    flat, off = swg.synth_db(0x5EED0001, 1024)                         # config 1's database
    qs = [swg.synth_query(0xA14 + i, L) for i, L in enumerate((128, 60, 1750, 128, 1))]
    actx.set_scoring(sc, -2, -1)
    db = swg.Database(flat, off).upload(actx)
    _, hits, _ = actx.search_multi(db, qs, k=8, want_scores=False)
    pssms = [sc[q.astype(np.int64)] for q in qs]
    got_idx = actx.align_hits_multi(db, qs, hits)
    got_p = actx.align_hits_multi_pssm(db, pssms, hits)
    assert got_p == got_idx
    assert got_p == _loop(actx, db, pssms, hits, pssm=True)
    _oracle_check(orc, qs, flat, off, sc, -2, -1, got_idx)
    db.close()


def test_batch_pssm_random_columns(swg, actx):
    rng = np.random.default_rng(0xA15)
    flat, off = swg.synth_db(0xA15, 700, max_len=2000)
    actx.set_scoring(np.zeros((32, 32), dtype=np.int8), -11, -1)      # the table is not read while PSSMs score
    db = swg.Database(flat, off).upload(actx)
    pssms = [rng.integers(-128, 128, size=(L, 32)).astype(np.int8) for L in (1, 40, 128, 600, 1701)]
    _, hits, _ = actx.search_multi_pssm(db, pssms, k=6, want_scores=False)
    got = actx.align_hits_multi_pssm(db, pssms, hits)
    assert got == _loop(actx, db, pssms, hits, pssm=True)
    n = 0
    for p, row, h in zip(pssms, got, hits):
        assert [a["score"] for a in row] == [s for s, _ in h]
        for a in row:
            assert _path_score(p, flat[int(off[a["index"]]):int(off[a["index"] + 1])], -11, -1, a) == a["score"]
            n += 1
    assert n == sum(len(h) for h in hits) > 0
    db.close()


# ---- 5. row shapes -------------------------------------------------------------------------------------------------
def _raw(swg, c, db, qs, rows, k, out, ops=None, stride=0):
    qoff = np.zeros(len(qs) + 1, dtype=np.uint64)
    qoff[1:] = np.cumsum([len(q) for q in qs])
    qflat = np.ascontiguousarray(np.concatenate(qs) if qs else np.zeros(0), dtype=np.int8)
    hits = (swg.Hit * max(len(qs) * k, 1))()
    nh = (C.c_size_t * max(len(qs), 1))()
    for i, row in enumerate(rows):
        nh[i] = len(row)                             # (may pass k: the call must refuse that before it reads a hit)
        for j, (s, ix) in enumerate(row[:k]):
            hits[i * k + j].score, hits[i * k + j].index = s, ix
    return swg.lib.swg_align_hits_multi(c.handle, db.handle, _vp(qflat), _vp(qoff), len(qs), C.cast(hits, C.c_void_p), k,
                                        C.cast(nh, C.c_void_p), C.cast(out, C.c_void_p),
                                        C.cast(ops, C.c_void_p) if ops is not None else None, stride)


def test_batch_row_shapes(swg, orc, actx):
    sc = swg.load_scoring("BLOSUM62").table()
    flat, off = swg.synth_db(0xA16, 300)
    qs = [swg.synth_query(0xA160 + i, L) for i, L in enumerate((90, 45, 200, 130))]
    actx.set_scoring(sc, -2, -1)
    db = swg.Database(flat, off).upload(actx)
    _, hits, _ = actx.search_multi(db, qs, k=5)
    shared = hits[1][:1] + hits[3][:1]
    rows = [[],                                      # no hits
            hits[1][:2],                             # fewer than k
            shared + [h for h in hits[2] if h[1] not in {i for _, i in shared}][:2],   # sequences rows 1 and 3 hold
            hits[3][::-1]]                           # out of score order
    ix = [{i for _, i in r} for r in rows]
    assert ix[2] & ix[1] and ix[2] & ix[3]
    got = actx.align_hits_multi(db, qs, rows)
    assert [len(r) for r in got] == [len(r) for r in rows]
    assert got == _loop(actx, db, qs, rows)
    _oracle_check(orc, qs, flat, off, sc, -2, -1, got)
    bare = actx.align_hits_multi(db, qs, rows, want_ops=False)
    assert bare == [[{f: v for f, v in a.items() if f != "ops"} for a in row] for row in got]
    # slots past a row's count, and every slot of an empty row, are not written
    k = 5
    out = (swg.Alignment * (len(qs) * k))()
    for a in out:
        a.score = -7
    assert _raw(swg, actx, db, qs, rows, k, out) == swg.SWG_OK
    for i, row in enumerate(rows):
        for j in range(k):
            assert (out[i * k + j].score == -7) == (j >= len(row)), (i, j)
    # no queries, or no hits at all: SWG_OK, nothing written
    assert actx.align_hits_multi(db, [], []) == []
    for a in out:
        a.score = -7
    assert _raw(swg, actx, db, qs, [[], [], [], []], k, out) == swg.SWG_OK
    assert _raw(swg, actx, db, [], [], k, out) == swg.SWG_OK
    assert all(a.score == -7 for a in out)
    # ops_stride: the bound works; one byte less than the longest path needs does not
    qoff = np.concatenate([[0], np.cumsum([len(q) for q in qs])]).astype(np.uint64)
    bound = swg.lib.swg_align_ops_bound_multi(db.handle, _vp(qoff), len(qs))
    assert actx.align_hits_multi(db, qs, rows, ops_stride=bound) == got
    need = max(a["n_ops"] for row in got for a in row) + 1
    assert actx.align_hits_multi(db, qs, rows, ops_stride=need) == got
    with pytest.raises(swg.SwgError) as e:
        actx.align_hits_multi(db, qs, rows, ops_stride=need - 1)
    assert e.value.code == swg.SWG_ERR_ARG
    db.close()


# ---- 6. the context's own query is neither read nor changed -----------------------------------------------------
def test_batch_keeps_the_context_query(swg, actx):
    rng = np.random.default_rng(0xA17)
    sc = swg.load_scoring("BLOSUM62").table()
    flat, off = swg.synth_db(0xA17, 500)
    actx.set_scoring(sc, -2, -1)
    db = swg.Database(flat, off).upload(actx)
    qs = [swg.synth_query(0xA170 + i, L) for i, L in enumerate((70, 1800, 128))]
    _, hits, _ = actx.search_multi(db, qs, k=4, want_scores=False)
    pssms = [rng.integers(-20, 21, size=(len(q), 32)).astype(np.int8) for q in qs]
    own_q = swg.synth_query(0xA171, 111)
    own_p = rng.integers(-10, 11, size=(95, 32)).astype(np.int8)
    for set_own in (lambda: actx.set_query(own_q), lambda: actx.set_query_pssm(own_p)):
        set_own()
        before_s, before_h, _ = actx.search(db, k=6)
        before_a = actx.align_hits(db, before_h)
        before_bound = swg.lib.swg_align_ops_bound(actx.handle, db.handle)
        actx.align_hits_multi(db, qs, hits)
        actx.align_hits_multi_pssm(db, pssms, hits)
        after_s, after_h, _ = actx.search(db, k=6)
        assert np.array_equal(after_s, before_s) and after_h == before_h
        assert actx.align_hits(db, after_h) == before_a
        assert swg.lib.swg_align_ops_bound(actx.handle, db.handle) == before_bound
    db.close()


# ---- 7. errors -----------------------------------------------------------------------------------------------------
def test_batch_errors(swg, actx):
    sc = swg.load_scoring("BLOSUM62").table()
    flat, off = swg.synth_db(0xA18, 300)
    actx.set_scoring(sc, -2, -1)
    db = swg.Database(flat, off).upload(actx)
    qs = [swg.synth_query(0xA180, 50), swg.synth_query(0xA181, 80)]
    _, hits, _ = actx.search_multi(db, qs, k=3, want_scores=False)
    good = actx.align_hits_multi(db, qs, hits)

    def code(fn, *a, **kw):
        with pytest.raises(swg.SwgError) as e:
            fn(*a, **kw)
        return e.value.code

    # queries: empty (offsets not increasing), residues outside 1..31, longer than 2^24
    assert code(actx.align_hits_multi, db, [qs[0], np.zeros(0, dtype=np.int8)], hits) == swg.SWG_ERR_ARG
    bad = qs[1].copy()
    bad[7] = 0
    assert code(actx.align_hits_multi, db, [qs[0], bad], hits) == swg.SWG_ERR_RESIDUE
    bad[7] = 32
    assert code(actx.align_hits_multi, db, [qs[0], bad], hits) == swg.SWG_ERR_RESIDUE
    huge = np.ones((1 << 24) + 1, dtype=np.int8)
    assert code(actx.align_hits_multi, db, [huge], [hits[0]]) == swg.SWG_ERR_ARG
    assert code(actx.align_hits_multi_pssm, db, [np.zeros((8, 32), dtype=np.int8), np.zeros((0, 32), dtype=np.int8)],
                hits) == swg.SWG_ERR_ARG
    # n_hits[i] > k
    out = (swg.Alignment * 8)()
    assert _raw(swg, actx, db, qs, [hits[0][:3], hits[1][:3]], 2, out) == swg.SWG_ERR_ARG
    # a hit that is not in this shard; a shard's own hit works
    half = swg.Database(flat, off, shard_rank=1, shard_count=2).upload(actx)
    mine = set(int(i) for i in half.order() if i != 0xFFFFFFFF)
    other = next(i for i in range(300) if i not in mine)
    assert code(actx.align_hits_multi, half, qs, [[(0, next(iter(mine)))], [(0, other)]]) == swg.SWG_ERR_ARG
    assert code(actx.align_hits_multi, db, qs, [[(0, 300)], []]) == swg.SWG_ERR_ARG       # no such sequence
    ok = actx.align_hits_multi(half, qs, [[(0, next(iter(mine)))], []])
    assert ok[0][0]["index"] in mine
    half.close()
    # a pair too large for a traceback ((lq + len) * lq past 16 Gi cells)
    assert code(actx.align_hits_multi, db, [np.ones(1 << 17, dtype=np.int8)], [[hits[0][0]]], want_ops=False) \
        == swg.SWG_ERR_ARG
    # more than 2^20 hits in all
    many = (1 << 20) + 1
    big = (swg.Alignment * 1)()
    qoff = np.array([0, 50], dtype=np.uint64)
    hh = (swg.Hit * many)()
    nh = (C.c_size_t * 1)(many)
    assert swg.lib.swg_align_hits_multi(actx.handle, db.handle, _vp(qs[0]), _vp(qoff), 1, C.cast(hh, C.c_void_p), many,
                                        C.cast(nh, C.c_void_p), C.cast(big, C.c_void_p), None, 0) == swg.SWG_ERR_ARG
    # ops_stride 0 with ops; NULL queries
    assert code(actx.align_hits_multi, db, qs, hits, ops_stride=0) == swg.SWG_ERR_ARG
    assert swg.lib.swg_align_hits_multi(actx.handle, db.handle, None, _vp(qoff), 1, C.cast(hh, C.c_void_p), 1,
                                        C.cast(nh, C.c_void_p), C.cast(big, C.c_void_p), None, 0) == swg.SWG_ERR_ARG
    # a database that is not resident
    cold = swg.Database(flat, off)
    assert code(actx.align_hits_multi, cold, qs, hits) == swg.SWG_ERR_STATE
    assert code(actx.align_hits_multi_pssm, cold, [sc[q.astype(np.int64)] for q in qs], hits) == swg.SWG_ERR_STATE
    cold.close()
    # after every failure the context still works
    assert actx.align_hits_multi(db, qs, hits) == good
    db.close()
    # no scoring
    c = swg.Context(0)
    try:
        d2 = swg.Database(flat, off).upload(c)
        assert code(c.align_hits_multi, d2, qs, hits) == swg.SWG_ERR_STATE
        assert code(c.align_hits_multi_pssm, d2, [sc[q.astype(np.int64)] for q in qs], hits) == swg.SWG_ERR_STATE
        d2.close()
    finally:
        c.close()


# ---- 8. the CLI: --allqueries --topk 5 --align ---------------------------------------------------------------
def _run(*a):
    r = subprocess.run([CLI, "--substitution_matrix", B62] + [str(x) for x in a], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r.stdout


def _alone(*a):
    """One record run on its own: its block without the `Query File=` line and the Total Time line."""
    return [l for l in _run(*a).splitlines()[1:] if not l.startswith("Total Time:")]


def test_cli_allqueries_align(swg, tmp_path):
    flat, off = swg.synth_db(0x5EED9, 600)
    df = tmp_path / "d.fa"
    df.write_text("".join(">s%d\n%s\n" % (i, letters(swg, flat[int(off[i]):int(off[i + 1])]))
                          for i in range(len(off) - 1)))
    recs = [letters(swg, swg.synth_query(0xA19 + r, L)) for r, L in enumerate((160, 90, 1800, 40, 300))]
    recs[1] = recs[1].lower()
    qf = tmp_path / "q.fa"
    qf.write_text("".join(">rec%d\n%s\n" % (r, s) for r, s in enumerate(recs)))
    blocks = _blocks(_run("--allqueries", "--topk", "5", "--align", "--files", qf, df))
    assert sorted(blocks) == list(range(len(recs)))
    for r, s in enumerate(recs):
        one = tmp_path / ("one%d.fa" % r)
        one.write_text(">rec%d\n%s\n" % (r, s))
        alone = _alone("--topk", "5", "--align", "--files", one, df)
        assert sum(l.startswith("Alignment #") for l in alone) == 5
        assert blocks[r] == alone, r


def test_cli_allqueries_align_pssmlist(swg, tmp_path):
    sc = swg.load_scoring("BLOSUM62")
    rng = np.random.default_rng(0xA1A)
    flat, off = swg.synth_db(0x5EED9, 600)
    df = tmp_path / "d.fa"
    df.write_text("".join(">s%d\n%s\n" % (i, letters(swg, flat[int(off[i]):int(off[i + 1])]))
                          for i in range(len(off) - 1)))
    recs, pfs = [], []
    for r, L in enumerate((160, 90, 1750, 200)):
        q = swg.synth_query(0xA1A0 + r, L)
        ql = letters(swg, q)
        pf = tmp_path / ("r%d.pssm" % r)
        write_ascii_pssm(pf, ql, rng.integers(-6, 9, size=(32, 20))[q.astype(np.int64)])
        recs.append(ql)
        pfs.append(pf)
    qf, lf = tmp_path / "q.fa", tmp_path / "list.txt"
    qf.write_text("".join(">rec%d\n%s\n" % (r, s) for r, s in enumerate(recs)))
    lf.write_text("".join("%s\n" % p for p in pfs))
    blocks = _blocks(_run("--allqueries", "--pssmlist", lf, "--topk", "5", "--align", "--files", qf, df))
    assert sorted(blocks) == list(range(len(recs)))
    for r, s in enumerate(recs):
        one = tmp_path / ("one%d.fa" % r)
        one.write_text(">rec%d\n%s\n" % (r, s))
        alone = _alone("--pssm", pfs[r], "--topk", "5", "--align", "--files", one, df)
        assert sum(l.startswith("Alignment #") for l in alone) == 5
        assert blocks[r] == alone, r


def test_cli_allqueries_align_past_2_20_hits(swg, tmp_path):
    """520 records of 2 aa, --topk 2048 against 2 048 sequences of 1-4 aa: the 519 records after the first hold more
    than 2^20 hits in one search chunk, more than one alignment call takes, so the tool cuts the chunk into several
    calls.  The run succeeds, and the records around the cut print what they print when run on their own."""
    flat, off = swg.synth_db(0xA1B, 2048, median=2.0, sigma_ln=0.5, min_len=1, max_len=4)
    n = len(off) - 1
    df = tmp_path / "d.fa"
    df.write_text("".join(">s%d\n%s\n" % (i, letters(swg, flat[int(off[i]):int(off[i + 1])])) for i in range(n)))
    recs = [letters(swg, swg.synth_query(0xA1B0 + r, 2)) for r in range(520)]
    assert (len(recs) - 1) * n > 1 << 20
    qf = tmp_path / "q.fa"
    qf.write_text("".join(">rec%d\n%s\n" % (r, s) for r, s in enumerate(recs)))
    r = subprocess.run([CLI, "--substitution_matrix", B62, "--allqueries", "--topk", str(n), "--align", "--files",
                        str(qf), str(df)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = r.stdout
    assert out.count("\nAlignment #") == len(recs) * n
    for rec in (0, 1, 511, 512, 513, 519):
        b = out.index("\nQuery #%d: " % rec) + 1
        e = out.find("\nQuery #%d: " % (rec + 1), b)
        block = [l for l in out[b:e + 1 if e >= 0 else len(out)].splitlines()[1:] if not l.startswith("Total Time:")]
        one = tmp_path / ("one%d.fa" % rec)
        one.write_text(">rec%d\n%s\n" % (rec, recs[rec]))
        assert block == _alone("--topk", str(n), "--align", "--files", one, df), rec


def test_cli_allqueries_align_error_after_the_records_before_it(swg, tmp_path):
    """A record whose pairs are too large for a traceback (131 072 columns: (lq + len) * lq past 2^34 cells) in the
    middle of a search chunk: the records before it print in full, then its own block up to its alignments, then the
    error -- the stdout of the records run one at a time."""
    flat, off = swg.synth_db(0xA1C, 40, median=60.0, max_len=100)
    df = tmp_path / "d.fa"
    df.write_text("".join(">s%d\n%s\n" % (i, letters(swg, flat[int(off[i]):int(off[i + 1])])) for i in range(40)))
    recs = [letters(swg, swg.synth_query(0xA1C0 + r, L)) for r, L in enumerate((50, 70, 1 << 17, 40))]
    qf = tmp_path / "q.fa"
    qf.write_text("".join(">rec%d\n%s\n" % (r, s) for r, s in enumerate(recs)))

    def run(*a):
        return subprocess.run([CLI, "--substitution_matrix", B62] + [str(x) for x in a], stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, text=True, timeout=300)

    r = run("--allqueries", "--topk", "2", "--align", "--files", qf, df)
    assert r.returncode != 0 and "outside what a traceback holds" in r.stderr, r.stderr
    blocks = _blocks(r.stdout)
    assert sorted(blocks) == [0, 1, 2]
    for rec in range(3):
        one = tmp_path / ("one%d.fa" % rec)
        one.write_text(">rec%d\n%s\n" % (rec, recs[rec]))
        alone = run("--topk", "2", "--align", "--files", one, df)
        assert (alone.returncode == 0) == (rec < 2), alone.stderr
        assert blocks[rec] == [l for l in alone.stdout.splitlines()[1:] if not l.startswith("Total Time:")], rec
    assert sum(l.startswith("Alignment #") for l in blocks[2]) == 0
