"""GPU (-m gpu): batches of position-specific queries in one pass (swg_search_multi_pssm, Context.search_multi_pssm,
the CLI's --allqueries --pssmlist).

A PSSM equal to sub[q] is the index query q, so such a batch must give search_multi's scores, top-K and plan.  A PSSM
with at most 31 distinct columns is an index query over a synthetic table (q'[i] = the id of position i's column,
sub'[id] = that column), so those are checked bit for bit against orc.score_db; fully general PSSMs against the numpy
restatement of test_pssm_host.py, at small sizes."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, golden_names, load_golden
from test_pssm_host import letters, sw_numpy, write_ascii_pssm

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "seq-align-gpu_amd", "bin", "smith_waterman")
B62 = os.path.join(ROOT, "seq-align-gpu_amd", "data", "BLOSUM62.txt")
PLAN_FIELDS = ("engine", "cell_form", "cols_per_wave", "group_lanes", "waves", "passes", "fill_launches")


@pytest.fixture(scope="module")
def mctx(swg):
    c = swg.Context(0)
    yield c
    c.close()


def _options(c, **kw):
    base = dict(force_bits=0, engine=0, f16=1, qq=1, autotune=0, wide16=1, last_pass=1, work_queue=1)
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


def _bounds_agree(sub, qs, off):
    """Do sub[q] and q have the same score bound (search_multi's fast-path test) for every query?  A PSSM's smax is
    the largest entry of its own rows over residues 1..31, which can be below the table's; the bounds still agree
    where the sum of each position's best entry is below both products."""
    sub = np.asarray(sub, dtype=np.int64)
    smax_t = max(int(sub.max()), 0)
    longest = int(np.diff(np.asarray(off, dtype=np.int64)).max())
    for q in qs:
        rows = sub[np.asarray(q, dtype=np.int64)][:, 1:]
        best = np.maximum(rows.max(axis=1), 0)
        qbound, smax_p = int(best.sum()), int(best.max())
        cap = min(len(q), longest)
        if smax_p != smax_t and qbound > cap * smax_p:
            return False
    return True


def _same_as_index_batch(swg, c, db, sub, qs, off, k, **kw):
    """search_multi_pssm of sub[q] for q in qs against search_multi of qs: same scores and hits, same plan where the
    bounds agree.  -> (scores, hits, stats) of the PSSM batch."""
    s_idx, h_idx, st_idx = c.search_multi(db, qs, k=k, **kw)
    s_p, h_p, st_p = c.search_multi_pssm(db, [sub[np.asarray(q, dtype=np.int64)] for q in qs], k=k, **kw)
    if s_idx is not None:
        assert np.array_equal(s_p, s_idx)
    assert h_p == h_idx
    assert st_p["cells"] == st_idx["cells"] and st_p["bytes_alg"] == st_idx["bytes_alg"]
    if _bounds_agree(sub, qs, off):
        assert {f: st_p[f] for f in PLAN_FIELDS} == {f: st_idx[f] for f in PLAN_FIELDS}, (st_p, st_idx)
    return s_p, h_p, st_p


# ---- 1. a batch of PSSMs equal to sub[q] is the batch of index queries q -----------------------------------------
def test_pssm_batch_equals_index_batch_on_golden(swg, mctx):
    for name in golden_names():
        g = load_golden(name)
        go, ge = int(g["gaps"][0]), int(g["gaps"][1])
        _options(mctx)
        mctx.set_scoring(g["sub"], go, ge)
        db = swg.Database(g["flat"], g["offsets"]).upload(mctx)
        q = g["query"]
        qs = [q, q[:max(1, len(q) // 2)], q[::-1].copy()]
        s_p, _, _ = _same_as_index_batch(swg, mctx, db, g["sub"], qs, g["offsets"], 10)
        assert np.array_equal(s_p[0], g["oracle32"]), name
        db.close()


@pytest.mark.parametrize("opts,form", [({}, 3), ({"qq": 0}, 2), ({"f16": 0}, 0)], ids=["qq", "f16", "int16"])
def test_pssm_batch_equals_index_batch_config1(swg, orc, mctx, opts, form):
    sc = swg.load_scoring("BLOSUM62")
    tab = sc.table()
    _options(mctx, **opts)
    mctx.set_scoring(sc, -2, -1)
    flat, off = swg.synth_db(0x5EED0001, 1024)                         # config 1's database
    db = swg.Database(flat, off).upload(mctx)
    qs = [swg.synth_query(100 + i, 128) for i in range(64)]
    s_p, h_p, st = _same_as_index_batch(swg, mctx, db, tab, qs, off, 10)
    assert st["engine"] == 2 and st["passes"] == 1 and st["fill_launches"] == 1 and st["path_bits"] == 16, st
    assert st["cell_form"] == form or (form == 3 and st["cell_form"] == 2), st
    for i in (0, 63):
        want = orc.score_db(qs[i], flat, off, tab, -2, -1)
        assert np.array_equal(s_p[i], want) and h_p[i] == orc.topk(want, 10), i
    db.close()
    _options(mctx)


@pytest.mark.parametrize("opts", [{}, {"qq": 0}, {"f16": 0}], ids=["qq", "f16", "int16"])
def test_pssm_batch_odd_counts(swg, orc, mctx, opts):
    """Odd numbers of queries and of sequences, a 1-residue query, a database with a long class."""
    sc = swg.load_scoring("PAM250")
    tab = sc.table()
    mctx.set_scoring(sc, -3, -1)
    for n, max_len, lens in ((1023, 900, (128, 1, 77, 300, 299, 45, 128)), (9001, 5000, (367, 200, 366, 1, 90, 12, 250))):
        flat, off = swg.synth_db(70 + n, n, max_len=max_len)
        _options(mctx, **opts)
        db = swg.Database(flat, off).upload(mctx)
        qs = [swg.synth_query(300 + i, L) for i, L in enumerate(lens)]
        s_p, h_p, _ = _same_as_index_batch(swg, mctx, db, tab, qs, off, 4)
        for i in (0, 1, len(qs) - 1):
            want = orc.score_db(qs[i], flat, off, tab, -3, -1)
            assert np.array_equal(s_p[i], want) and h_p[i] == orc.topk(want, 4), (opts, n, i)
        db.close()
    _options(mctx)


# ---- 2. position-specific columns against the oracle -------------------------------------------------------------
def test_pssm_batch_random_columns_against_oracle(swg, orc, mctx):
    rng = np.random.default_rng(2025)
    _options(mctx)
    mctx.set_scoring(np.zeros((32, 32), dtype=np.int8), -11, -1)       # the table is not read while PSSMs score
    flat, off = swg.synth_db(0x5EED0001, 1024)
    db = swg.Database(flat, off).upload(mctx)
    batch = [_pssm31(rng, int(rng.integers(1, 201)), -12, 12) for _ in range(300)]   # two chunks of at most 256
    got, hits, st = mctx.search_multi_pssm(db, [b[0] for b in batch], k=3)
    assert st["cells"] == sum(len(b[1]) for b in batch) * len(flat)
    for i in (0, 7, 255, 256, 299):
        _, qp, subp = batch[i]
        want = orc.score_db(qp, flat, off, subp, -11, -1)
        assert np.array_equal(got[i], want) and hits[i] == orc.topk(want, 3), (i, len(qp))
    db.close()
    # a larger database with a long tail (bulk and long class side by side), scores past the f16 cells' range
    flat, off = swg.synth_db(31, 20000)
    db = swg.Database(flat, off).upload(mctx)
    batch = [_pssm31(rng, 367, -20, 30) for _ in range(8)]
    got, _, st = mctx.search_multi_pssm(db, [b[0] for b in batch])
    print("8 x 367 positions vs 20 000 sequences:", {f: st[f] for f in PLAN_FIELDS + ("path_bits", "long_pairs")})
    for i in (0, 7):
        _, qp, subp = batch[i]
        assert np.array_equal(got[i], orc.score_db(qp, flat, off, subp, -11, -1)), i
    db.close()


# ---- 3. general PSSMs (every position its own column) against the numpy restatement -----------------------------
@pytest.mark.parametrize("lo,hi", [(-6, 6), (-128, 127)], ids=["f16", "int16"])
def test_pssm_batch_general_columns_against_numpy(swg, mctx, lo, hi):
    rng = np.random.default_rng(hi)
    flat, off = swg.synth_db(0xBEEF, 200, median=50.0, sigma_ln=0.5, min_len=1, max_len=120)
    _options(mctx)
    mctx.set_scoring(np.zeros((32, 32), dtype=np.int8), -10, -1)
    db = swg.Database(flat, off).upload(mctx)
    pssms = [rng.integers(lo, hi + 1, size=(lq, 32)).astype(np.int8) for lq in (1, 17, 64, 40)]
    got, _, st = mctx.search_multi_pssm(db, pssms)
    for i, p in enumerate(pssms):
        assert np.array_equal(got[i], sw_numpy(p, flat, off, -10, -1)), (i, st)
    db.close()


# ---- 4. the batch's top-K selected on the device ---------------------------------------------------------------
def test_pssm_batch_device_topk(swg, orc, mctx):
    rng = np.random.default_rng(4)
    flat, off = swg.synth_db(0x5EED4, 1023, max_len=900)
    _options(mctx)
    mctx.set_scoring(np.zeros((32, 32), dtype=np.int8), -11, -1)
    db = swg.Database(flat, off).upload(mctx)
    pssms = [_pssm31(rng, L, -10, 10)[0] for L in (128, 1, 77, 300, 45)]
    got, _, _ = mctx.search_multi_pssm(db, pssms)
    for k in (1, 4, 300):                  # (k = 300 reaches deep into the 1-position query's ties)
        none, hits, _ = mctx.search_multi_pssm(db, pssms, k=k, want_scores=False)
        assert none is None
        for i in range(len(pssms)):
            assert hits[i] == orc.topk(got[i], k), (k, i)
    db.close()


# ---- 5. the fall-backs (one PSSM after another) are exact -------------------------------------------------------
def test_pssm_batch_fallbacks(swg, orc, mctx):
    rng = np.random.default_rng(5)
    _options(mctx)
    mctx.set_scoring(np.zeros((32, 32), dtype=np.int8), -2, -1)
    flat, off = swg.synth_db(32, 600, max_len=400)
    db = swg.Database(flat, off).upload(mctx)
    # several passes
    batch = [_pssm31(rng, 90, -6, 6)] + [_pssm31(rng, 2500, -6, 6) for _ in range(2)]
    got, hits, st = mctx.search_multi_pssm(db, [b[0] for b in batch], k=5)
    assert st["passes"] > 1, st
    for i, (_, qp, subp) in enumerate(batch):
        want = orc.score_db(qp, flat, off, subp, -2, -1)
        assert np.array_equal(got[i], want) and hits[i] == orc.topk(want, 5), i
    # positive gap scores: the int32 cells
    mctx.set_scoring(np.zeros((32, 32), dtype=np.int8), 1, -2)
    got, _, st = mctx.search_multi_pssm(db, [batch[0][0], batch[0][0][:60]])
    assert st["path_bits"] == 32, st
    assert np.array_equal(got[0], orc.score_db(batch[0][1], flat, off, batch[0][2], 1, -2))
    assert np.array_equal(got[1], orc.score_db(batch[0][1][:60], flat, off, batch[0][2], 1, -2))
    db.close()


def test_pssm_batch_fallback_rescores_past_int16(swg, orc, mctx):
    """Columns boosted to ~10x BLOSUM62 and near-copies of the query planted: with the wide form off the best scores
    pass 32767, the batch runs one PSSM after another and the flagged sequences are re-scored exactly."""
    lq = 800
    rng = np.random.default_rng(lq)
    sub = swg.load_scoring("BLOSUM62").table().astype(np.int64)
    subp = np.clip(sub * 10 + rng.integers(-3, 4, size=(32, 32)), -128, 127).astype(np.int8)
    subp[:, 0] = 0
    q = swg.synth_query(lq, lq)
    flat, off, planted = swg.synth_db(lq, 1500, median=200.0, max_len=1700, query=q, fraction=0.01, subst=0.05)
    assert planted > 0
    _options(mctx, wide16=0)
    mctx.set_scoring(np.zeros((32, 32), dtype=np.int8), -11, -1)
    db = swg.Database(flat, off).upload(mctx)
    q2 = q[100:400].copy()
    got, hits, st = mctx.search_multi_pssm(db, [subp[q.astype(np.int64)], subp[q2.astype(np.int64)]], k=10)
    want = orc.score_db(q, flat, off, subp, -11, -1)
    assert np.array_equal(got[0], want) and hits[0] == orc.topk(want, 10)
    assert np.array_equal(got[1], orc.score_db(q2, flat, off, subp, -11, -1))
    assert want.max() >= 32767 and st["n_rescored"] > 0, (int(want.max()), st)
    db.close()
    _options(mctx)


# ---- 6. the context's own query survives both paths -------------------------------------------------------------
def test_pssm_batch_keeps_the_context_query(swg, orc, mctx):
    rng = np.random.default_rng(6)
    sc = swg.load_scoring("BLOSUM62").table()
    _options(mctx)
    mctx.set_scoring(sc, -2, -1)
    flat, off = swg.synth_db(0x5EED0001, 1024)                         # config 1's database
    db = swg.Database(flat, off).upload(mctx)
    fast = [sc[swg.synth_query(100 + i, 128).astype(np.int64)] for i in range(64)]   # one pass
    slow = [fast[0], _pssm31(rng, 2500, -4, 4)[0]]                      # several passes: one after another
    own_p, own_qp, own_subp = _pssm31(rng, 150, -10, 10)
    own_q = swg.synth_query(66, 120)
    for set_own, want in ((lambda: mctx.set_query_pssm(own_p), orc.score_db(own_qp, flat, off, own_subp, -2, -1)),
                          (lambda: mctx.set_query(own_q), orc.score_db(own_q, flat, off, sc, -2, -1))):
        set_own()
        _, _, st = mctx.search_multi_pssm(db, fast, want_scores=False, k=1)
        assert st["fill_launches"] == 1 and st["passes"] == 1, st
        assert np.array_equal(mctx.search(db)[0], want)
        _, _, st = mctx.search_multi_pssm(db, slow, want_scores=False, k=1)
        assert st["passes"] > 1, st
        assert np.array_equal(mctx.search(db)[0], want)
    db.close()


# ---- 7. errors --------------------------------------------------------------------------------------------------
def test_pssm_batch_errors(swg, mctx):
    import ctypes as C
    _options(mctx)
    mctx.set_scoring(swg.load_scoring("BLOSUM62").table(), -11, -1)
    flat, off = swg.synth_db(9, 64)
    db = swg.Database(flat, off).upload(mctx)
    p = np.ones((8, 32), dtype=np.int8)
    with pytest.raises(swg.SwgError) as e:                              # an empty PSSM: non-increasing offsets
        mctx.search_multi_pssm(db, [p, np.zeros((0, 32), dtype=np.int8)])
    assert e.value.code == swg.SWG_ERR_ARG
    op = np.array([0, 8], dtype=np.uint64)
    assert swg.lib.swg_search_multi_pssm(mctx.handle, db.handle, None, op.ctypes.data_as(C.c_void_p), 1,
                                         None, None, 0, None, None) == swg.SWG_ERR_ARG
    # a search in flight
    mctx.set_query(swg.synth_query(9, 40))
    t = mctx.search_begin(db)
    with pytest.raises(swg.SwgError) as e:
        mctx.search_multi_pssm(db, [p, p])
    assert e.value.code == swg.SWG_ERR_STATE
    mctx.search_end(t)
    got, _, _ = mctx.search_multi_pssm(db, [p, p])                      # (and the context still works)
    assert got.shape == (2, 64)
    db.close()
    # no scoring
    c = swg.Context(0)
    try:
        db = swg.Database(flat, off).upload(c)
        with pytest.raises(swg.SwgError) as e:
            c.search_multi_pssm(db, [p, p])
        assert e.value.code == swg.SWG_ERR_STATE
        db.close()
    finally:
        c.close()


# ---- 8. the rate: a PSSM batch runs at the index batch's speed ---------------------------------------------------
def test_pssm_batch_rate(swg, mctx):
    """64 PSSMs of 128 positions against config 1's database: the same plan and fill kernels as the 64 index queries
    they equal, so at least 0.9x their rate, and at least 8x one PSSM search (which cannot fill the GPU)."""
    sc = swg.load_scoring("BLOSUM62")
    tab = sc.table()
    _options(mctx)
    mctx.set_scoring(sc, -2, -1)
    flat, off = swg.synth_db(0x5EED0001, 1024)
    db = swg.Database(flat, off).upload(mctx)
    qs = [swg.synth_query(100 + i, 128) for i in range(64)]
    pssms = [tab[q.astype(np.int64)] for q in qs]
    mctx.search_multi(db, qs, want_scores=False)                        # warm-up: tokens, code objects
    mctx.search_multi_pssm(db, pssms, want_scores=False)
    best_idx = best_pssm = 0.0
    for _ in range(3):
        _, _, st = mctx.search_multi(db, qs, want_scores=False)
        best_idx = max(best_idx, st["cells"] / (st["fill_ms"] * 1e-3) / 1e9)
        _, _, st = mctx.search_multi_pssm(db, pssms, want_scores=False)
        best_pssm = max(best_pssm, st["cells"] / (st["fill_ms"] * 1e-3) / 1e9)
    mctx.set_query_pssm(pssms[0])
    mctx.search(db, want_scores=False)
    _, _, one = mctx.search(db, want_scores=False)
    single = one["cells"] / (one["fill_ms"] * 1e-3) / 1e9
    print("one PSSM %.1f GCUPS, 64 PSSMs in one pass %.1f GCUPS, 64 index queries in one pass %.1f GCUPS" %
          (single, best_pssm, best_idx))
    assert best_pssm >= 0.9 * best_idx and best_pssm >= 8.0 * single
    db.close()


# ---- 9. the CLI: --allqueries --pssmlist ------------------------------------------------------------------------
def _blocks(out):
    """--allqueries stdout -> {record: its block without the `Query #n` header and the Total Time line}."""
    blocks, cur = {}, None
    for line in out.splitlines():
        m = re.match(r"Query #(\d+): ", line)
        if m:
            cur = int(m.group(1))
            blocks[cur] = []
        elif cur is not None and not line.startswith("Total Time:"):
            blocks[cur].append(line)
    return blocks


def test_cli_pssmlist(swg, orc, mctx, tmp_path):
    sc = swg.load_scoring("BLOSUM62")
    rng = np.random.default_rng(9)
    flat, off = swg.synth_db(0x5EED9, 600)
    seqs = [letters(swg, flat[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)]
    df = tmp_path / "d.fa"
    df.write_text("".join(">s%d\n%s\n" % (i, s) for i, s in enumerate(seqs)))
    # each record's PSSM scores a position by its residue (a 20-column table per record), so it is the index query
    # over a table of its own and the oracle checks it; the table's other columns come from BLOSUM62
    recs, pfs, tabs = [], [], []
    for r, L in enumerate((160, 90, 200)):
        q = swg.synth_query(0x5EED90 + r, L)
        ql = letters(swg, q)
        t20 = rng.integers(-6, 9, size=(32, 20))
        pf = tmp_path / ("r%d.pssm" % r)
        write_ascii_pssm(pf, ql, t20[q.astype(np.int64)])
        pssm, pq = swg.read_pssm(str(pf), sc)
        assert np.array_equal(pq, q)
        subp = np.zeros((32, 32), dtype=np.int8)
        subp[q.astype(np.int64)] = pssm
        assert np.array_equal(subp[q.astype(np.int64)], pssm)
        recs.append((q, ql if r != 1 else ql.lower(), pssm))
        pfs.append(pf)
        tabs.append(subp)
    qf, lf = tmp_path / "q.fa", tmp_path / "list.txt"
    qf.write_text("".join(">rec%d\n%s\n" % (r, ql) for r, (_, ql, _) in enumerate(recs)))
    lf.write_text("".join("%s\n" % p for p in pfs))

    def run(*a):
        r = subprocess.run([CLI, "--substitution_matrix", B62] + [str(x) for x in a], stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        return r.stdout

    blocks = _blocks(run("--allqueries", "--pssmlist", lf, "--files", qf, df))
    assert sorted(blocks) == [0, 1, 2]
    for r, (q, ql, _) in enumerate(recs):
        one = tmp_path / ("one%d.fa" % r)
        one.write_text(">rec%d\n%s\n" % (r, ql))
        alone = [l for l in run("--pssm", pfs[r], "--files", one, df).splitlines()[1:] if not l.startswith("Total Time:")]
        assert blocks[r] == alone, r
        got = [int(l.split()[1]) for l in blocks[r] if l.startswith("score:")]
        assert got == orc.score_db(q, flat, off, tabs[r], -2, -1).tolist(), r
    # --topk 5 --align: every record's alignments are made against its own PSSM
    out = run("--allqueries", "--pssmlist", lf, "--topk", "5", "--align", "--files", qf, df)
    blocks = _blocks(out)
    for r, (q, _, pssm) in enumerate(recs):
        lines = blocks[r]
        n = 0
        for k, l in enumerate(lines):
            m = re.match(r"Alignment #\d+: entry (\d+) score (-?\d+) query (\d+)\.\.(\d+) entry (\d+)\.\.(\d+)$", l)
            if not m:
                continue
            i, s, qb, qe, db_, de = (int(x) for x in m.groups())
            ql_, dl_ = lines[k + 1], lines[k + 2]
            ops = "".join("I" if a == "-" else "D" if b == "-" else "M" for a, b in zip(ql_, dl_))
            a = dict(q_begin=qb, q_end=qe, d_begin=db_, d_end=de, ops=ops)
            assert _path_score(pssm, flat[int(off[i]):int(off[i + 1])], -2, -1, a) == s, (r, l)
            n += 1
        assert n == 5, (r, lines[-20:])
