"""GPU (-m gpu): alignment statistics without the traceback (swg_align_stats, swg_align_stats_multi,
swg_align_stats_multi_pssm, Context.align_stats*, the CLI's --tabular).

Every comparison is on all eleven fields: the seven of align_bounds* (score, index, q_begin, q_end, d_begin, d_end, n_ops),
which must equal align_bounds* on the same context, and the four counts (n_ident, n_match, n_gap_open, n_gap).  The truth
for an index query is the int32 oracle's traceback (orc.pair_trace) with the counts taken from its ops string --
n_gap_open is the number of matches of I+|D+ --; for a PSSM it is the ops string align_hits_multi_pssm returns on the same
context, identity counted against the PSSM's consensus (the lowest residue index in 1..31 whose score is the row's maximum
over 1..31)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "seq-align-gpu_amd", "bin", "smith_waterman")
B62 = os.path.join(ROOT, "seq-align-gpu_amd", "data", "BLOSUM62.txt")
GEOMETRIES = [(16, 4), (16, 8), (32, 8), (64, 8), (64, 16)]   # (G, K) of swg_stats_kernel's instantiations (swg_bounds.hip)
LIMIT = 1024                                                  # the column limit: 64 lanes x 16 columns, stats included
BOUNDS = ("score", "index", "q_begin", "q_end", "d_begin", "d_end", "n_ops")
COUNTS = ("n_ident", "n_match", "n_gap_open", "n_gap")
FIELDS = BOUNDS + COUNTS
GAPS3 = [(-11, -1), (0, 0), (2, 1)]
FEW = np.array([1, 3, 4, 5], dtype=np.int8)                   # a four-letter alphabet: short random pairs tie often


@pytest.fixture(scope="module")
def sctx(swg):
    c = swg.Context(0)
    c.set_option("autotune", 0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def b62(swg):
    return swg.load_scoring("BLOSUM62").table()


def _pack(seqs):
    flat = np.concatenate(seqs).astype(np.int8)
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
    return flat, off


def _every(off):
    return [(0, i) for i in range(len(off) - 1)]


def counts_of(q, d, q_begin, d_begin, ops):
    """(n_ident, n_match, n_gap_open, n_gap) of a spelled path; q = the query's residues (a PSSM's consensus)."""
    qi, di, ident = q_begin, d_begin, 0
    for o in ops:
        if o == "M":
            ident += int(q[qi] == d[di])
            qi, di = qi + 1, di + 1
        elif o == "I":
            di += 1
        else:
            qi += 1
    return ident, ops.count("M"), len(re.findall("I+|D+", ops)), len(ops) - ops.count("M")


def consensus(pssm):
    return (np.argmax(np.asarray(pssm)[:, 1:32], axis=1) + 1).astype(np.int8)     # (argmax: the first = lowest index)


def _oracle(orc, queries, flat, off, sub, go, ge, rows):
    """Every row of `rows` against the oracle's traceback -> the oracle's ops strings, in order."""
    all_ops = []
    for q, row in zip(queries, rows):
        for a in row:
            d = flat[int(off[a["index"]]):int(off[a["index"] + 1])]
            sc, co, ops = orc.pair_trace(q, d, sub, go, ge)
            want = (sc, a["index"], co[0], co[1], co[2], co[3], len(ops)) + counts_of(q, d, co[0], co[2], ops)
            assert tuple(a[f] for f in FIELDS) == want, (len(q), a, want, ops)
            all_ops.append(ops)
    return all_ops


def _strip(rows):
    return [[{f: a[f] for f in BOUNDS} for a in row] for row in rows]


def _batch(sctx, db, queries, hits):
    got = sctx.align_stats_multi(db, queries, hits)
    last = sctx.debug_bounds_last()
    assert all(tuple(a) == FIELDS for row in got for a in row)
    assert _strip(got) == sctx.align_bounds_multi(db, queries, hits)
    return got, last


# ---- 1. lane and column edges of every instantiation ------------------------------------------------------------------
@pytest.mark.parametrize("G,K", GEOMETRIES)
@pytest.mark.parametrize("gaps", [(-2, -1), (-3, 1), (2, 1)])
def test_stats_lane_and_column_edges(swg, orc, sctx, b62, G, K, gaps):
    """The queries and sequences of test_bounds_lane_and_column_edges.  With a positive gap_extend paths run in from the
    matrix border (checked with the oracle below): the border hand-overs' opening is counted."""
    rng = np.random.default_rng(G * 100 + K)
    base = FEW[rng.integers(0, 4, size=LIMIT + 1)]
    lqs = sorted({1, 2, K - 1, K, K + 1, G * K - 1, G * K, G * K + 1, LIMIT, LIMIT + 1})
    lens = sorted({1, 2, G - 1, G, G + 1, 3 * G + 5})
    queries = []
    for lq in lqs:
        q = base[:lq].copy()
        m = rng.random(lq) < 0.08
        q[m] = FEW[rng.integers(0, 4, size=int(m.sum()))]
        queries.append(q)
    seqs = []
    for L in lens:
        for start in (0, max(0, G * K - L // 2 - 1)):             # the query's first columns, and across its last lane
            s = base[start:start + L].copy()
            if L > 8:
                s = np.delete(s, L // 2)                           # an indel: gapped paths
                s = np.append(s, FEW[rng.integers(0, 4)])
            seqs.append(s)
    flat, off = _pack(seqs)
    sctx.set_scoring(b62, *gaps)
    db = swg.Database(flat, off).upload(sctx)
    hits = [_every(off) for _ in queries]
    got, last = _batch(sctx, db, queries, hits)
    within = sum(len(off) - 1 for lq in lqs if lq <= LIMIT)
    assert (last["kernel_pairs"], last["fallback_pairs"]) == (within, len(off) - 1), last   # the last query: the fallback
    ops = _oracle(orc, queries, flat, off, b62, gaps[0], gaps[1], got)
    assert len(ops) == len(lqs) * len(seqs)
    flat_got = [a for row in got for a in row]
    assert any(a["n_gap_open"] >= 2 for a in flat_got) and any(a["n_ident"] < a["n_match"] for a in flat_got)
    if gaps[1] > 0:                                              # a path that runs in from the border, beginning with a gap
        assert any(o[:1] in ("I", "D") and (a["q_begin"] == 0 or a["d_begin"] == 0) for o, a in zip(ops, flat_got))
    db.close()


# ---- 2. ties ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gaps", GAPS3)
def test_stats_ties(swg, orc, sctx, b62, gaps):
    """The set of test_bounds_ties: one letter throughout, and a period-3 repeat against its own repeats."""
    a40 = np.full(40, 1, dtype=np.int8)
    rep = np.tile(np.array([1, 3, 4], dtype=np.int8), 14)[:40]
    seqs = [np.full(L, 1, dtype=np.int8) for L in (1, 39, 40, 41, 90)]
    seqs += [np.tile(np.array([1, 3, 4], dtype=np.int8), 31)[s:s + L] for s, L in ((0, 3), (1, 39), (0, 40), (2, 41), (0, 90))]
    flat, off = _pack(seqs)
    sctx.set_scoring(b62, *gaps)
    db = swg.Database(flat, off).upload(sctx)
    queries = [a40, rep]
    got, last = _batch(sctx, db, queries, [_every(off), _every(off)])
    assert last["fallback_pairs"] == 0
    _oracle(orc, queries, flat, off, b62, gaps[0], gaps[1], got)
    db.close()


# ---- 3. several pairs through one lane group ----------------------------------------------------------------------------
@pytest.mark.parametrize("groups", [1, 2])
def test_stats_pairs_one_after_another_in_a_group(swg, orc, sctx, b62, groups):
    """The 9 pairs of test_bounds_pairs_one_after_another_in_a_group: longest first, a group sees two copies of the query
    (100 identical columns) directly followed by 180 x 'W' (score 0), and at the end a one-residue pair and a one-residue
    score-0 pair.  No count of one job may reach the next."""
    q = swg.synth_query(0xB0D, 100)
    q[np.isin(q, (6, 23, 25))] = 1                         # no F, W, Y in the query:
    rng = np.random.default_rng(0xB0D)
    w = np.array([23], dtype=np.int8)                      # then 'W' scores below 0 against every column
    assert (b62[23, q.astype(np.int64)] < 0).all()
    seqs = [np.concatenate([q, q]), np.array([q[50]], dtype=np.int8), np.tile(w, 180), q[10:70].copy(), np.tile(w, 1),
            swg.synth_query(77, 150), q[::-1].copy(), np.concatenate([q[:40], q[45:]]), swg.synth_query(78, 120)]
    order = rng.permutation(len(seqs))
    seqs = [seqs[i] for i in order]
    flat, off = _pack(seqs)
    sctx.set_scoring(b62, -11, -1)
    sctx.set_query(q)
    db = swg.Database(flat, off).upload(sctx)
    sctx.set_option("bounds_groups", groups)
    try:
        got = sctx.align_stats(db, _every(off))
        last = sctx.debug_bounds_last()
        assert _strip([got])[0] == sctx.align_bounds(db, _every(off))
    finally:
        sctx.set_option("bounds_groups", 0)
    assert (last["kernel_pairs"], last["fallback_pairs"], last["launches"]) == (9, 0, 1)
    _oracle(orc, [q], flat, off, b62, -11, -1, [got])
    zero = [a for a in got if a["score"] == 0]
    assert len(zero) == 2 and all(tuple(a[f] for f in FIELDS if f != "index") == (0,) * 10 for a in zero)
    assert max(a["n_ident"] for a in got) == 100 and any(a["n_gap_open"] == 1 for a in got)
    one = [a for a in got if a["score"] > 0 and int(off[a["index"] + 1] - off[a["index"]]) == 1]
    assert one and all((a["n_ident"], a["n_match"], a["n_gap_open"], a["n_gap"]) == (1, 1, 0, 0) for a in one)
    db.close()


# ---- 4. field widths ---------------------------------------------------------------------------------------------------
def test_stats_widest_identity(swg, orc, sctx, b62):
    """A 1024-column query against a sequence that contains it: the identity count's largest value."""
    q = swg.synth_query(0x57A7, LIMIT)
    seqs = [np.concatenate([swg.synth_query(1, 50), q, swg.synth_query(2, 50)]), q[:700].copy()]
    flat, off = _pack(seqs)
    sctx.set_scoring(b62, -11, -1)
    db = swg.Database(flat, off).upload(sctx)
    got, last = _batch(sctx, db, [q], [_every(off)])
    assert (last["kernel_pairs"], last["fallback_pairs"]) == (2, 0)
    _oracle(orc, [q], flat, off, b62, -11, -1, got)
    assert (got[0][0]["n_ident"], got[0][0]["n_match"], got[0][0]["n_gap_open"]) == (LIMIT, LIMIT, 0)
    assert got[0][1]["n_ident"] == 700
    db.close()


def test_stats_widest_gap_openings(swg, orc, sctx):
    """Query and sequence 1024 x residue 1, every substitution score -100, gaps (2, 1): an opened gap step pays 3 and an
    extended one 1, so the path alternates I and D and ends in its one M: 2045 openings, the opening count's largest
    value but four (2 * 1024 + 1 is the bound the tag's field is sized for)."""
    sub = np.full((32, 32), -100, dtype=np.int8)
    q = np.ones(LIMIT, dtype=np.int8)
    flat, off = _pack([q.copy()])
    sctx.set_scoring(sub, 2, 1)
    db = swg.Database(flat, off).upload(sctx)
    got, last = _batch(sctx, db, [q], [[(0, 0)]])
    assert (last["kernel_pairs"], last["fallback_pairs"]) == (1, 0)
    _oracle(orc, [q], flat, off, sub, 2, 1, got)
    a = got[0][0]
    assert (a["score"], a["n_ops"], a["n_gap_open"], a["n_gap"], a["n_match"], a["n_ident"]) == (6035, 2046, 2045, 2045, 1, 1)
    db.close()


# ---- 5. PSSMs --------------------------------------------------------------------------------------------------------
def _pssm_truth(sctx, db, flat, off, pssms, hits, got):
    walked = sctx.align_hits_multi_pssm(db, pssms, hits)
    for p, row_w, row_g in zip(pssms, walked, got):
        cons = consensus(p)
        for w, g in zip(row_w, row_g):
            d = flat[int(off[w["index"]]):int(off[w["index"] + 1])]
            want = tuple(w[f] for f in BOUNDS) + counts_of(cons, d, w["q_begin"], w["d_begin"], w["ops"])
            assert tuple(g[f] for f in FIELDS) == want, (len(p), g, want)


def test_stats_pssm(swg, orc, sctx, b62):
    rng = np.random.default_rng(0x57A8)
    flat, off = swg.synth_db(0xB0F, 300, max_len=700)
    qs = [swg.synth_query(0xB10 + i, L) for i, L in enumerate((128, 60, 1, 700, 1100))]
    sctx.set_scoring(b62, -2, -1)
    db = swg.Database(flat, off).upload(sctx)
    _, hits, _ = sctx.search_multi(db, qs, k=6, want_scores=False)
    got_idx, _ = _batch(sctx, db, qs, hits)
    # a PSSM equal to the table's rows: BLOSUM62's diagonal is each row's strict maximum, so the consensus is the query
    pssms = [b62[q.astype(np.int64)] for q in qs]
    assert all(np.array_equal(consensus(p), q) for p, q in zip(pssms, qs))
    got = sctx.align_stats_multi_pssm(db, pssms, hits)
    last = sctx.debug_bounds_last()
    assert got == got_idx
    assert (last["kernel_pairs"], last["fallback_pairs"]) == (24, 6), last
    assert _strip(got) == sctx.align_bounds_multi_pssm(db, pssms, hits)
    # random PSSMs; one of them with tied maxima, where the lowest index must win
    rnd = [rng.integers(-128, 128, size=(L, 32)).astype(np.int8) for L in (5, 64, 65, 300, 1030)]
    rnd[1][:, 1:32] = np.minimum(rnd[1][:, 1:32], 40)
    rnd[1][np.arange(64), rng.integers(1, 20, size=64)] = 40                   # every row's maximum over 1..31 is 40,
    rnd[1][:, 20] = 40                                                        # reached at least twice
    assert all((row[1:32] == row[1:32].max()).sum() >= 2 for row in rnd[1]) and (consensus(rnd[1]) < 20).all()
    _, rhits, _ = sctx.search_multi_pssm(db, rnd, k=5, want_scores=False)
    got = sctx.align_stats_multi_pssm(db, rnd, rhits)
    last = sctx.debug_bounds_last()
    assert (last["kernel_pairs"], last["fallback_pairs"]) == (20, 5), last
    assert _strip(got) == sctx.align_bounds_multi_pssm(db, rnd, rhits)
    _pssm_truth(sctx, db, flat, off, rnd, rhits, got)
    assert any(a["n_ident"] > 0 for a in got[1])                               # the tied rows' consensus is matched
    for p, row, want in zip(rnd, rhits, got):                                  # the single call on the context's PSSM
        sctx.set_query_pssm(p)
        assert sctx.align_stats(db, row) == want
    db.close()


# ---- 6. views ----------------------------------------------------------------------------------------------------------
def test_stats_through_a_view(swg, orc, sctx, b62):
    flat, off = swg.synth_db(0xB11, 400, max_len=300)
    q = swg.synth_query(0xB11, 90)
    sctx.set_scoring(b62, -11, -1)
    sctx.set_query(q)
    db = swg.Database(flat, off).upload(sctx)
    half = list(range(1, 400, 2))
    view = db.view(sctx, half)
    _, hits, _ = sctx.search(view, k=8)
    assert all(i % 2 == 1 for _, i in hits)
    got = sctx.align_stats(view, hits)
    assert sctx.debug_bounds_last()["kernel_pairs"] == 8
    assert got == sctx.align_stats(db, hits) and _strip([got])[0] == sctx.align_bounds(view, hits)
    _oracle(orc, [q], flat, off, b62, -11, -1, [got])
    assert sctx.align_stats_multi(view, [q, q[:30]], [hits, hits[:2]]) == sctx.align_stats_multi(db, [q, q[:30]], [hits, hits[:2]])
    with pytest.raises(swg.SwgError) as e:
        sctx.align_stats(view, [(0, 2)])                       # in the database, outside the view
    assert e.value.code == swg.SWG_ERR_ARG
    with pytest.raises(swg.SwgError) as e:
        sctx.align_stats_multi(view, [q], [[hits[0], (0, 400)]])
    assert e.value.code == swg.SWG_ERR_ARG
    view.close()
    db.close()


# ---- 7. the context's query, and errors ----------------------------------------------------------------------------------
def test_stats_batch_leaves_the_context_query(swg, sctx, b62):
    rng = np.random.default_rng(0xB12)
    flat, off = swg.synth_db(0xB12, 200, max_len=200)
    own = swg.synth_query(0xB12, 77)
    others = [swg.synth_query(0xB13, 50), swg.synth_query(0xB14, 200)]
    pss = [rng.integers(-5, 9, size=(40, 32)).astype(np.int8)]
    sctx.set_scoring(b62, -2, -1)
    db = swg.Database(flat, off).upload(sctx)
    for setter, mine in ((sctx.set_query, own), (sctx.set_query_pssm, b62[own.astype(np.int64)] + 1)):
        setter(mine)
        before, hits, _ = sctx.search(db, k=4)
        single = sctx.align_stats(db, hits)
        sctx.align_stats_multi(db, others, [hits, hits])
        sctx.align_stats_multi_pssm(db, pss, [hits])
        after, hits2, _ = sctx.search(db, k=4)
        assert np.array_equal(before, after) and hits2 == hits
        assert sctx.align_stats(db, hits) == single and _strip([single])[0] == sctx.align_bounds(db, hits)
    db.close()


def test_stats_argument_errors(swg, sctx, b62):
    flat, off = swg.synth_db(0xB15, 50, max_len=100)
    q = swg.synth_query(0xB15, 30)
    sctx.set_scoring(b62, -2, -1)
    sctx.set_query(q)
    db = swg.Database(flat, off).upload(sctx)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)                                    # noqa: E731
    qoff = np.array([0, 30], dtype=np.uint64)
    k = 4
    arr = (swg.Hit * k)()
    out = np.full((k, 8), 0xA5A5A5A5, dtype=np.uint32)
    cnt = np.full((k, 4), 0xA5A5A5A5, dtype=np.uint32)
    call = lambda off_, k_, nh, o=out, c=cnt, d=db: swg.lib.swg_align_stats_multi(   # noqa: E731
        sctx.handle, d.handle, vp(q), vp(off_), len(off_) - 1, C.cast(arr, C.c_void_p), k_, C.cast(nh, C.c_void_p),
        vp(o) if o is not None else None, vp(c) if c is not None else None)
    assert call(qoff, k, (C.c_size_t * 1)(2)) == swg.SWG_OK
    want = sctx.align_stats_multi(db, [q], [[(0, 0), (0, 0)]])[0]
    for j in range(k):                                                            # slots past n_hits[0] are not written
        if j < 2:
            assert [int(v) for v in out[j][:7]] == [want[j][f] for f in BOUNDS] and out[j][7] == 0
            assert [int(v) for v in cnt[j]] == [want[j][f] for f in COUNTS]
        else:
            assert (out[j] == 0xA5A5A5A5).all() and (cnt[j] == 0xA5A5A5A5).all()
    assert call(qoff, 1, (C.c_size_t * 1)(2)) == swg.SWG_ERR_ARG                    # k < n_hits[0]
    assert call(np.array([0, 30, 30], dtype=np.uint64), 2, (C.c_size_t * 2)(1, 1)) == swg.SWG_ERR_ARG   # offsets not increasing
    assert call(qoff, k, (C.c_size_t * 1)(2), o=None) == swg.SWG_ERR_ARG            # NULL out
    assert call(qoff, k, (C.c_size_t * 1)(2), c=None) == swg.SWG_ERR_ARG            # NULL counts
    assert "swg_align_stats_multi" in swg.lib.swg_last_error(sctx.handle).decode()
    assert swg.lib.swg_align_stats(sctx.handle, db.handle, C.cast(arr, C.c_void_p), 2, vp(out), None) == swg.SWG_ERR_ARG
    assert swg.lib.swg_align_stats(sctx.handle, db.handle, C.cast(arr, C.c_void_p), 2, None, vp(cnt)) == swg.SWG_ERR_ARG
    assert sctx.align_stats(db, []) == [] and sctx.align_stats_multi(db, [q], [[]]) == [[]]
    with pytest.raises(swg.SwgError) as e:
        sctx.align_stats(db, [(0, 50)])                                            # no such sequence
    assert e.value.code == swg.SWG_ERR_ARG
    host_only = swg.Database(flat, off)                                            # packed, not uploaded
    assert call(qoff, k, (C.c_size_t * 1)(2), d=host_only) == swg.SWG_ERR_STATE
    with pytest.raises(swg.SwgError) as e:
        sctx.align_stats(host_only, [(0, 1)])
    assert e.value.code == swg.SWG_ERR_STATE
    host_only.close()
    db.close()


# ---- 8. the tool --------------------------------------------------------------------------------------------------------
def _letters(idx):
    return "".join(chr(int(v) + 64) for v in idx)


def _cli(*a):
    r = subprocess.run([CLI, "--substitution_matrix", B62, "--gapopen", "-11", "--gapextend", "-1"] + [str(x) for x in a],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return r.stdout


def _blocks(out):
    """-> the output per `Query #n` block (one block without --allqueries)."""
    parts = re.split(r"(?m)^Query #\d+: .*$", out)
    return parts[1:] if len(parts) > 1 else [out]


HEADER = "# Fields: query, entry, pident, length, mismatch, gapopen, qstart, qend, sstart, send, score"


def test_stats_tool(swg, sctx, b62, tmp_path):
    base = swg.synth_query(0xB16, 120)
    flat, off, _ = swg.synth_db(0xB16, 40, query=base, fraction=0.4, subst=0.1, max_len=250)
    qs = [base, base[20:90].copy(), swg.synth_query(0xB17, 45)]
    qf, df = tmp_path / "q.fa", tmp_path / "d.fa"
    qf.write_text("".join(">q%d\n%s\n" % (i, _letters(q)) for i, q in enumerate(qs)))
    df.write_text("".join(">d%d\n%s\n" % (i, _letters(flat[int(off[i]):int(off[i + 1])])) for i in range(len(off) - 1)))
    sctx.set_scoring(b62, -11, -1)
    db = swg.Database(flat, off).upload(sctx)

    def lines(rows):
        return [["q%d\td%d\t%.2f\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d" %
                 (i, a["index"], 100.0 * a["n_ident"] / a["n_ops"], a["n_ops"], a["n_match"] - a["n_ident"], a["n_gap_open"],
                  a["q_begin"] + 1, a["q_end"], a["d_begin"] + 1, a["d_end"], a["score"]) for a in row if a["score"] > 0]
                for i, row in enumerate(rows)]

    def tabular_of(out):
        got = []
        for b in _blocks(out):
            ls = b.splitlines()
            assert ls.count(HEADER) == 1
            at = ls.index(HEADER)
            assert any(l.startswith("Top ") for l in ls[:at])              # after the Top-K report
            got.append([l for l in ls[at + 1:] if l.count("\t") == 10])
        return got

    # one query
    sctx.set_query(qs[0])
    _, hits, _ = sctx.search(db, k=5)
    one = _cli("--topk", 5, "--tabular", "--files", qf, df)
    want = lines([sctx.align_stats(db, hits)])
    assert tabular_of(one) == want and len(want[0]) == 5
    assert "Alignment #" not in one and "Bounds #" not in one
    # every record
    _, mh, _ = sctx.search_multi(db, qs, k=3, want_scores=False)
    want = lines(sctx.align_stats_multi(db, qs, mh))
    allq = _cli("--allqueries", "--topk", 3, "--tabular", "--files", qf, df)
    assert tabular_of(allq) == want and all(len(w) == 3 for w in want)
    assert any(float(l.split("\t")[2]) < 100.0 for w in want for l in w) and any(int(l.split("\t")[5]) > 0 for w in want for l in w)
    # behind the prefilter (40 entries, 20 candidates per record)
    pre = _cli("--allqueries", "--prefilter", 20, "--topk", 3, "--tabular", "--files", qf, df)
    tops = [[l.split("\t") for l in re.search(r"(?m)^Top \d+ hits.*\n((?:-?\d+\t.*\n)*)", b).group(1).splitlines()] for b in _blocks(pre)]
    ph = [[(int(t[0]), int(t[1])) for t in row] for row in tops]
    assert tabular_of(pre) == lines(sctx.align_stats_multi(db, qs, ph)) and all(len(r) == 3 for r in ph)
    db.close()
