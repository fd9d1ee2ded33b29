"""GPU (-m gpu): the scoring-parameter edges -- gap magnitudes at every hand-over between cell forms (2048 / 2049:
f16 -> int16, 32767 / 32768: 16-bit -> int32, 65536 in the int32 kernels and the trace kernel) and table entries
over the whole of int8, garbage in row / column 0 included -- on every route the geometry tests already run.
Everything against the int32 oracle, bit for bit, per sequence; the databases come from tests/scoring_edges.py,
built so that a large gap magnitude is OBSERVABLE (some best alignment goes through a gap), which every test asserts
first from the oracle alone.  The route (swg_stats.path_bits, cell_form) is part of each expectation."""
import numpy as np
import pytest

import scoring_edges as se
from test_gpu_align import _check
from test_gpu_parity import _f16_part
from test_gpu_pssm import PLAN_FIELDS

pytestmark = pytest.mark.gpu

OPTIONS = ("force_bits", "engine", "cols_per_wave", "max_waves", "group_lanes", "long_split", "workgroups",
           "segment_blocks", "f16_pair")
DEFAULT_ON = ("work_queue", "wide16", "f16", "qq", "last_pass")

@pytest.fixture(scope="module")
def ectx(swg):
    c = swg.Context(0)
    yield c
    c.close()


def _reset_options(c):
    c.set_option("batch", 8)
    c.set_option("batch_blocks", 0)
    for k in OPTIONS:
        c.set_option(k, 0)
    for k in DEFAULT_ON:
        c.set_option(k, 1)
    c.set_option("long_helps", 0)


def _geometry(lq):
    """A forced lane-group geometry of several passes for this query length, from those
    test_diagonal_geometry_does_not_change_scores / test_q32_geometry_does_not_change_scores run.  The narrowest
    geometry there is, 2 columns x 16 lanes, covers 32 columns: a 40-column query (the g = 2047 .. 2049 points' own
    flanks of 20) takes 2 passes, never 3.  Those points reach 5 passes on their second database (flanks of 262);
    test_gap_points_on_every_route asserts that every 16-bit point ran 3 passes or more on one of its databases."""
    if lq <= 96:
        return {"cols_per_wave": 2, "group_lanes": 16, "max_waves": 4}
    if lq <= 400:
        return {"cols_per_wave": 6, "group_lanes": 16, "max_waves": 4}
    if lq <= 700:
        return {"cols_per_wave": 8, "group_lanes": 16, "max_waves": 4}
    return {"cols_per_wave": 8, "group_lanes": 32, "max_waves": 8}


def _option_sets(lq, max_len, long_split):
    geo = _geometry(lq)
    seg = (int(max_len) + 5) // 4 * 2 + 1
    return [
        ("default", {}),
        ("engine1", {"engine": 1}),
        ("engine2_f16_0", {"engine": 2, "f16": 0}),
        ("engine2_f16_2", {"engine": 2, "f16": 2}),
        ("f16_2_pair1", {"f16": 2, "f16_pair": 1}),
        ("f16_2_pair2", {"f16": 2, "f16_pair": 2}),
        ("wide16_0", {"wide16": 0}),
        ("wide16_1", {"engine": 2, "wide16": 1}),
        ("work_queue_0", {"work_queue": 0}),
        ("int32", {"force_bits": 32}),
        ("int32_geometry", dict(geo, engine=2, force_bits=32)),
        ("passes", dict(geo, engine=2)),
        ("passes_f16_2", dict(geo, engine=2, f16=2)),
        ("passes_segments", dict(geo, engine=2, segment_blocks=seg)),
        ("passes_segments_f16_2", dict(geo, engine=2, f16=2, segment_blocks=seg)),
        ("long_split", {"engine": 2, "long_split": long_split}),
        ("last_pass_0", dict(geo, engine=2, last_pass=0)),
    ]


def _score_bound(sub, q, lens):
    """The library's bound on any score of a search (swg_api.cpp: the query's best total over residues 1 .. 31, and
    the longest sequence -- in whole token blocks of 4 rows -- times the largest table entry)."""
    sub = np.asarray(sub).astype(np.int64)
    qbound = int(sub[q.astype(np.int64)][:, 1:].max(axis=1).clip(min=0).sum())
    return min(qbound, min(len(q), (int(lens.max()) + 3) // 4 * 4) * max(0, int(sub.max())))


def _search_and_check(swg, orc, c, sub, q, flat, off, want, go, ge, bits, f16_ok, name, opts, seen, k=10):
    """One search under `opts`: scores, hits, route and n_rescored."""
    _reset_options(c)
    for key, v in opts.items():
        c.set_option(key, v)
    db = swg.Database(flat, off).upload(c)
    got, hits, st = c.search(db, k=k)
    db.close()
    form = st["cell_form"]
    seen.add((st["path_bits"], form, st["engine"]))
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (name, opts, st, bad[:8], got[bad[:8]], want[bad[:8]])
    assert hits == orc.topk(want, k), (name, opts, st)
    want_bits = 32 if bits == 32 or opts.get("force_bits") == 32 else 16
    assert st["path_bits"] == want_bits, (name, opts, st)
    lens = np.diff(off.astype(np.int64))
    if "engine" in opts:
        assert st["engine"] == opts["engine"], (name, opts, st)
    if "cols_per_wave" in opts and want_bits == 16:
        assert (st["cols_per_wave"], st["group_lanes"]) == (opts["cols_per_wave"], opts["group_lanes"]), (name, st)
        assert st["passes"] == -(-len(q) // (opts["cols_per_wave"] * opts["group_lanes"])), (name, st)
    if "long_split" in opts and want_bits == 16:
        # (as test_random_database_matches_oracle counts them: pairs of the length-sorted order whose longer member
        # is beyond the cut, a class of their own unless they are more than a quarter of all pairs)
        n_long = int((np.sort(lens)[::-1][::2] + 2 > max(opts["long_split"], 64)).sum())
        assert 0 < n_long * 4 <= (len(lens) + 1) // 2 and st["long_pairs"] == n_long, (name, opts, n_long, st)
    if want_bits == 32:
        assert st["n_rescored"] == 0, (name, opts, st)
        return st
    if not f16_ok or opts.get("f16") == 0:
        assert form in (0, 1), (name, opts, st)          # above 2048 the f16 cells must not run, even when asked for
    elif st["engine"] == 1:
        # the systolic engine has no flag-and-re-run route: the f16 cells exactly where no score can reach their ceiling
        # (and the query takes one pass: its f16 rows have no form with edges)
        assert form == (2 if _score_bound(sub, q, lens) < 4096 and st["passes"] == 1 else 0), (name, opts, st)
    elif opts.get("work_queue") == 0:
        assert form in (0, 1), (name, opts, st)          # (the f16 cells exist in the work-queue kernels only)
    elif opts.get("f16") == 2:
        assert form == 2, (name, opts, st)
    if st["engine"] == 1:
        assert st["n_rescored"] == (0 if form == 2 else int((want >= 32767).sum())), (name, opts, st)
    elif form == 2:
        assert st["n_rescored"] == int((want >= 4096).sum()), (name, opts, st)
    elif form == 0:
        assert st["n_rescored"] == int((want >= 32767).sum()), (name, opts, st)
    elif form == 1:
        assert st["n_rescored"] == int((want >= 65535).sum()), (name, opts, st)
    else:
        assert form in (4, 5) and st["split_rows"] > 0, (name, opts, st)
        part = _f16_part(lens, st["split_rows"])
        assert st["n_rescored"] == int((want[part] >= 4096).sum()) + int((want >= (65535 if form == 4 else 32767)).sum()), (name, opts, st)
    return st


def _point_db(orc, p, n, salt, long_decoys=0):
    sub = se.diag127()
    rng = np.random.default_rng([p["g"], p["e"], salt])
    q, flat, off, kinds = se.split_db(p["g"], n, rng, long_decoys=long_decoys)
    n_gap, n_i, n_d = se.gapped_relatives(orc, q, flat, off, kinds, sub, p["go"], p["ge"])
    # the self-check: without it the module would pass on data where the gap magnitude is invisible
    assert n_gap >= 5 and n_i >= 1 and n_d >= 1, (p, n_gap, n_i, n_d)
    return sub, q, flat, off, kinds


# ---- 1. gap points x routes, search -----------------------------------------------------------------------------
@pytest.mark.parametrize("p", se.GAP_POINTS, ids=se.point_id)
def test_gap_points_on_every_route(swg, orc, ectx, p):
    """Every gap point on its split_db (about 3000 sequences: several workgroups, queue shards, both pair classes)
    under every option set: scores and top-K equal the oracle's, the route is the documented one, and n_rescored is
    the count of oracle scores at or above the ceiling of the cells that ran (4096 f16, 32767 int16, 65535 wide).
    With diag127 a copy of the query scores 254 F and a relative with one indel about 254 F - g: at g = 2047 / 2048
    either side of the f16 ceiling, at g = 32767 beyond the wide form and inside it; g = 32767 on the PLAIN int16
    cells (wide16 = 0, engine 1) is a saturation test only -- no gap can pay below 32767 there, the gapped relatives
    are flagged and re-scored in int32.  A 16-bit point whose own flanks keep every score below 32767 runs a second
    database with flanks of 262, so that the wide form meets its gap magnitude too.  The forms and engines that ran are
    printed per point, and every form the point is entitled to must be among them."""
    go, ge = p["go"], p["ge"]
    seen, most_passes = set(), {}
    dbs = [_point_db(orc, p, se.SEARCH_DB_SIZE, 1, long_decoys=24)]
    if p["bits"] == 16 and se.flank_len(p["g"]) < 262:
        # the point's own flanks keep every score below 32767, where the library has no use for the wide form: the same
        # relatives of a query with flanks of 262 (a copy 66548: beyond the wide form; one indel 66548 - g: inside it)
        rng = np.random.default_rng([p["g"], p["e"], 2])
        wq = rng.integers(1, 32, size=524).astype(np.int8)
        dbs.append((dbs[0][0],) + se.split_db(p["g"], 1001, rng, query=wq, long_decoys=24))
        assert se.gapped_relatives(orc, *dbs[1][1:], dbs[1][0], go, ge)[0] >= 5
    ectx.set_scoring(dbs[0][0], go, ge)
    for sub, q, flat, off, kinds in dbs:
        want = orc.score_db(q, flat, off, sub, go, ge)
        F = len(q) // 2
        assert want.max() == 254 * F
        ectx.set_query(q)
        lens = np.diff(off.astype(np.int64))
        for name, opts in _option_sets(len(q), lens.max(), max(64, 3 * F + 3)):
            st = _search_and_check(swg, orc, ectx, sub, q, flat, off, want, go, ge, p["bits"], p["f16"], (F, name), opts, seen)
            if name.startswith("passes") or name == "last_pass_0":
                most_passes[name] = max(most_passes.get(name, 0), st["passes"])
    forms = sorted(seen)
    print("gap point %s: g %d e %d flanks %s; (path_bits, cell_form, engine) observed: %s" % (
        se.point_id(p), p["g"], p["e"], [len(d[1]) // 2 for d in dbs], forms))
    if p["bits"] == 32:
        assert {b for b, _, _ in seen} == {32}
    else:
        got_forms = {f for b, f, _ in seen if b == 16}
        assert (2 in got_forms) == p["f16"] and {0, 1} <= got_forms, forms    # every form the point is entitled to
        assert 32 in {b for b, _, _ in seen} and {1, 2} <= {e for _, _, e in seen}
        # 3 passes or more, with and without segments, on the int16 and the f16 (or int16 again) cells, last_pass off
        assert len(most_passes) == 5 and min(most_passes.values()) >= 3, most_passes
    _reset_options(ectx)


# ---- 2. tables x routes, search ---------------------------------------------------------------------------------
@pytest.mark.parametrize("gaps", [(-2, -1), (-11, -1)], ids=["gap2_1", "gap11_1"])
@pytest.mark.parametrize("tname", ["full_range", "all_127", "all_m128", "blosum62_dirty0"])
def test_tables_on_every_route(swg, orc, ectx, tname, gaps):
    """Table entries over the whole of int8, rows and columns 0 included (index 0 is no residue: the kernels pad with
    it, so whatever the table holds there must never reach a score): short sequences (1 .. 60; lq 17, 64) and long
    ones (to 1200; lq 300, 1100), same option sets.  all_127 has the closed form 127 min(lq, len), all_m128 scores 0
    everywhere (top-K = the first K indices), blosum62_dirty0 must score as plain BLOSUM62."""
    b62 = swg.load_scoring("BLOSUM62").table()
    sub = se.table(tname, b62)
    go, ge = gaps
    rng = np.random.default_rng([go * -1, len(tname), 7])
    ectx.set_scoring(sub, go, ge)
    seen = set()
    for lq, n, lo, hi in ((17, 3001, 1, 60), (64, 3001, 1, 60), (300, 401, 1, 1200), (1100, 401, 1, 1200)):
        q = rng.integers(1, 32, size=lq).astype(np.int8)
        flat, off = se.random_db(rng, n, lo, hi)
        lens = np.diff(off.astype(np.int64))
        lens_sorted = np.sort(lens)
        assert lens_sorted[0] == 1 and lens_sorted[1] <= 2 and n % 2 == 1
        if tname != "all_m128":        # plant relatives of the query: its prefixes
            for i in range(0, n, 37):
                m = min(int(lens[i]), lq)
                flat[int(off[i]):int(off[i]) + m] = q[:m]
        want = orc.score_db(q, flat, off, sub, go, ge)
        if tname == "all_127":
            assert np.array_equal(want, 127 * np.minimum(lq, lens))
        elif tname == "all_m128":
            assert not want.any() and orc.topk(want, 10) == [(0, i) for i in range(10)]
        elif tname == "blosum62_dirty0":
            assert np.array_equal(want, orc.score_db(q, flat, off, b62, go, ge))
        ectx.set_query(q)
        for name, opts in _option_sets(lq, lens.max(), int(lens_sorted[-(n // 10)])):
            if name == "long_split" and hi <= 62:
                continue          # (no class of long pairs below 64 rows: nothing to cut off in the short database)
            _search_and_check(swg, orc, ectx, sub, q, flat, off, want, go, ge, 16, True, (tname, lq, name), opts, seen)
    print("table %s gaps %s: (path_bits, cell_form, engine) observed: %s; largest score %d" % (tname, gaps, sorted(seen), int(want.max())))
    _reset_options(ectx)


# ---- 3. batches of queries --------------------------------------------------------------------------------------
BATCH_POINTS = [p for p in se.GAP_POINTS if p["g"] <= 16000]       # g = 2047, 2048, 2049, 16000: eight points


@pytest.mark.parametrize("p", BATCH_POINTS + [None], ids=[se.point_id(p) for p in BATCH_POINTS] + ["full_range"])
def test_gap_points_in_query_batches(swg, orc, ectx, p):
    """swg_search_multi and swg_search_multi_pssm (pssm = sub[q]) either side of the f16 hand-over.  The batch path has
    no re-run, so it takes the f16 cells only where no query can reach 4096 -- and a gap of magnitude g pays only in
    an alignment of more than 2 g: on the f16 forms (3: two queries per lane, 2) a magnitude of 2047 can never show in
    a score, what is tested there is that the unfloored G = M - g and the reset rows leave every score right.  So two
    batches per point: short queries (flanks of 8, 12, 16 and 5: every bound below 4096 -- forms 3, 2, 0 by option at
    g <= 2048, form 0 above), and the point's own query with two of other flank lengths, on which the gap is visible
    (int16 cells, or one query after another where a query can pass 32767).  Odd batch sizes, odd sequence counts.
    full_range (gaps -11 / -1): the short batch only, same forms -- every entry of int8 and garbage in row and column
    0 on the two-queries-per-lane profile.  Form 3 must have run wherever the f16 cells are allowed."""
    if p is None:
        sub, go, ge, f16_ok, g = se.full_range(), -11, -1, True, 300
    else:
        sub, go, ge, f16_ok, g = se.diag127(), p["go"], p["ge"], p["f16"], p["g"]
    rng = np.random.default_rng([g, -ge, 3])
    ectx.set_scoring(sub, go, ge)
    # (a) short queries: bounds 127 * lq < 4096
    qs = [se.split_query(127 * (F - 4), rng)[0] for F in (8, 12, 16)] + [rng.integers(1, 32, size=5).astype(np.int8)]
    # (both odd batch sizes: 3 queries where e is large, 5 elsewhere -- the last pair of an odd batch holds one query twice)
    qs = qs[:3] if p is not None and p["e"] > 1 else qs + [qs[2][:31].copy()]
    assert [len(x) for x in qs[:3]] == [16, 24, 32] and len(qs) % 2 == 1
    _, flat, off, _ = se.split_db(127 * 12, 1201, rng, query=qs[2])
    wants = [orc.score_db(x, flat, off, sub, go, ge) for x in qs]
    lens = np.diff(off.astype(np.int64))
    # no query of the batch can reach the f16 ceiling (the library's own bound, for the index query and for its PSSM)
    assert max(_score_bound(sub, x, lens) for x in qs) < 4096
    ectx.set_query(qs[0])
    seen = set()
    for opts, form in (({}, 3), ({"qq": 0}, 2), ({"f16": 0}, 0)):
        _reset_options(ectx)
        ectx.set_option("engine", 2)
        for key, v in opts.items():
            ectx.set_option(key, v)
        db = swg.Database(flat, off).upload(ectx)
        for route in ("index", "pssm"):
            if route == "index":
                got, hits, st = ectx.search_multi(db, qs, k=5)
            else:
                got, hits, st = ectx.search_multi_pssm(db, [sub[x.astype(np.int64)] for x in qs], k=5)
            for i in range(len(qs)):
                assert np.array_equal(got[i], wants[i]) and hits[i] == orc.topk(wants[i], 5), (p, opts, route, i, st)
            print("batch of short queries", "full_range" if p is None else se.point_id(p), opts, route, "cell_form", st["cell_form"])
            seen.add(st["cell_form"])
            # (two queries per lane need twice the LDS per column: where that does not fit the batch stays on form 2)
            assert st["path_bits"] == 16 and (st["cell_form"] == (form if f16_ok else 0) or (f16_ok and form == 3 and st["cell_form"] == 2)), (p, opts, route, st)
        db.close()
    assert seen == ({0, 2, 3} if f16_ok else {0}), (p, seen)
    if p is None:
        _reset_options(ectx)
        return
    # (b) the point's own query among others: the gap is visible
    sub, q, flat, off, kinds = _point_db(orc, p, 301, 4)
    qs = [se.split_query(127 * 6, rng)[0], q, se.split_query(127 * 40, rng)[0]]
    wants = [orc.score_db(x, flat, off, sub, go, ge) for x in qs]
    for opts in ({}, {"qq": 0}, {"f16": 0}):
        _reset_options(ectx)
        ectx.set_option("engine", 2)
        for key, v in opts.items():
            ectx.set_option(key, v)
        db = swg.Database(flat, off).upload(ectx)
        got, hits, st = ectx.search_multi(db, qs, k=5)
        got_p, hits_p, st_p = ectx.search_multi_pssm(db, [sub[x.astype(np.int64)] for x in qs], k=5)
        db.close()
        for i in range(3):
            assert np.array_equal(got[i], wants[i]) and hits[i] == orc.topk(wants[i], 5), (p, opts, i, st)
            assert np.array_equal(got_p[i], wants[i]) and hits_p[i] == hits[i], (p, opts, i, st_p)
        # (the point's own query can reach 4096 and the batch path has no re-run: int16 cells whatever the options)
        assert st["path_bits"] == st_p["path_bits"] == 16 and st["cell_form"] == st_p["cell_form"] == 0, (p, opts, st, st_p)
        print("batch with the point's own query", se.point_id(p), opts, "cell_form", st["cell_form"], st_p["cell_form"])
    _reset_options(ectx)


# ---- 4. the position-specific route -----------------------------------------------------------------------------
@pytest.mark.parametrize("p", se.GAP_POINTS, ids=se.point_id)
def test_gap_points_position_specific(swg, orc, ectx, p):
    """set_query_pssm(sub[q]) is the index query q: same scores, hits and plan at every gap point."""
    sub, q, flat, off, kinds = _point_db(orc, p, 1001, 5)
    want = orc.score_db(q, flat, off, sub, p["go"], p["ge"])
    ectx.set_scoring(sub, p["go"], p["ge"])
    for opts in ({}, {"f16": 2}, {"engine": 1}, {"force_bits": 32}):
        _reset_options(ectx)
        ectx.set_option("autotune", 0)
        for key, v in opts.items():
            ectx.set_option(key, v)
        db = swg.Database(flat, off).upload(ectx)
        ectx.set_query(q)
        s_idx, h_idx, st_idx = ectx.search(db, k=10)
        ectx.set_query_pssm(sub[q.astype(np.int64)])
        s_p, h_p, st_p = ectx.search(db, k=10)
        db.close()
        assert np.array_equal(s_idx, want) and np.array_equal(s_p, want) and h_p == h_idx == orc.topk(want, 10), (p, opts, st_p)
        assert st_p["path_bits"] == st_idx["path_bits"] == (32 if "force_bits" in opts else p["bits"])
        assert {f: st_p[f] for f in PLAN_FIELDS} == {f: st_idx[f] for f in PLAN_FIELDS}, (p, opts, st_p, st_idx)
    ectx.set_option("autotune", 1)
    ectx.set_query(q)
    _reset_options(ectx)


# ---- 5. alignments ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", se.GAP_POINTS, ids=se.point_id)
def test_gap_points_alignments(swg, orc, ectx, p):
    """Every sequence of the small split_db aligned (swg_align_hits, and swg_align_hits_multi with three queries of
    different flank lengths): score, coordinates and path equal the oracle's and the path's scores add up.  The
    trace kernel works in int32 at every point (hu + go with go down to -65536); at least one path holds an I and
    one a D."""
    sub, q, flat, off, kinds = _point_db(orc, p, 49, 6)
    go, ge = p["go"], p["ge"]
    rng = np.random.default_rng([p["g"], 9])
    _reset_options(ectx)
    ectx.set_scoring(sub, go, ge)
    ectx.set_query(q)
    db = swg.Database(flat, off).upload(ectx)
    scores, _, st = ectx.search(db)
    want = orc.score_db(q, flat, off, sub, go, ge)
    assert np.array_equal(scores, want), st
    every = [(int(scores[i]), i) for i in range(len(scores))]
    als = ectx.align_hits(db, every)
    _check(orc, q, flat, off, sub, go, ge, als, want)
    assert any("I" in a["ops"] for a in als) and any("D" in a["ops"] for a in als)
    qs = [q, se.split_query(127 * 8, rng)[0], np.concatenate([q[:len(q) // 2 - 3], q[len(q) // 2 + 2:]])]
    rows = [[(int(s), i) for i, s in enumerate(orc.score_db(x, flat, off, sub, go, ge))] for x in qs]
    multi = ectx.align_hits_multi(db, qs, rows)
    for x, row, got in zip(qs, rows, multi):
        assert [a["index"] for a in got] == [i for _, i in row]
        _check(orc, x, flat, off, sub, go, ge, got, [s for s, _ in row])
    db.close()


def test_alignments_of_a_wide_query_with_large_gaps(swg, orc, ectx):
    """lq 1800 (flanks of 900) at g = 65536: the trace kernel's form without LDS, with the largest gap magnitudes."""
    p = se.gap_point(-32768, -32768)
    sub = se.diag127()
    rng = np.random.default_rng(1800)
    q = rng.integers(1, 32, size=1800).astype(np.int8)
    _, flat, off, kinds = se.split_db(p["g"], 13, rng, query=q)
    # (e = 32768: only single indels pay -- one of each, whatever the builder drew)
    seqs = [np.concatenate([q[:900], q[:1], q[900:]]), np.concatenate([q[:899], q[900:]])] + se.seqs_of(flat, off)
    kinds = np.concatenate([[1, 2], kinds])
    flat = np.concatenate(seqs)
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
    n_gap, n_i, n_d = se.gapped_relatives(orc, q, flat, off, kinds, sub, p["go"], p["ge"])
    assert n_gap >= 2 and n_i and n_d
    _reset_options(ectx)
    ectx.set_scoring(sub, p["go"], p["ge"])
    ectx.set_query(q)
    db = swg.Database(flat, off).upload(ectx)
    scores, _, st = ectx.search(db)
    want = orc.score_db(q, flat, off, sub, p["go"], p["ge"])
    assert np.array_equal(scores, want) and st["path_bits"] == 32
    als = ectx.align_hits(db, [(int(s), i) for i, s in enumerate(scores)])
    _check(orc, q, flat, off, sub, p["go"], p["ge"], als, want)
    assert any("I" in a["ops"] for a in als) and any("D" in a["ops"] for a in als)
    db.close()


# ---- 6. reference-shaped batches: the gapedge_* fixtures are in test_golden_through_reference_shaped_batches' list ----


# ---- 7. the range of swg_set_scoring ----------------------------------------------------------------------------
def test_set_scoring_range(swg, orc, ectx):
    """-32768 and 32767 are accepted for either score, -32769 and 32768 are SWG_ERR_ARG, and a refused call leaves the
    context searching with the scoring it had."""
    sub = se.diag127()
    p = se.gap_point(-2047, -1)
    _, q, flat, off, _ = _point_db(orc, p, 301, 8)
    want = orc.score_db(q, flat, off, sub, p["go"], p["ge"])
    _reset_options(ectx)
    for go, ge in ((-32768, -1), (32767, -1), (-1, -32768), (-1, 32767), (-32768, -32768), (32767, 32767)):
        ectx.set_scoring(sub, go, ge)
    ectx.set_scoring(sub, p["go"], p["ge"])
    ectx.set_query(q)
    db = swg.Database(flat, off).upload(ectx)
    for go, ge in ((-32769, -1), (32768, -1), (-1, -32769), (-1, 32768)):
        with pytest.raises(swg.SwgError) as e:
            ectx.set_scoring(sub, go, ge)
        assert e.value.code == swg.SWG_ERR_ARG
        got, hits, st = ectx.search(db, k=5)
        assert np.array_equal(got, want) and hits == orc.topk(want, 5), (go, ge, st)
    db.close()


# ---- 8. positive increments of real size ------------------------------------------------------------------------
@pytest.mark.parametrize("gaps", [(300, -1), (0, 200), (-50, 127)])
@pytest.mark.parametrize("opts", [{}, {"cols_per_wave": 7, "group_lanes": 16}, {"work_queue": 0}, {"engine": 1}],
                         ids=["default", "k7_g16", "work_queue_0", "engine1"])
def test_positive_increments_of_real_size(swg, orc, ectx, gaps, opts):
    """Gap scores whose increment is positive and large run on the exact int32 cells.  No cell value can exceed
    (lq + len) * 300 (every step of a path adds at most 300): with lq <= 400 and len <= 400 that is 240 000, four
    orders of magnitude below 2^31 -- the overflow itself is not probed."""
    go, ge = gaps
    sub = swg.load_scoring("BLOSUM62").table()
    for lq, n in ((61, 501), (400, 201)):
        rng = np.random.default_rng([lq, go + 100, ge + 100])
        q = rng.integers(1, 25, size=lq).astype(np.int8)
        flat, off = se.random_db(rng, n, 1, 400, hi=24)
        assert (lq + int(np.diff(off.astype(np.int64)).max())) * 300 <= 240000 < 2 ** 31 // 1000
        want = orc.score_db(q, flat, off, sub, go, ge)
        _reset_options(ectx)
        ectx.set_scoring(sub, go, ge)
        ectx.set_query(q)
        for key, v in opts.items():
            ectx.set_option(key, v)
        db = swg.Database(flat, off).upload(ectx)
        got, hits, st = ectx.search(db, k=8)
        db.close()
        assert np.array_equal(got, want), (gaps, opts, lq, st)
        assert hits == orc.topk(want, 8) and st["path_bits"] == 32
    _reset_options(ectx)


# ---- 9. a class that fits one segment of a buffer that does not --------------------------------------------------
@pytest.mark.parametrize("opts", [{"cols_per_wave": 24, "group_lanes": 32, "max_waves": 4},
                                  {"cols_per_wave": 24, "group_lanes": 32, "max_waves": 4, "wide16": 0}],
                         ids=["wide", "int16"])
def test_bulk_behind_a_long_class_in_one_segment(swg, orc, ectx, opts):
    """Found by the edges soak (fuzz_gpu seed 11, case 885): the kernels with edges -- every pass of a multi-pass
    fill, and the wide form even in one pass -- address tokens from their segment's origin.  With two classes and
    segment_blocks below the whole buffer, a class that fits ONE segment was launched with origin 0 and no blocks:
    400 sequences of 1 .. 7 residues behind a long class of 16 pairs all scored 0.  Two classes off the work queue
    exist in one pass only, so the wide form in one pass is where it shows (the plain int16 cells, without edges
    there, are the control).  Same shape here: the relatives of a 524-column query (long class) and 400 tiny
    sequences (bulk), segments of about five long pairs."""
    p = se.gap_point(-32766, -1)
    sub = se.diag127()
    rng = np.random.default_rng(885)
    q, flat, off, _ = se.split_db(p["g"], 37, rng)
    seqs = se.seqs_of(flat, off) + [rng.integers(1, 32, size=int(L)).astype(np.int8) for L in rng.integers(1, 8, size=400)]
    seqs = [seqs[i] for i in rng.permutation(len(seqs))]
    flat = np.concatenate(seqs)
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
    lens = np.diff(off.astype(np.int64))
    want = orc.score_db(q, flat, off, sub, p["go"], p["ge"])
    assert (want[lens <= 7] > 0).sum() > 300
    _reset_options(ectx)
    ectx.set_scoring(sub, p["go"], p["ge"])
    ectx.set_query(q)
    ectx.set_option("engine", 2)
    ectx.set_option("f16", 0)
    ectx.set_option("segment_blocks", (int(lens.max()) + 5) // 4 * 5 + 1)
    for key, v in opts.items():
        ectx.set_option(key, v)
    db = swg.Database(flat, off).upload(ectx)
    got, hits, st = ectx.search(db, k=10)
    db.close()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (opts, st, bad[:8], lens[bad[:8]], got[bad[:8]], want[bad[:8]])
    assert hits == orc.topk(want, 10)
    # the shape the test is for: two classes, cells with edges, more launches than passes only for the long class
    assert st["long_pairs"] > 0 and st["cell_form"] == (0 if opts.get("wide16") == 0 else 1), st
    assert st["passes"] == -(-len(q) // (opts["cols_per_wave"] * opts["group_lanes"])), st
    _reset_options(ectx)
