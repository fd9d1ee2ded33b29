"""GPU (-m gpu): several non-overlapping alignments per hit on the device (swg_align_hsps, swg_align_hsps_multi,
swg_align_hsps_multi_pssm).

Every case of hsps_cases.py runs through swg_align_hsps and, grouped into batches, through the two batch calls; the
number of alignments, every field, every path and every count must equal the host twin swg_align_hsps_host exactly, and
on the small cases the Python model of hsps_model.py too.  There is no tolerance and no case is left out.  Then what
the calls promise around that: equality with swg_align_hits*, outputs that are not wanted, a batch of several launches
with unwritten slots, repeated hits, views, a context left as it was, and refusals that touch nothing."""
import ctypes as C

import numpy as np
import pytest

import hsps_cases as hc
import hsps_model as hm

pytestmark = pytest.mark.gpu

FIELDS = ("score", "q_begin", "q_end", "d_begin", "d_end", "n_ops", "ops", "n_ident", "n_match", "n_gap_open", "n_gap")
SENTINEL = 0xAB


@pytest.fixture(scope="module")
def hctx(swg):
    c = swg.Context(0)
    c.set_option("autotune", 0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def world(swg, hctx):
    """The cases, one resident database that holds case c's sequence as entry c (the free PSSM's last), and what the
    host twin (every case) and the model (the small ones) say: computed once, shared, never changed."""
    b62, pam = swg.load_scoring("BLOSUM62").table(), swg.load_scoring("PAM250").table()
    cases = hc.all_cases(b62, pam)
    free = hc.free_pssm_case()
    seqs = [c["seq"] for c in cases] + [free["seq"]]
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    flat = np.ascontiguousarray(np.concatenate(seqs), dtype=np.int8)
    db = swg.Database(flat, off).upload(hctx)
    twin, twin_p, model = [], [], {}
    for n, c in enumerate(cases):
        kw = dict(max_hsps=c["max_hsps"], min_score=c["min_score"], want_counts=True)
        twin.append(swg.align_hsps_host(c["sub"], c["gap_open"], c["gap_extend"], c["seq"], query=c["query"], **kw))
        twin_p.append(swg.align_hsps_host(None, c["gap_open"], c["gap_extend"], c["seq"], pssm=hc.pssm_of(c), **kw))
        if c["small"]:
            model[n] = hm.align(c["sub"], c["gap_open"], c["gap_extend"], c["seq"], c["max_hsps"], c["min_score"], query=c["query"])[0]
    free_twin = swg.align_hsps_host(None, free["gap_open"], free["gap_extend"], free["seq"], pssm=free["pssm"], max_hsps=free["max_hsps"],
                                    min_score=free["min_score"], want_counts=True)
    yield {"cases": cases, "free": free, "db": db, "flat": flat, "off": off, "twin": twin, "twin_p": twin_p, "model": model,
           "free_twin": free_twin}
    db.close()


def strip(als):
    return [{f: a[f] for f in FIELDS} for a in als]


def placed(als, index):
    """The twin's alignments as the device reports them for entry `index`."""
    return [dict(a, index=index) for a in als]


def groups(cases):
    """Cases that one batch call can hold: the same scoring and the same limits -> {key: [case numbers]}."""
    out = {}
    for n, c in enumerate(cases):
        key = (c["sub"].tobytes(), c["gap_open"], c["gap_extend"], c["max_hsps"], c["min_score"])
        out.setdefault(key, []).append(n)
    return out


def set_case(ctx, c):
    ctx.set_scoring(c["sub"], c["gap_open"], c["gap_extend"])


# ---- 1. every case, one call each, against the twin and the model ------------------------------------------------------
def test_every_case_through_the_single_call(hctx, world):
    db = world["db"]
    for n, c in enumerate(world["cases"]):
        set_case(hctx, c)
        hctx.set_query(c["query"])
        got = hctx.align_hsps(db, [(0, n)], c["max_hsps"], c["min_score"], want_counts=True)
        assert got == [placed(world["twin"][n], n)], c["name"]
        if n in world["model"]:
            assert strip(got[0]) == strip(world["model"][n]), c["name"]
        hctx.set_query_pssm(hc.pssm_of(c))
        got = hctx.align_hsps(db, [(0, n)], c["max_hsps"], c["min_score"], want_counts=True)
        assert got == [placed(world["twin_p"][n], n)], c["name"]
    f, n = world["free"], len(world["cases"])
    hctx.set_scoring(np.zeros((32, 32), dtype=np.int8), f["gap_open"], f["gap_extend"])      # (the table is not read under a PSSM)
    hctx.set_query_pssm(f["pssm"])
    got = hctx.align_hsps(db, [(0, n)], f["max_hsps"], f["min_score"], want_counts=True)
    assert len(got[0]) >= 2 and got == [placed(world["free_twin"], n)]


# ---- 2. the same cases grouped into batches: both batch calls ----------------------------------------------------------
def test_every_case_through_the_batch_calls(hctx, world):
    db, cases = world["db"], world["cases"]
    for key, members in groups(cases).items():
        c0 = cases[members[0]]
        set_case(hctx, c0)
        qs = [cases[n]["query"] for n in members]
        hits = [[(0, n)] for n in members]
        got = hctx.align_hsps_multi(db, qs, hits, c0["max_hsps"], c0["min_score"], want_counts=True)
        assert got == [[placed(world["twin"][n], n)] for n in members], c0["name"]
        got = hctx.align_hsps_multi_pssm(db, [hc.pssm_of(cases[n]) for n in members], hits, c0["max_hsps"], c0["min_score"], want_counts=True)
        assert got == [[placed(world["twin_p"][n], n)] for n in members], c0["name"]


# ---- 3. equality with swg_align_hits* -----------------------------------------------------------------------------------
def test_one_hsp_at_score_one_is_align_hits(hctx, world):
    """max_hsps = 1 / min_score = 1 equals swg_align_hits* on the same hits, fields and paths; and so does the first
    alignment under the case's own limits wherever the pair reaches its min_score."""
    db, cases = world["db"], world["cases"]
    for key, members in groups(cases).items():
        c0 = cases[members[0]]
        set_case(hctx, c0)
        qs = [cases[n]["query"] for n in members]
        hits = [[(0, n), (0, members[0])] for n in members]               # two hits a row: the row's own and the group's first
        want = hctx.align_hits_multi(db, qs, hits)
        got = hctx.align_hsps_multi(db, qs, hits, 1, 1)
        assert [[als for als in row] for row in got] == [[[a] if a["score"] > 0 else [] for a in row] for row in want], c0["name"]
        more = hctx.align_hsps_multi(db, qs, hits, c0["max_hsps"], c0["min_score"])
        for row, wrow in zip(more, want):
            for als, a in zip(row, wrow):
                assert (als[0] == a) if a["score"] >= c0["min_score"] else (als == []), c0["name"]
        ps = [hc.pssm_of(cases[n]) for n in members]
        assert [[als for als in row] for row in hctx.align_hsps_multi_pssm(db, ps, hits, 1, 1)] == \
            [[[a] if a["score"] > 0 else [] for a in row] for row in hctx.align_hits_multi_pssm(db, ps, hits)]
        n = members[-1]
        hctx.set_query(cases[n]["query"])
        single = hctx.align_hits(db, [(0, n)])
        assert hctx.align_hsps(db, [(0, n)], 1, 1) == [[a] if a["score"] > 0 else [] for a in single]


# ---- 4. outputs that are not wanted -------------------------------------------------------------------------------------
def test_without_paths_and_without_counts(hctx, world):
    db, cases = world["db"], world["cases"]
    n = next(i for i, c in enumerate(cases) if c["name"] == "matrix_blosum62")
    c = cases[n]
    set_case(hctx, c)
    hctx.set_query(c["query"])
    full = hctx.align_hsps(db, [(0, n)], c["max_hsps"], c["min_score"], want_counts=True)[0]
    assert len(full) >= 3
    keep = ("score", "index", "q_begin", "q_end", "d_begin", "d_end", "n_ops")
    for want_ops, want_counts in ((False, False), (True, False), (False, True)):
        got = hctx.align_hsps(db, [(0, n)], c["max_hsps"], c["min_score"], want_ops=want_ops, want_counts=want_counts)[0]
        names = keep + (("ops",) if want_ops else ()) + (tuple(FIELDS[7:]) if want_counts else ())
        assert got == [{k: a[k] for k in names} for a in full]


# ---- raw calls: what is and is not written -------------------------------------------------------------------------------
def raw_multi(swg, ctx, db, queries, hits, k, max_hsps, min_score, n_hits=None, pssm=False):
    """swg_align_hsps_multi[_pssm] over buffers filled with a sentinel -> (rc, out bytes [nq*k*max_hsps, 32], n_hsps bytes
    [nq*k, 4], counts bytes, ops bytes [nq*k*max_hsps, stride]) as uint8 arrays."""
    nq = len(queries)
    qoff = np.zeros(nq + 1, dtype=np.uint64)
    qoff[1:] = np.cumsum([len(q) for q in queries])
    qflat = np.ascontiguousarray(np.concatenate(queries), dtype=np.int8)
    arr = (swg.Hit * max(nq * k, 1))()
    nh = (C.c_size_t * nq)()
    for i, row in enumerate(hits):
        nh[i] = len(row) if n_hits is None else n_hits[i]
        for j, (sc, ix) in enumerate(row):
            arr[i * k + j].score, arr[i * k + j].index = sc, ix
    vp = C.c_void_p
    stride = int(swg.lib.swg_align_ops_bound_multi(db.handle, qoff.ctypes.data_as(vp), nq))
    per = max(max_hsps, 1)
    out = np.full((nq * k * per, 32), SENTINEL, dtype=np.uint8)
    nout = np.full((nq * k, 4), SENTINEL, dtype=np.uint8)
    cnt = np.full((nq * k * per, 16), SENTINEL, dtype=np.uint8)
    ops = np.full((nq * k * per, stride), SENTINEL, dtype=np.uint8)
    fn = swg.lib.swg_align_hsps_multi_pssm if pssm else swg.lib.swg_align_hsps_multi
    rc = fn(ctx.handle, db.handle, qflat.ctypes.data_as(vp), qoff.ctypes.data_as(vp), nq, C.cast(arr, vp), k, C.cast(nh, vp), max_hsps,
            min_score, out.ctypes.data_as(vp), nout.ctypes.data_as(vp), cnt.ctypes.data_as(vp), ops.ctypes.data_as(vp), stride)
    return rc, out, nout, cnt, ops


def untouched(*arrays):
    return all((a == SENTINEL).all() for a in arrays)


# ---- 5. a mixed batch: several launches, shared sequences, short rows, unwritten slots ----------------------------------
def test_mixed_batch_of_several_launches_keeps_unwritten_slots(swg, hctx, world):
    """Queries of 255 and 600 columns (two LDS classes) and 1701 (the class above the LDS limit): three launches.  Entry
    `shared` is hit by all of them; row 1 holds fewer hits than k and row 3 none."""
    db, cases = world["db"], world["cases"]
    by_name = {c["name"]: n for n, c in enumerate(cases)}
    n255, n600, n1701 = by_name["width_255"], by_name["width_600"], by_name["width_1701"]
    shared = n600
    c0 = cases[n255]
    set_case(hctx, c0)
    qs = [cases[n255]["query"], cases[n600]["query"], cases[n1701]["query"], cases[n255]["query"]]
    k, H, ms = 3, 5, 30
    hits = [[(0, n255), (0, shared), (0, n1701)], [(0, shared), (0, n600)], [(0, n1701), (0, shared), (0, n255)], []]
    rc, out, nout, cnt, ops = raw_multi(swg, hctx, db, qs, hits, k, H, ms)
    assert rc == swg.SWG_OK
    got = hctx.align_hsps_multi(db, qs, hits, H, ms, want_counts=True)
    nh = nout.view(np.uint32).reshape(len(qs), k)
    al = out.view(np.uint32).reshape(len(qs), k, H, 8)
    for i, row in enumerate(hits):
        for j in range(k):
            if j >= len(row):
                assert untouched(nout[i * k + j], out[(i * k + j) * H:(i * k + j + 1) * H], cnt[(i * k + j) * H:(i * k + j + 1) * H],
                                 ops[(i * k + j) * H:(i * k + j + 1) * H])
                continue
            index = row[j][1]
            want = swg.align_hsps_host(c0["sub"], c0["gap_open"], c0["gap_extend"], cases[index]["seq"], H, ms, query=qs[i], want_counts=True)
            assert got[i][j] == placed(want, index)
            assert nh[i, j] == len(want)
            assert [int(x) for x in al[i, j, :len(want), 0]] == [a["score"] for a in want] and (al[i, j, :len(want), 7] == 0).all()
            s = (i * k + j) * H
            assert untouched(out[s + len(want):s + H], cnt[s + len(want):s + H], ops[s + len(want):s + H])   # slots past n_hsps
    assert len(got[0][0]) >= 3 and len(got[1][1]) >= 3 and len(got[2][0]) >= 3


# ---- 6. repeated hits: marks must not leak between jobs -----------------------------------------------------------------
def test_a_hit_repeated_in_one_call_gets_the_same_answer(hctx, world):
    db, cases = world["db"], world["cases"]
    n = next(i for i, c in enumerate(cases) if c["name"] == "repeat")
    c = cases[n]
    set_case(hctx, c)
    hctx.set_query(c["query"])
    got = hctx.align_hsps(db, [(0, n)] * 5, c["max_hsps"], c["min_score"], want_counts=True)
    assert got == [placed(world["twin"][n], n)] * 5 and len(got[0]) == 5
    assert [(a["score"], a["q_begin"], a["q_end"], a["d_begin"], a["d_end"], a["n_ops"]) for a in got[0]] == hc.REPEAT_EXPECTED


# ---- 7. a view ---------------------------------------------------------------------------------------------------------
def test_a_view_gives_the_same_alignments_with_original_indices(hctx, world):
    db, cases = world["db"], world["cases"]
    by_name = {c["name"]: n for n, c in enumerate(cases)}
    members = [by_name["domains_swapped"], by_name["matrix_blosum62"], by_name["width_257"]]
    c0 = cases[members[0]]
    assert all(cases[n]["sub"].tobytes() == c0["sub"].tobytes() for n in members)
    hctx.set_scoring(c0["sub"], -11, -1)
    view = db.view(hctx, members)
    qs = [cases[n]["query"] for n in members]
    hits = [[(0, n)] for n in members]
    assert hctx.align_hsps_multi(view, qs, hits, 5, 30, want_counts=True) == hctx.align_hsps_multi(db, qs, hits, 5, 30, want_counts=True)
    hctx.set_query(qs[2])
    got = hctx.align_hsps(view, hits[2], 5, 30)
    assert got == hctx.align_hsps(db, hits[2], 5, 30) and got[0][0]["index"] == members[2]
    view.close()


# ---- 8. the context afterwards -------------------------------------------------------------------------------------------
def test_the_context_is_left_as_it_was_and_calls_repeat(swg, hctx, world):
    db, cases = world["db"], world["cases"]
    by_name = {c["name"]: n for n, c in enumerate(cases)}
    own = cases[by_name["matrix_blosum62"]]
    set_case(hctx, own)
    hctx.set_query(own["query"])
    before = hctx.search(db, k=5)
    members = [by_name["width_256"], by_name["domains_swapped"]]
    qs = [cases[n]["query"] for n in members]
    hits = [[(0, n)] for n in members]
    first = hctx.align_hsps_multi(db, qs, hits, 5, 30, want_counts=True)
    again = hctx.align_hsps_multi(db, qs, hits, 5, 30, want_counts=True)
    assert first == again and all(len(row[0]) >= 2 for row in first)
    after = hctx.search(db, k=5)
    assert (before[0] == after[0]).all() and before[1] == after[1]
    n = by_name["matrix_blosum62"]                                        # the context's own query still scores its calls
    assert hctx.align_hsps(db, [(0, n)], own["max_hsps"], own["min_score"], want_counts=True) == [placed(world["twin"][n], n)]


# ---- 9. refusals come before anything is written --------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(swg, hctx, world):
    db, cases = world["db"], world["cases"]
    n = next(i for i, c in enumerate(cases) if c["name"] == "repeat")
    c = cases[n]
    set_case(hctx, c)
    qs, total = [c["query"], c["query"]], len(cases) + 1

    def refused(code, text, *a, **kw):
        rc, out, nout, cnt, ops = raw_multi(swg, hctx, *a, **kw)
        assert rc == code and text in swg.lib.swg_last_error(hctx.handle).decode(), swg.lib.swg_last_error(hctx.handle)
        assert untouched(out, nout, cnt, ops)

    good = [[(0, n)], [(0, n)]]
    refused(swg.SWG_ERR_ARG, "swg_align_hsps_multi: max_hsps 0 outside 1..64", db, qs, good, 1, 0, 1)
    refused(swg.SWG_ERR_ARG, "swg_align_hsps_multi: max_hsps 65 outside 1..64", db, qs, good, 1, 65, 1)
    refused(swg.SWG_ERR_ARG, "swg_align_hsps_multi: min_score 0 below 1", db, qs, good, 1, 4, 0)
    refused(swg.SWG_ERR_ARG, "swg_align_hsps_multi_pssm: min_score -5 below 1", db, [hc.pssm_of(c)] * 2, good, 1, 4, -5, pssm=True)
    # the second row's hit is not in the database: the first row's pair is not run either
    refused(swg.SWG_ERR_ARG, "swg_align_hsps_multi: sequence %u is not in this database shard" % total, db, qs, [[(0, n)], [(0, total)]], 1, 4, 1)
    refused(swg.SWG_ERR_ARG, "swg_align_hsps_multi: row 1 holds 2 hits, more than k = 1", db, qs, good, 1, 4, 1, n_hits=[1, 2])
    host_only = swg.Database(world["flat"], world["off"])
    refused(swg.SWG_ERR_STATE, "swg_align_hsps_multi: database is not resident", host_only, qs, good, 1, 4, 1)
    hctx.set_query(c["query"])
    for bad, text in (((0, 1), "max_hsps 0 outside 1..64"), ((65, 1), "max_hsps 65 outside 1..64"), ((4, 0), "min_score 0 below 1")):
        with pytest.raises(swg.SwgError) as e:
            hctx.align_hsps(db, [(0, n)], *bad)
        assert e.value.code == swg.SWG_ERR_ARG and "swg_align_hsps: " + text in str(e.value)
    with pytest.raises(swg.SwgError) as e:
        hctx.align_hsps(host_only, [(0, n)], 4, 1)
    assert e.value.code == swg.SWG_ERR_STATE and "swg_align_hsps: database is not resident" in str(e.value)
    with pytest.raises(swg.SwgError) as e:
        hctx.align_hsps(db, [(0, total)], 4, 1)
    assert e.value.code == swg.SWG_ERR_ARG and "swg_align_hsps: sequence %u is not in this database shard" % total in str(e.value)
    vp = C.c_void_p
    hit = (swg.Hit * 1)()
    hit[0].index = n
    out = (swg.Alignment * 4)()
    assert swg.lib.swg_align_hsps(hctx.handle, db.handle, C.cast(hit, vp), 1, 4, 1, C.cast(out, vp), None, None, None, 0) == swg.SWG_ERR_ARG
    assert b"swg_align_hsps: NULL argument" in swg.lib.swg_last_error(hctx.handle)
    host_only.close()
