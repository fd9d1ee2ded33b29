"""GPU (-m gpu): the reference-shaped replay (swg_fill_batches16) at its edges -- the calls of tests/batches16_cases.py
through the C function itself, with buffers of the test's own, on both routes: "device" (the batches uploaded as they
are, pair tokens built from them on the device, in buffers the context keeps between calls) and "host" (work_queue = 0:
un-transposed and packed on the host).  Truth is the int32 oracle on every lane's column as given, delivered as
min(truth, 32767); every comparison is bit-exact.  max_scores are pre-filled with a sentinel: the entries at or beyond
vector_size must still hold it.  tests/test_batches16_cases_host.py proves without a device that the calls are what they
claim, and holds their truths against the reference's own fill."""
import ctypes as C

import numpy as np
import pytest

import batches16_cases as bc
from test_gpu_parity import _reset_options

pytestmark = pytest.mark.gpu

ROUTES = ("device", "host")


@pytest.fixture(scope="module")
def bctx(swg):
    c = swg.Context(0)
    c.set_option("autotune", 0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _options(swg, bctx):
    _reset_options(bctx)
    yield
    swg.debug_launch_log(False)
    _reset_options(bctx)


class Call:
    """One swg_fill_batches16 call: the swg_batch16 array and the max_scores it points to, [n][16] int16 of SENTINEL."""

    def __init__(self, swg, batches):
        n = len(batches)
        self.batches = batches
        self.arr = (swg.Batch16 * max(n, 1))()
        self.out = np.full((max(n, 1), 16), bc.SENTINEL, dtype=np.int16)
        for i, (a, vs) in enumerate(batches):
            assert a.dtype == np.int8 and a.flags.c_contiguous and a.shape[1] == 16
            self.arr[i].db_idx_t = a.ctypes.data
            self.arr[i].max_len = a.shape[0]
            self.arr[i].vector_size = vs
            self.arr[i].max_scores = self.out[i].ctypes.data
        self.swg = swg

    def run(self, ctx, n=None, seconds=True):
        """-> (return code, the context's message)."""
        secs = C.c_double(-1.0)
        rc = self.swg.lib.swg_fill_batches16(ctx.handle, self.arr, len(self.batches) if n is None else n,
                                             C.byref(secs) if seconds else None)
        if seconds:
            assert secs.value >= 0.0
        return rc, (self.swg.lib.swg_last_error(ctx.handle) or b"").decode("utf-8", "replace")

    def untouched(self):
        return bool((self.out == bc.SENTINEL).all())


def _set(ctx, case, route="device"):
    ctx.set_scoring(case["sub"], *case["gaps"])
    ctx.set_query(case["query"])
    ctx.set_option("work_queue", 0 if route == "host" else 1)


def _check(call, case, label):
    """Every live lane against min(truth, 32767), every other entry of max_scores against the sentinel."""
    for b, ((a, vs), want) in enumerate(zip(case["batches"], bc.expected(case))):
        got = call.out[b]
        assert np.array_equal(got[:vs], want), (label, case["name"], b, a.shape[0], vs, got[:vs].tolist(), want.tolist())
        assert (got[vs:] == bc.SENTINEL).all(), (label, case["name"], b, a.shape[0], vs, got.tolist())


def _fill(swg, ctx, case, label, log=False):
    """One call of the case on ctx as it is set up, checked lane for lane -> the launch log if asked for."""
    call = Call(swg, case["batches"])
    if log:
        swg.debug_launch_log(True)
    rc, msg = call.run(ctx)
    recs = swg.debug_launch_log_read() if log else None
    if log:
        swg.debug_launch_log(False)
    assert rc == swg.SWG_OK, (label, case["name"], rc, msg)
    _check(call, case, (label, recs))
    return recs


def _assert_route(recs, route, label):
    """What the launch log can tell of the route: the device route's database has pair tokens only, so what works off it
    is the work-queue lane-group launch ("dyn"); work_queue = 0 on the host route's packed database takes fixed streams."""
    main = [r["family"] for r in recs if not r["list"]]
    assert main and set(main) == {"dyn" if route == "device" else "streams"}, (label, route, recs)


def _as_database(case):
    """The live lanes of a case as an ordinary database: (flat, offsets, truth)."""
    cols = [np.ascontiguousarray(a[:, l]) for a, vs in case["batches"] for l in range(vs)]
    off = np.zeros(len(cols) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(c) for c in cols])
    return np.concatenate(cols), off, np.concatenate(case["truth"])


# ---- 1. the shape matrix ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
def test_shape_matrix(swg, bctx, route):
    """max_len 1 .. 9, 15, 16, 17 x vector_size 0, 1, 2, 3, 15, 16 in one call: every live lane, nothing written at or
    beyond vector_size (all 16 of an empty batch), bytes outside 1..31 in the dead lanes accepted; and the same batches
    in a seeded random order give the same results batch for batch."""
    case = bc.shape_matrix()
    _set(bctx, case, route)
    _assert_route(_fill(swg, bctx, case, route, log=True), route, "sorted")
    _assert_route(_fill(swg, bctx, bc.shuffled(), route, log=True), route, "shuffled")


# ---- 2. the ceilings of the cells ------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide16", [1, 0])
@pytest.mark.parametrize("route", ROUTES)
def test_ceilings(swg, bctx, route, wide16):
    """Truths 4064, 4191, 32766, 32767, 32768, 32893 and 66040 among lanes in the hundreds: min(truth, 32767) exactly --
    saturated, not wrapped, 32766 not rounded up.  On the device route the levels behind the first run on pair tokens
    alone: the re-run of what a level flagged is a launch off a list, and what passes 65535 (wide16 = 0: 32767) is
    re-scored by the int32 lane groups."""
    case = bc.ceilings()
    _set(bctx, case, route)
    bctx.set_option("wide16", wide16)
    recs = _fill(swg, bctx, case, (route, wide16), log=True)
    _assert_route(recs, route, wide16)
    if route == "device":
        assert any(r["list"] == 1 for r in recs), recs
        assert any(r["family"] == "q32" and r["list"] == 1 for r in recs), recs


# ---- 3. queries of several passes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("f16", [1, 0])
@pytest.mark.parametrize("route", ROUTES)
def test_multipass(swg, bctx, route, f16):
    """2100 query columns: relatives across every pass boundary, a third of them gapped; f16 automatic and off."""
    case = bc.multipass()
    _set(bctx, case, route)
    bctx.set_option("f16", f16)
    recs = _fill(swg, bctx, case, (route, f16), log=True)
    if route == "device":
        _assert_route(recs, route, f16)
        assert all(r["edges"] == 1 for r in recs if not r["list"]) and sum(not r["list"] for r in recs) >= 2, recs
        if f16 == 0:
            assert all(r["form"] != 2 for r in recs), recs


# ---- 4. an upload in several runs ------------------------------------------------------------------------------------
def test_staging_runs(swg, bctx):
    """9.6 MB to stage (three runs of the upload), handed over unsorted: copies in the first rows, the middle and the last
    rows of the long lanes, and the small batches behind them."""
    case = bc.staging()
    _set(bctx, case)
    _assert_route(_fill(swg, bctx, case, "staging", log=True), "device", "staging")


# ---- 5. BLOSUM62 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
def test_mixed_blosum62(swg, bctx, route):
    case = bc.mixed()
    _set(bctx, case, route)
    _fill(swg, bctx, case, route)


# ---- 6. one context, call after call -------------------------------------------------------------------------------------
def test_sequence_of_calls_on_one_context(swg):
    """The cache of device and pinned buffers is grown, never shrunk: a small call, one that grows every buffer, the small
    one again (stale tokens and lengths behind it), other queries, scorings and pass counts, an ordinary search in
    between, the other route and back -- every call lane for lane against its own truth."""
    ctx = swg.Context(0)
    ctx.set_option("autotune", 0)
    try:
        small, other = bc.shape_matrix(0), bc.shape_matrix(1)
        _set(ctx, small)
        _fill(swg, ctx, small, "1 small")
        _set(ctx, bc.staging())
        _fill(swg, ctx, bc.staging(), "2 grows")
        _set(ctx, small)
        _fill(swg, ctx, small, "3 small again")
        _fill(swg, ctx, bc.shuffled(0), "3 shuffled")
        _set(ctx, bc.multipass())
        _fill(swg, ctx, bc.multipass(), "4 multipass")
        ctx.set_query(other["query"])                    # (the scoring stays: both are the hot table's)
        _fill(swg, ctx, other, "5 another query")
        _set(ctx, bc.mixed())
        _fill(swg, ctx, bc.mixed(), "5 another scoring")
        # an ordinary search of a resident database on the same context
        _set(ctx, bc.multipass())
        flat, off, truth = _as_database(bc.multipass())
        db = swg.Database(flat, off).upload(ctx)
        scores, hits, _ = ctx.search(db, k=5)
        assert np.array_equal(scores, truth)
        _fill(swg, ctx, bc.multipass(), "6 behind a search")
        scores, _, _ = ctx.search(db)
        assert np.array_equal(scores, truth)
        db.close()
        _set(ctx, bc.ceilings())
        _fill(swg, ctx, bc.ceilings(), "7 ceilings")
        _set(ctx, small, "host")
        _assert_route(_fill(swg, ctx, small, "8 host", log=True), "host", 8)
        _set(ctx, small, "device")
        _assert_route(_fill(swg, ctx, small, "8 device again", log=True), "device", 8)
        _set(ctx, bc.ceilings())
        _fill(swg, ctx, bc.ceilings(), "9 ceilings again")
        _set(ctx, small)
        _fill(swg, ctx, small, "9 small")
    finally:
        swg.debug_launch_log(False)
        ctx.close()


# ---- 7. a residue outside 1..31 in a live lane ---------------------------------------------------------------------------
def _bad_spots(case):
    """(batch, row, lane) of the three places, all in one batch of 15 lanes in the middle of the call."""
    n = len(case["batches"])
    b = next(i for i in range(n // 3, n) if case["batches"][i][1] == 15 and case["batches"][i][0].shape[0] >= 4)
    max_len = case["batches"][b][0].shape[0]
    return {"lane0_row0": (b, 0, 0), "lane1_last_row": (b, max_len - 1, 1), "unpaired_last_lane": (b, max_len // 2, 14)}


@pytest.mark.parametrize("spot", ["lane0_row0", "lane1_last_row", "unpaired_last_lane"])
@pytest.mark.parametrize("route", ROUTES)
def test_bad_residue_is_refused_and_forgotten(swg, bctx, route, spot):
    """A single 0, 32 or -1 in a live lane of a batch in the middle of the call: SWG_ERR_RESIDUE, the message names the
    batches; the next, clean call on the same context is right (the device route's flag word is zeroed per call)."""
    case = bc.shape_matrix()
    _set(bctx, case, route)
    b, row, lane = _bad_spots(case)[spot]
    assert 0 < b < len(case["batches"]) - 1 and lane < case["batches"][b][1]
    for byte in (0, 32, -1):
        a = case["batches"][b][0].copy()
        a[row, lane] = byte
        batches = list(case["batches"])
        batches[b] = (a, batches[b][1])
        rc, msg = Call(swg, batches).run(bctx)
        assert rc == swg.SWG_ERR_RESIDUE, (route, spot, byte, rc, msg)
        assert "swg_fill_batches16" in msg and "batch" in msg and "1..31" in msg, (route, spot, byte, msg)
        _fill(swg, bctx, case, (route, spot, byte, "clean call behind the refusal"))


# ---- 8. state and arguments ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
def test_refused_while_a_search_is_in_flight(swg, bctx, route):
    """A swg_search_begin ticket outstanding: SWG_ERR_STATE on either route, nothing written; swg_search_end still gives
    that search's result, and the call then succeeds."""
    case = bc.shape_matrix()
    _set(bctx, case, route)
    flat, off, truth = _as_database(case)
    db = swg.Database(flat, off).upload(bctx)
    ticket = bctx.search_begin(db, k=3, want_scores=True)
    call = Call(swg, case["batches"])
    rc, msg = call.run(bctx)
    scores, hits, _ = bctx.search_end(ticket)                # (before any assertion: a failure here leaves no ticket behind)
    assert rc == swg.SWG_ERR_STATE and "in flight" in msg, (route, rc, msg)
    assert call.untouched()
    assert np.array_equal(scores, truth)
    assert hits == sorted(((int(s), i) for i, s in enumerate(truth)), key=lambda h: (-h[0], h[1]))[:3]
    _fill(swg, bctx, case, (route, "behind the search"))
    db.close()


def test_arguments(swg, bctx):
    case = bc.shape_matrix()
    _set(bctx, case)
    lib = swg.lib
    four = [b for b in case["batches"] if b[1] == 16][:4]
    assert len(four) == 4
    # nothing to do
    assert lib.swg_fill_batches16(bctx.handle, None, 0, None) == swg.SWG_OK
    call = Call(swg, four)
    assert call.run(bctx, n=0)[0] == swg.SWG_OK and call.untouched()
    empty = Call(swg, [(a, 0) for a, _ in four])                       # batches, but no live lane in any
    rc, msg = empty.run(bctx)
    assert rc == swg.SWG_OK and empty.untouched(), (rc, msg)
    # NULL batches
    secs = C.c_double(0)
    assert lib.swg_fill_batches16(bctx.handle, None, 3, C.byref(secs)) == swg.SWG_ERR_ARG
    assert b"NULL" in lib.swg_last_error(bctx.handle)
    # a bad batch, named by its index, and nothing written for any batch
    for field, value in (("db_idx_t", None), ("max_scores", None), ("vector_size", 17), ("max_len", 0)):
        call = Call(swg, four)
        setattr(call.arr[2], field, value)
        rc, msg = call.run(bctx)
        assert rc == swg.SWG_ERR_ARG and "bad batch 2" in msg, (field, rc, msg)
        assert call.untouched(), field
    # fill_seconds is optional
    call = Call(swg, four)
    rc, msg = call.run(bctx, seconds=False)
    assert rc == swg.SWG_OK, msg
    want = {id(a): t for (a, _), t in zip(case["batches"], bc.expected(case))}
    for i, (a, vs) in enumerate(four):
        assert np.array_equal(call.out[i], want[id(a)])
    _fill(swg, bctx, case, "behind the refusals")
