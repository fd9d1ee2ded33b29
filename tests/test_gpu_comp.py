"""GPU: composition-based score adjustment of reported hits (swg_comp_adjust / _multi / _multi_pssm).

Every case of comp_cases.py through the device call, every field against the host twin (the integers equal, lambda_hit
within 1e-9 relative) -- the twin is held against the numpy model on the CPU (test_comp_host.py).  At F = 1 the fill is
tied to the int32 oracle independently of the twin, with the table built from the DEVICE's ratio16.  Then the three calls
against each other, the context's own query, views, a masked root and a shard pair, which instantiation ran, the host
route, the option's range and the refusals."""
import numpy as np
import pytest

import comp_cases as cc
import comp_model as cm
import pssm_build_cases as pc

pytestmark = pytest.mark.gpu
INT_FIELDS = ("adj_score", "scaled_score", "ratio16", "status")
REL = 1e-9


@pytest.fixture(scope="module")
def cctx(swg):
    c = swg.Context(0)
    yield c
    c.close()


def _hits(ix):
    return [(0, int(i)) for i in ix]


def _set(cctx, c, F=None):
    cctx.set_scoring(c["sub"], c["gap_open"], c["gap_extend"])
    cctx.set_option("comp_scale", c["F"] if F is None else F)
    if c["query"] is not None:
        cctx.set_query(c["query"])
    else:
        cctx.set_query_pssm(c["pssm"])


def _device(swg, cctx, c, F=None):
    flat, off = cc.database(c)
    db = swg.Database(flat, off).upload(cctx)
    try:
        _set(cctx, c, F)
        return cctx.comp_adjust(db, _hits(c["hits"]), freq=c["freq"]) + (cctx.debug_comp_last(),)
    finally:
        db.close()


def _twin(swg, c, i, F=None):
    return swg.comp_adjust_host(c["sub"], c["gap_open"], c["gap_extend"], c["seqs"][i], query=c["query"], pssm=c["pssm"], freq=c["freq"],
                                scale=c["F"] if F is None else F)


def _same(got, want, what):
    for f in INT_FIELDS:
        assert int(got[f]) == int(want[f]), (what, f, got, want)
    a, b = float(got["lambda_hit"]), float(want["lambda_hit"])
    assert abs(a - b) <= REL * abs(b), (what, a, b)


def _group(c):
    n = c["name"]
    return "inst" if "G" in c else "limit" if "over" in c else "pssm" if n.startswith("pssm") else "gaps" if n.startswith("gaps") else "bias"


@pytest.mark.parametrize("group", ["bias", "gaps", "pssm", "inst", "limit"])
def test_every_case_equals_the_twin(swg, cctx, group):
    n = 0
    for c in cc.all_cases():
        if _group(c) != group:
            continue
        recs, lam_std, last = _device(swg, cctx, c)
        assert len(recs) == len(c["hits"])
        for slot, i in enumerate(c["hits"]):
            want, want_std = _twin(swg, c, i)
            _same(recs[slot], want, (c["name"], slot, i))
            assert abs(lam_std - want_std) <= REL * abs(want_std), (c["name"], lam_std, want_std)
        # which instantiation ran, and what went to the host route
        over = c.get("over", False)
        cls = cc.class_of(cc.lq_of(c))
        want_pairs = {gk: (len(c["hits"]) if not over and k == cls else 0) for k, gk in enumerate(cc.CLASSES)}
        assert last["class_pairs"] == want_pairs, (c["name"], last)
        assert (last["kernel_pairs"], last["host_pairs"], last["launches"]) == ((0, len(c["hits"]), 0) if over else (len(c["hits"]), 0, 1)), (c["name"], last)
        assert (last["column_limit"], last["scale"]) == (cc.COLS, c["F"])
        if "G" in c:
            assert cc.CLASSES[cls] == (c["G"], c["K"])
        n += 1
    assert n >= 4


def test_scale_one_is_the_oracle_under_the_devices_table(swg, cctx, orc):
    """F = 1: scaled_score against the int32 oracle under T o sub, T from the DEVICE's ratio16 -- index queries and the
    31-column PSSMs, with no twin in between."""
    n = adjusted = 0
    for c in cc.all_cases():
        form = (c["query"], c["sub"]) if c["query"] is not None else c.get("index_form")
        if form is None or c.get("over") or (cc.lq_of(c) > 400 and c["pssm"] is not None):
            continue
        recs, _, _ = _device(swg, cctx, c, F=1)
        for slot, i in enumerate(c["hits"]):
            T = cm.table(1, int(recs[slot]["ratio16"]))
            tsub = T[np.asarray(form[1], dtype=np.int64) + 128].astype(np.int8)
            want = orc.pair(form[0], c["seqs"][i], tsub, c["gap_open"], c["gap_extend"])
            assert int(recs[slot]["scaled_score"]) == int(recs[slot]["adj_score"]) == want, (c["name"], slot)
            n += 1
            adjusted += int(recs[slot]["ratio16"]) < 65536
    assert n >= 300 and adjusted >= 100


@pytest.fixture(scope="module")
def world(swg, cctx):
    """One database of biased, unbiased and short subjects, and queries of four classes and one beyond the limit."""
    rng = np.random.default_rng(77)
    seqs = [cc.shuffled_composition(rng, 120 + 9 * i, cc.QEK, 0.05 * (i % 8)) for i in range(24)]
    seqs += [cc.background_seq(rng, n) for n in (1, 2, 3, 19, 67, 400)] + [np.full(25, cc.X, dtype=np.int8)]
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    flat = np.concatenate(seqs).astype(np.int8)
    queries = [cc.qek_query()] + [cc.background_seq(rng, n) for n in (7, 64, 65, 300, 1100, cc.COLS + 5)]
    db = swg.Database(flat, off).upload(cctx)
    yield dict(seqs=seqs, flat=flat, off=off, queries=queries, db=db, b62=pc.table("BLOSUM62"))
    db.close()


def _rows(world):
    n = len(world["seqs"])
    rng = np.random.default_rng(5)
    rows = [sorted(rng.choice(n, size=5 + 3 * i, replace=False).tolist()) for i in range(len(world["queries"]))]
    rows[1] = rows[1] + rows[1][:2]          # a repeat
    rows[3] = []                              # a query without hits
    return rows


def test_the_three_calls_agree_and_leave_the_query_alone(swg, cctx, world):
    b62, db, queries = world["b62"], world["db"], world["queries"]
    rows = _rows(world)
    cctx.set_scoring(b62, -11, -1)
    cctx.set_option("comp_scale", 32)
    sentinel = cc.background_seq(np.random.default_rng(9), 33)
    cctx.set_query(sentinel)
    multi, lam_m = cctx.comp_adjust_multi(db, queries, [_hits(r) for r in rows])
    last = cctx.debug_comp_last()
    n_over = len(rows[-1])
    assert last["host_pairs"] == n_over > 0 and last["kernel_pairs"] == sum(len(r) for r in rows) - n_over
    assert last["launches"] == len({cc.class_of(len(q)) for q, r in zip(queries[:-1], rows) if r})
    multi_p, lam_p = cctx.comp_adjust_multi_pssm(db, [b62[q.astype(np.int64)] for q in queries], [_hits(r) for r in rows])
    assert np.array_equal(lam_m, lam_p) and all(a.tobytes() == b.tobytes() for a, b in zip(multi, multi_p))
    # the context's own query is the sentinel still: its single call is the twin's answer for the sentinel
    single, lam_s = cctx.comp_adjust(db, _hits(rows[0]))
    for slot, i in enumerate(rows[0]):
        want, want_std = swg.comp_adjust_host(b62, -11, -1, world["seqs"][i], query=sentinel)
        _same(single[slot], want, ("sentinel", i))
        assert abs(lam_s - want_std) <= REL * want_std
    # row i of the batch is the single call with query i set, byte for byte, in both forms
    for qi, (q, r) in enumerate(zip(queries, rows)):
        cctx.set_query(q)
        one, lam1 = cctx.comp_adjust(db, _hits(r))
        assert one.tobytes() == multi[qi].tobytes() and lam1 == lam_m[qi], qi
        cctx.set_query_pssm(b62[q.astype(np.int64)])
        onep, lam1p = cctx.comp_adjust(db, _hits(r))
        assert onep.tobytes() == multi[qi].tobytes() and lam1p == lam_m[qi], qi
        for slot, i in enumerate(r):
            want, _ = swg.comp_adjust_host(b62, -11, -1, world["seqs"][i], query=q)
            _same(one[slot], want, (qi, i))
    # two identical calls return identical bytes
    again, lam_a = cctx.comp_adjust_multi(db, queries, [_hits(r) for r in rows])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(multi, again)) and np.array_equal(lam_m, lam_a)


def test_few_lane_groups_take_many_pairs_each(swg, cctx, world):
    """Option bounds_groups bounds the fill's lane groups as it bounds the bounds kernel's: one group then takes every pair
    of its launch in turn, each under the table of its own pair."""
    b62, db = world["b62"], world["db"]
    cctx.set_scoring(b62, -11, -1)
    cctx.set_option("comp_scale", 32)
    hits = _hits(list(range(len(world["seqs"]))) * 2)
    want, ratios = {}, set()
    try:
        for groups in (0, 1, 3):
            cctx.set_option("bounds_groups", groups)
            for q in (world["queries"][0], world["queries"][4]):
                for pssm in (False, True):
                    if pssm:
                        cctx.set_query_pssm(b62[q.astype(np.int64)])
                    else:
                        cctx.set_query(q)
                    recs, _ = cctx.comp_adjust(db, hits)
                    assert want.setdefault(len(q), recs.tobytes()) == recs.tobytes(), (groups, len(q), pssm)
                    ratios |= {int(r["ratio16"]) for r in recs}
    finally:
        cctx.set_option("bounds_groups", 0)
    assert len(ratios) > 8 and min(ratios) == 32768           # (many different tables met one lane group)


def test_views_a_masked_root_and_shards(swg, cctx, world):
    b62, db, seqs = world["b62"], world["db"], world["seqs"]
    n = len(seqs)
    cctx.set_scoring(b62, -11, -1)
    cctx.set_option("comp_scale", 32)
    q = world["queries"][0]
    cctx.set_query(q)
    hits = _hits(range(n))
    root, lam = cctx.comp_adjust(db, hits)
    assert (root["status"] != swg.COMP_UNWRITTEN).all()
    # a view: the records of the hits it holds, the others untouched
    held = [1, 4, 5, 20, n - 1]
    view = db.view(cctx, held)
    got, lam_v = cctx.comp_adjust(view, hits)
    assert lam_v == lam
    for i in range(n):
        if i in held:
            assert got[i].tobytes() == root[i].tobytes(), i
        else:
            assert got[i]["status"] == swg.COMP_UNWRITTEN and got[i]["scaled_score"] == 0, i
    with pytest.raises(swg.SwgError) as e:                              # an index outside the whole database
        cctx.comp_adjust(view, _hits([n]))
    assert e.value.code == swg.SWG_ERR_ARG
    view.close()
    # a masked root: the composition and the score of the bytes it holds
    masked = db.mask(cctx)
    got, _ = cctx.comp_adjust(masked, hits)
    changed = 0
    for i in range(n):
        m = masked.sequence(i)
        want, _ = swg.comp_adjust_host(b62, -11, -1, m, query=q)
        _same(got[i], want, ("masked", i))
        if np.array_equal(m, seqs[i]):
            assert got[i].tobytes() == root[i].tobytes(), i
        else:
            changed += 1
    masked.close()
    # a shard pair: every hit written exactly once across the two handles
    shards = swg.Database.pack_shards(world["flat"], world["off"], 2)
    written = np.zeros(n, dtype=np.int64)
    for sh in shards:
        sh.upload(cctx)
        got, _ = cctx.comp_adjust(sh, hits)
        w = got["status"] != swg.COMP_UNWRITTEN
        written += w
        assert all(got[i].tobytes() == root[i].tobytes() for i in np.nonzero(w)[0])
        sh.close()
    assert (written == 1).all()


def test_the_option_range_and_the_refusals(swg, cctx, world):
    b62, db = world["b62"], world["db"]
    for bad in (0, -1, 65, 1 << 20):
        with pytest.raises(swg.SwgError) as e:
            cctx.set_option("comp_scale", bad)
        assert e.value.code == swg.SWG_ERR_ARG
    for ok in (1, 64, 32):
        cctx.set_option("comp_scale", ok)
    with pytest.raises(swg.SwgError) as e:
        cctx.set_option("comp_scal", 3)
    assert e.value.code == swg.SWG_ERR_ARG and "unknown key" in str(e.value)
    cctx.set_scoring(b62, -11, -1)
    cctx.set_query(world["queries"][1])
    # no hits: nothing to do, and lambda_std still answered
    recs, lam = cctx.comp_adjust(db, [])
    assert len(recs) == 0 and lam > 0
    for bad in (np.full(32, np.nan), -pc.builtin_freq(), np.zeros(32), np.r_[1.0, pc.builtin_freq()[1:]]):
        with pytest.raises(swg.SwgError) as e:
            cctx.comp_adjust(db, _hits([0]), freq=bad)
        assert e.value.code == swg.SWG_ERR_ARG
    # a database that is not resident; a fresh context without scoring or query
    host_only = swg.Database(world["flat"], world["off"])
    with pytest.raises(swg.SwgError) as e:
        cctx.comp_adjust(host_only, _hits([0]))
    assert e.value.code == swg.SWG_ERR_STATE
    host_only.close()
    fresh = swg.Context(0)
    try:
        with pytest.raises(swg.SwgError) as e:
            fresh.comp_adjust(db, _hits([0]))
        assert e.value.code == swg.SWG_ERR_STATE
        fresh.set_scoring(b62, -11, -1)
        with pytest.raises(swg.SwgError) as e:
            fresh.comp_adjust(db, _hits([0]))
        assert e.value.code == swg.SWG_ERR_STATE
    finally:
        fresh.close()
    # a search in flight on the context
    ticket = cctx.search_begin(db, k=3)
    try:
        with pytest.raises(swg.SwgError) as e:
            cctx.comp_adjust(db, _hits([0]))
        assert e.value.code == swg.SWG_ERR_STATE and "in flight" in str(e.value)
    finally:
        cctx.search_end(ticket)
    # a pair whose int32 cells could wrap, refused before anything runs
    cctx.set_scoring(b62, 30000, 2000)
    cctx.set_option("comp_scale", 64)
    cctx.set_query(world["queries"][5])            # (1100 + 400 residues) x 64 x 32000 >= 2^31
    with pytest.raises(swg.SwgError) as e:
        cctx.comp_adjust(db, _hits([len(world["seqs"]) - 2]))
    assert e.value.code == swg.SWG_ERR_ARG
    cctx.set_option("comp_scale", 32)
    cctx.set_scoring(b62, -11, -1)


def test_comp_scale_moves_nothing_but_its_own_call(swg, cctx, world):
    """What the call-order tables (tests/call_order_cases.py) ask of every option, for this family's own: the option is read
    inside one swg_comp_adjust* call and nothing is remembered.  While comp_scale is away from its default the context's
    other calls answer as before; the call itself answers by the value of the moment; back at the default it returns the
    bytes it returned before the move."""
    b62, db, seqs = world["b62"], world["db"], world["seqs"]
    q = world["queries"][0]
    hits = _hits(range(len(seqs)))
    cctx.set_scoring(b62, -11, -1)
    cctx.set_query(q)

    def others():
        scores, top, _ = cctx.search(db, k=5)
        return scores.tobytes(), top, cctx.align_bounds(db, top), cctx.align_stats(db, top)

    cctx.set_option("comp_scale", 32)
    before, others_before = cctx.comp_adjust(db, hits), others()
    cctx.set_option("comp_scale", 7)
    assert others() == others_before
    away = cctx.comp_adjust(db, hits)
    for i in range(len(seqs)):
        want, _ = swg.comp_adjust_host(b62, -11, -1, seqs[i], query=q, scale=7)
        _same(away[0][i], want, ("scale 7", i))
    assert away[0].tobytes() != before[0].tobytes() and away[1] == before[1]
    cctx.set_option("comp_scale", 32)
    after = cctx.comp_adjust(db, hits)
    assert after[0].tobytes() == before[0].tobytes() and after[1] == before[1] and others() == others_before
    # a fresh context starts at the default
    fresh = swg.Context(0)
    try:
        fresh.set_scoring(b62, -11, -1)
        fresh.set_query(q)
        assert fresh.comp_adjust(db, hits)[0].tobytes() == before[0].tobytes() and fresh.debug_comp_last()["scale"] == 32
    finally:
        fresh.close()
