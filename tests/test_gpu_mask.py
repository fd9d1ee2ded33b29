"""GPU (-m gpu): swg_db_mask -- a masked copy of a resident database made on the device.  The host image of the copy
(Database.sequence of every sequence) and its counts (mask_info) must equal the host twin applied to the parent's
sequences, byte for byte; the DEVICE bytes are checked through what reads them: searches, the gapless prefilter,
alignment statistics, the composition kernel and views of the masked copy against a freshly packed and uploaded database
of the twin-masked sequences.  (The refusal of a parent built from 16-lane batches is not reachable here: such a database
lives inside swg_fill_batches16 and has no public handle.)"""
import numpy as np
import pytest

import mask_cases as mc
from test_gpu_parity import _reset_options

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _options(ctx):
    _reset_options(ctx)
    ctx.set_option("autotune", 0)
    yield
    _reset_options(ctx)
    ctx.set_option("autotune", 1)
    ctx.set_option("side_readout", 1)


@pytest.fixture(scope="module")
def structural(swg, ctx):
    cases = mc.structural_cases()
    names = sorted(cases)
    seqs = [cases[n] for n in names]
    flat, off = mc.flat_of(seqs)
    parent = swg.Database(flat, off).upload(ctx)
    yield dict(names=names, seqs=seqs, flat=flat, off=off, parent=parent)
    parent.close()


def _twin(swg, seqs, p):
    """-> (masked sequences, counts as mask_info gives them) by the host twin."""
    out, res, nseq, segs = [], 0, 0, 0
    for s in seqs:
        m, k = swg.seg_mask(s, want_segments=True, **p)
        out.append(mc.apply_mask(s, m, p["replace"]))
        res += int(m.sum())
        nseq += bool(m.any())
        segs += k
    return out, {"residues_masked": res, "sequences_masked": nseq, "segments": segs}


def _check_against_twin(swg, masked, seqs, names, p):
    want, counts = _twin(swg, seqs, p)
    for i, w in enumerate(want):
        got = masked.sequence(i)
        assert np.array_equal(got, w), (names[i], len(w), int((got != w).sum()), np.flatnonzero(got != w)[:8])
    info = masked.mask_info()
    assert {k: info[k] for k in counts} == counts
    assert (info["window"], info["replace"], info["trigger"], info["extend"]) == (p["window"], p["replace"], p["trigger"], p["extend"])
    assert info["kernel_ms"] > 0 and info["host_image_ms"] > 0
    return want


@pytest.mark.parametrize("pname", sorted(mc.PARAM_SETS))
def test_masked_copy_equals_the_twin(swg, ctx, structural, pname):
    p = mc.PARAM_SETS[pname]
    masked = structural["parent"].mask(ctx, **p)
    assert (masked.count, masked.total_count, masked.residues) == (structural["parent"].count, structural["parent"].total_count,
                                                                   structural["parent"].residues)
    assert np.array_equal(masked.order(), structural["parent"].order())
    _check_against_twin(swg, masked, structural["seqs"], structural["names"], p)
    masked.close()


def _query_and_scoring(swg, ctx, rng):
    sc = swg.load_scoring("BLOSUM62", -11, -1)
    ctx.set_scoring(sc.table(), -11, -1)
    q = np.concatenate([mc._iid(rng, 60), mc.homopolymer(20), mc.middle(30), mc._iid(rng, 40)]).astype(np.int8)
    ctx.set_query(q)
    return q


def _all_searches(ctx, db, k=12):
    """What reads the device bytes: the gapped search on the f16 and on the int16 cells, the gapless prefilter, the
    alignment statistics of the top hits."""
    out = {}
    for f16 in (1, 0):
        ctx.set_option("f16", f16)
        scores, hits, st = ctx.search(db, want_scores=True, k=k)
        out["scores_f16_%d" % f16] = scores.tolist()
        out["hits_f16_%d" % f16] = hits
        out["form_%d" % f16] = st["cell_form"]
    ctx.set_option("f16", 1)
    gs, gh, _ = ctx.search_gapless(db, want_scores=True, k=k)
    out["gapless"] = (gs.tolist(), gh)
    out["stats"] = ctx.align_stats(db, [h for h in out["hits_f16_1"] if h[0] > 0])  # (an empty sequence has no alignment)
    return out


def test_device_bytes_through_searches_composition_and_views(swg, ctx, structural):
    p = mc.DEFAULT
    q = _query_and_scoring(swg, ctx, np.random.default_rng(11))
    masked = structural["parent"].mask(ctx, **p)
    want, _ = _twin(swg, structural["seqs"], p)
    wflat, woff = mc.flat_of(want)
    fresh = swg.Database(wflat, woff).upload(ctx)
    a, b = _all_searches(ctx, masked), _all_searches(ctx, fresh)
    assert a["form_1"] != a["form_0"]                       # two cell routes did run
    assert a == b
    assert max(a["scores_f16_1"]) > 0
    comp = masked.composition(ctx)
    assert np.array_equal(comp, np.bincount(wflat[:int(woff[-1])].astype(np.int64), minlength=32).astype(np.uint64))
    # a view of the masked copy against the same view of the fresh database
    sel = np.arange(0, len(want), 3, dtype=np.uint32)
    va, vb = masked.view(ctx, sel), fresh.view(ctx, sel)
    assert _all_searches(ctx, va) == _all_searches(ctx, vb)
    assert np.array_equal(va.composition(ctx), vb.composition(ctx))
    for i in sel[:10]:
        assert np.array_equal(va.sequence(int(i)), want[int(i)])
    for d in (va, vb, fresh, masked):
        d.close()


def test_save_load_round_trip(swg, ctx, structural, tmp_path):
    p = mc.PARAM_SETS["replace_A"]
    _query_and_scoring(swg, ctx, np.random.default_rng(12))
    masked = structural["parent"].mask(ctx, **p)
    path = str(tmp_path / "masked.swg")
    masked.save(path)
    loaded = swg.Database(path=path)
    want, _ = _twin(swg, structural["seqs"], p)
    for i, w in enumerate(want):
        assert np.array_equal(loaded.sequence(i), w)
    with pytest.raises(swg.SwgError) as e:
        loaded.mask_info()                                    # a file holds an ordinary database
    assert e.value.code == swg.SWG_ERR_STATE
    loaded.upload(ctx)
    assert ctx.search(loaded, True, 10)[:2][0].tolist() == ctx.search(masked, True, 10)[:2][0].tolist()
    loaded.close()
    masked.close()


def test_independence_of_parent_and_copy(swg, ctx, structural):
    _query_and_scoring(swg, ctx, np.random.default_rng(13))
    parent = swg.Database(structural["flat"], structural["off"]).upload(ctx)
    before, hits_before, st_before = ctx.search(parent, True, 10)
    m1 = parent.mask(ctx)
    m2 = parent.mask(ctx)
    after, hits_after, st_after = ctx.search(parent, True, 10)
    assert np.array_equal(before, after) and hits_before == hits_after
    for f in ("engine", "cell_form", "cols_per_wave", "group_lanes", "waves", "passes"):
        assert st_before[f] == st_after[f]
    for i in range(parent.total_count):                      # the parent's host image too
        assert np.array_equal(parent.sequence(i), structural["seqs"][i])
    s1 = ctx.search(m1, True, 10)
    for i in range(m1.total_count):                          # two calls: the same bytes
        assert np.array_equal(m1.sequence(i), m2.sequence(i))
    assert np.array_equal(m1.composition(ctx), m2.composition(ctx))
    i1, i2 = m1.mask_info(), m2.mask_info()
    assert all(i1[k] == i2[k] for k in ("residues_masked", "sequences_masked", "segments"))
    parent.close()
    s2 = ctx.search(m1, True, 10)                            # the copy outlives its parent
    assert np.array_equal(s1[0], s2[0]) and s1[1] == s2[1]
    assert np.array_equal(ctx.search(m2, True, 10)[0], s1[0])
    m1.close()
    assert np.array_equal(ctx.search(m2, True, 10)[0], s1[0])
    m2.close()


def test_refusals(swg, ctx, structural):
    parent = structural["parent"]
    view = parent.view(ctx, np.arange(5, dtype=np.uint32))
    with pytest.raises(swg.SwgError) as e:
        view.mask(ctx)
    assert e.value.code == swg.SWG_ERR_ARG and "mask the root" in str(e.value) and "view of the result" in str(e.value)
    view.close()
    host_only = swg.Database(structural["flat"], structural["off"])
    with pytest.raises(swg.SwgError) as e:
        host_only.mask(ctx)
    assert e.value.code == swg.SWG_ERR_STATE
    host_only.close()
    for bad in (dict(window=3), dict(window=65), dict(trigger=3.0, extend=2.5), dict(trigger=-1.0), dict(replace=0), dict(replace=32)):
        with pytest.raises(swg.SwgError) as e:
            parent.mask(ctx, **bad)
        assert e.value.code == swg.SWG_ERR_ARG, bad
    with pytest.raises(swg.SwgError) as e:
        parent.mask_info()
    assert e.value.code == swg.SWG_ERR_STATE
    masked = parent.mask(ctx)
    again = masked.mask(ctx, window=4, trigger=0.9, extend=1.6)  # a masked copy is a root: it can be masked again
    assert again.mask_info()["window"] == 4
    again.close()
    masked.close()


def test_a_failed_allocation_leaves_nothing_behind(swg, ctx, structural):
    """Each of the call's seven device allocations in turn finds no memory: SWG_ERR_NOMEM, no database, and both the
    parent and the next call are whole."""
    _query_and_scoring(swg, ctx, np.random.default_rng(14))
    parent = structural["parent"]
    before = ctx.search(parent, True, 10)
    for n in range(1, 8):
        swg.debug_mask_fail_alloc(n)
        with pytest.raises(swg.SwgError) as e:
            parent.mask(ctx)
        assert e.value.code == swg.SWG_ERR_NOMEM, n
    swg.debug_mask_fail_alloc(8)                               # beyond the last allocation: the call succeeds and disarms the hook
    masked = parent.mask(ctx)
    _check_against_twin(swg, masked, structural["seqs"], structural["names"], mc.DEFAULT)
    again = parent.mask(ctx)
    assert again.mask_info()["residues_masked"] == masked.mask_info()["residues_masked"]
    after = ctx.search(parent, True, 10)
    assert np.array_equal(before[0], after[0]) and before[1] == after[1]
    again.close()
    masked.close()


def test_empty_and_tiny_databases(swg, ctx):
    for seqs in ([mc.homopolymer(0)], [mc.homopolymer(11)], [mc.homopolymer(12)], [mc.homopolymer(3)] * 129 + [mc.homopolymer(40)]):
        flat, off = mc.flat_of(seqs)
        db = swg.Database(flat, off).upload(ctx)
        m = db.mask(ctx)
        _check_against_twin(swg, m, seqs, ["%d" % len(s) for s in seqs], mc.DEFAULT)
        m.close()
        db.close()


def test_end_to_end(swg, ctx, orc):
    """Unmasked, decoys that share only a Q/E-rich run with the query take most of the top 5; on the masked copy the top
    5 is exactly the relatives.  Both lists are the oracle's (test_mask_host.py pins the seed on the CPU)."""
    c = mc.end_to_end()
    sc = swg.load_scoring("BLOSUM62", -11, -1)
    ctx.set_scoring(sc.table(), -11, -1)
    ctx.set_query(c["query"])
    flat, off = mc.flat_of(c["seqs"])
    db = swg.Database(flat, off).upload(ctx)
    plain = orc.score_db(c["query"], flat, off, sc.table(), -11, -1)
    masked_flat, counts = swg.seg_mask_flat(flat, off)
    want = orc.score_db(c["query"], masked_flat, off, sc.table(), -11, -1)
    _, hits, _ = ctx.search(db, False, 5)
    assert hits == mc.top_hits(plain, 5)
    assert sum(i in c["decoys"] for _, i in hits) >= 3
    masked = db.mask(ctx)
    scores, mhits, _ = ctx.search(masked, True, 5)
    assert np.array_equal(scores, want)
    assert mhits == mc.top_hits(want, 5)
    assert {i for _, i in mhits} == c["relatives"]
    info = masked.mask_info()
    assert {k: info[k] for k in counts} == counts
    # soft masking: the hits of the masked copy aligned against the parent carry the parent's scores
    stats = ctx.align_stats(db, mhits)
    assert [s["score"] for s in stats] == [int(plain[i]) for _, i in mhits]
    masked.close()
    db.close()
