"""GPU (-m gpu): swg_db_translate -- the six-frame translation of a resident nucleotide database, made on the device.
The translation must be indistinguishable from swg_db_pack + swg_db_upload of the host twin's frames given in index order
6 i + g: the host image (order, counts, every sequence byte for byte) and the counts against the string model of
translate_cases.py, and the DEVICE bytes through what reads them -- searches on both cell forms, the gapless search,
search_above, alignments with paths, alignment statistics, the composition kernel and views -- against the freshly packed
twin database, compared with ==."""
import numpy as np
import pytest

import translate_cases as tc
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
    """The structural database with the six planted records in front (record i holds the query in frame i)."""
    plant = tc.planted()
    cases = tc.structural_cases(swg.TRANSLATE_TILE_CODONS)
    names = ["plant_%d" % i for i in range(6)] + sorted(cases)
    seqs = plant["records"] + [cases[n] for n in sorted(cases)]
    flat, off = tc.flat_of(seqs)
    parent = swg.Database(flat, off).upload(ctx)
    assert (6 * len(seqs)) % 128 != 0                        # the translation's last bin has empty slots
    yield dict(names=names, seqs=seqs, flat=flat, off=off, parent=parent, plant=plant)
    parent.close()


def _twin_frames(swg, seqs, code=1, unknown=24):
    """The host twin's frames in index order 6 i + g."""
    out = []
    for s in seqs:
        out.extend(swg.translate_seq(tc.indices(s), code=code, unknown=unknown))
    return out


def _fresh(swg, ctx, frames):
    flat, off = tc.flat_of(frames)
    return swg.Database(flat, off).upload(ctx), flat, off


CODES = {"code1": (1, tc.TABLES[1]), "code4": (4, tc.TABLES[4]), "custom": (None, tc.CUSTOM)}


@pytest.mark.parametrize("name", sorted(CODES))
def test_translation_equals_the_packed_twin(swg, ctx, structural, name):
    ncbi, letters = CODES[name]
    code = ncbi if ncbi is not None else tc.table_indices(letters)
    tr = structural["parent"].translate(ctx, code=code)
    frames = _twin_frames(swg, structural["seqs"], code=code)
    fresh, _, _ = _fresh(swg, ctx, frames)
    assert (tr.count, tr.total_count, tr.residues) == (fresh.count, fresh.total_count, fresh.residues)
    assert tr.total_count == 6 * structural["parent"].total_count
    assert np.array_equal(tr.order(), fresh.order())
    assert tr.packed_bytes == fresh.packed_bytes
    for j, want in enumerate(frames):
        got = tr.sequence(j)
        assert np.array_equal(got, want), (structural["names"][j // 6], j % 6, len(want))
        model = tc.model(structural["seqs"][j // 6], letters)[j % 6]
        assert np.array_equal(got, tc.indices(model)), (structural["names"][j // 6], j % 6)
    info = tr.translate_info()
    assert (info["codons"], info["stops"], info["unknown_codons"]) == tc.model_counts(structural["seqs"], letters)
    assert info["codons"] == tr.residues and info["kernel_ms"] > 0 and info["host_image_ms"] > 0
    assert np.array_equal(info["codon"], tc.table_indices(letters)) and info["unknown"] == 24
    fresh.close()
    tr.close()


def _scoring_and_query(swg, ctx, plant):
    sc = swg.load_scoring("BLOSUM62", -11, -1)
    ctx.set_scoring(sc.table(), -11, -1)
    q = tc.indices(plant["query"])
    ctx.set_query(q)
    return q


def _all_reads(ctx, db, k=12):
    """What reads the device bytes."""
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
    out["above"] = ctx.search_above(db, 40)[:2]
    top = [h for h in out["hits_f16_1"] if h[0] > 0]
    out["align"] = ctx.align_hits(db, top, want_ops=True)
    out["stats"] = ctx.align_stats(db, top)
    return out


def test_device_bytes_through_what_reads_them(swg, ctx, structural):
    plant = structural["plant"]
    _scoring_and_query(swg, ctx, plant)
    tr = structural["parent"].translate(ctx)
    frames = _twin_frames(swg, structural["seqs"])
    fresh, wflat, woff = _fresh(swg, ctx, frames)
    a, b = _all_reads(ctx, tr), _all_reads(ctx, fresh)
    assert a["form_1"] != a["form_0"]                       # two cell routes did run
    assert a == b
    comp = tr.composition(ctx)
    assert np.array_equal(comp, np.bincount(wflat[:int(woff[-1])].astype(np.int64), minlength=32).astype(np.uint64))
    # the planted records: the top six hits are exactly 6 i + f, and their coordinates are the planted nucleotides
    want = sorted(6 * rec + frame for rec, frame, _, _ in plant["plants"])
    top6 = a["hits_f16_1"][:6]
    assert sorted(i for _, i in top6) == want
    assert len({s for s, _ in top6}) == 1 and top6[0][0] > a["hits_f16_1"][6][0]
    by_index = {al["index"]: al for al in a["align"]}
    for rec, frame, nb, ne in plant["plants"]:
        assert swg.translate_hit(6 * rec + frame) == (rec, frame)
        al = by_index[6 * rec + frame]
        assert (al["q_begin"], al["q_end"]) == (0, len(plant["query"])) and set(al["ops"]) == {"M"}
        assert swg.translate_coords(frame, len(structural["seqs"][rec]), al["d_begin"], al["d_end"]) == (nb, ne)
    # a view of about 40 indices of each
    sel = np.concatenate([np.array(want, dtype=np.uint32), np.arange(7, 6 * len(structural["seqs"]), 41, dtype=np.uint32)])
    va, vb = tr.view(ctx, sel), fresh.view(ctx, sel)
    assert _all_reads(ctx, va) == _all_reads(ctx, vb)
    assert np.array_equal(va.composition(ctx), vb.composition(ctx))
    for d in (va, vb, fresh, tr):
        d.close()


def test_masks_compose_with_translations(swg, ctx, structural):
    _scoring_and_query(swg, ctx, structural["plant"])
    # a translation of a masked nucleotide root
    p = dict(window=12, trigger=2.2, extend=2.5, replace=14)                  # N: a masked nucleotide is no base
    masked = structural["parent"].mask(ctx, **p)
    tm = masked.translate(ctx)
    nt_masked = [np.where(swg.seg_mask(tc.indices(s), **p), 14, tc.indices(s)).astype(np.int8) for s in structural["seqs"]]
    frames = []
    for s in nt_masked:
        frames.extend(swg.translate_seq(s))
    for j, want in enumerate(frames):
        assert np.array_equal(tm.sequence(j), want), j
    fresh, _, _ = _fresh(swg, ctx, frames)
    assert ctx.search(tm, True, 10)[0].tolist() == ctx.search(fresh, True, 10)[0].tolist()
    for d in (fresh, tm, masked):
        d.close()
    # a mask of a translation
    tr = structural["parent"].translate(ctx)
    mt = tr.mask(ctx)
    frames = _twin_frames(swg, structural["seqs"])
    want = [np.where(swg.seg_mask(f), 24, f).astype(np.int8) for f in frames]
    for j, w in enumerate(want):
        assert np.array_equal(mt.sequence(j), w), j
    fresh, _, _ = _fresh(swg, ctx, want)
    assert ctx.search(mt, True, 10)[0].tolist() == ctx.search(fresh, True, 10)[0].tolist()
    assert mt.mask_info()["residues_masked"] == sum(int(swg.seg_mask(f).sum()) for f in frames)
    with pytest.raises(swg.SwgError) as e:
        mt.translate_info()                                   # the masked copy is swg_db_mask's, not swg_db_translate's
    assert e.value.code == swg.SWG_ERR_STATE
    for d in (fresh, mt, tr):
        d.close()


def test_refusals(swg, ctx, structural):
    parent = structural["parent"]
    view = parent.view(ctx, np.arange(5, dtype=np.uint32))
    with pytest.raises(swg.SwgError) as e:
        view.translate(ctx)
    assert e.value.code == swg.SWG_ERR_ARG and "swg_db_translate" in str(e.value) and "translate the root" in str(e.value)
    view.close()
    host_only = swg.Database(structural["flat"], structural["off"])
    with pytest.raises(swg.SwgError) as e:
        host_only.translate(ctx)
    assert e.value.code == swg.SWG_ERR_STATE and "swg_db_translate" in str(e.value)
    host_only.close()
    for entry in (0, 32):
        t = swg.codon_table(1).copy()
        t[40] = entry
        with pytest.raises(swg.SwgError) as e:
            parent.translate(ctx, code=t)
        assert e.value.code == swg.SWG_ERR_ARG and "swg_db_translate" in str(e.value)
    with pytest.raises(swg.SwgError) as e:
        parent.translate(ctx, unknown=0)
    assert e.value.code == swg.SWG_ERR_ARG and "swg_db_translate" in str(e.value)
    with pytest.raises(swg.SwgError) as e:
        parent.translate_info()
    assert e.value.code == swg.SWG_ERR_STATE


def test_save_load_and_a_shard(swg, ctx, structural, tmp_path):
    tr = structural["parent"].translate(ctx)
    path = str(tmp_path / "translated.swg")
    tr.save(path)
    loaded = swg.Database(path=path)
    for j in range(0, tr.total_count, 17):
        assert np.array_equal(loaded.sequence(j), tr.sequence(j))
    with pytest.raises(swg.SwgError) as e:
        loaded.translate_info()                               # a file holds an ordinary database
    assert e.value.code == swg.SWG_ERR_STATE
    loaded.close()
    tr.close()
    # a shard is a root: its frames keep 6 x the global index + g, in the order of a shard packed from them
    n = len(structural["seqs"])
    keep = np.arange(1, n, 3)
    sflat, soff = tc.flat_of([structural["seqs"][i] for i in keep])
    shard = swg.Database(sflat, soff, index=keep.astype(np.uint32), n_total=n).upload(ctx)
    ts = shard.translate(ctx)
    frames, index = [], []
    for i in keep:
        frames.extend(swg.translate_seq(tc.indices(structural["seqs"][i])))
        index.extend(6 * int(i) + g for g in range(6))
    fflat, foff = tc.flat_of(frames)
    want = swg.Database(fflat, foff, index=np.array(index, dtype=np.uint32), n_total=6 * n)
    assert (ts.count, ts.total_count, ts.residues) == (want.count, 6 * n, want.residues)
    assert np.array_equal(ts.order(), want.order())
    for j, f in zip(index[::7], frames[::7]):
        assert np.array_equal(ts.sequence(j), f)
    for d in (want, ts, shard):
        d.close()


def test_the_translation_outlives_its_parent(swg, ctx, structural):
    _scoring_and_query(swg, ctx, structural["plant"])
    parent = swg.Database(structural["flat"], structural["off"]).upload(ctx)
    tr = parent.translate(ctx)
    before = ctx.search(tr, True, 10)
    parent.close()
    after = ctx.search(tr, True, 10)
    assert np.array_equal(before[0], after[0]) and before[1] == after[1]
    assert ctx.align_stats(tr, before[1][:6]) == ctx.align_stats(tr, after[1][:6])
    tr.close()


def test_empty_and_tiny_databases(swg, ctx):
    T = swg.TRANSLATE_TILE_CODONS
    for seqs in ([""], ["AC"], ["ACG"], ["ACGTN"] * 129 + ["A" * (3 * T + 1)], ["ACGT" * (6 * T)]):
        flat, off = tc.flat_of(seqs)
        db = swg.Database(flat, off).upload(ctx)
        tr = db.translate(ctx)
        frames = _twin_frames(swg, seqs)
        assert tr.total_count == 6 * len(seqs) and tr.residues == sum(f.size for f in frames)
        for j, want in enumerate(frames):
            assert np.array_equal(tr.sequence(j), want), (len(seqs), j)
        tr.close()
        db.close()
