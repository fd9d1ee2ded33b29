"""CPU: low-complexity masking on the host -- the twin swg_seg_mask against the numpy restatement of the rule
(mask_cases.reference_mask, which recounts every window), proof that the case matrix holds every edge the GPU test relies
on, the integers of the rule, the refusals, swg_db_sequence, and the CPU half of the end-to-end case."""
import numpy as np
import pytest

import mask_cases as mc


@pytest.fixture(scope="module")
def cases():
    return mc.structural_cases()


@pytest.mark.parametrize("pname", sorted(mc.PARAM_SETS))
def test_twin_equals_restatement(swg, cases, pname):
    p = mc.PARAM_SETS[pname]
    for name, seq in cases.items():
        want, kept = mc.reference_mask(seq, **p)
        got, segments = swg.seg_mask(seq, want_segments=True, **p)
        assert np.array_equal(got, want), (pname, name, int(want.sum()), int(got.sum()))
        assert segments == len(kept), (pname, name)


def test_case_matrix_holds_every_edge(cases):
    flags = {n: mc.window_flags(s) for n, s in cases.items()}
    kept = {n: mc.reference_mask(s)[1] for n, s in cases.items()}
    lens = {len(s) for s in cases.values()}
    assert {0, 1, 11, 12, 13, 23, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, mc.LONG} <= lens
    assert {l % 4 for l in lens} == {0, 1, 2, 3}
    # homopolymers over a whole sequence, the long one included: one kept run, everything masked
    for n in ("homo12", "homo%d" % mc.LONG):
        assert kept[n] == [(0, len(cases[n]) - 11)] and mc.reference_mask(cases[n])[0].all()
    # a run whose only trigger is its first start / its last start, at the sequence's edge and inside it
    for n, at in (("first_trigger", "first"), ("last_trigger", "last"), ("first_trigger_in_high", "first"), ("last_trigger_in_high", "last"),
                  ("stretch5000_first", "first"), ("stretch5000_last", "last")):
        low1, low2 = flags[n]
        (b, e), = mc.runs_of(low2)
        assert np.flatnonzero(low1).tolist() == [b if at == "first" else e - 1], n
        assert kept[n] == [(b, e)]
    assert kept["stretch5000_first"][0][1] - kept["stretch5000_first"][0][0] == 5000
    # 5000 windows low at K2 with no trigger: a run, and nothing kept
    low1, low2 = flags["stretch5000_none"]
    assert mc.runs_of(low2) == [(0, 5000)] and not low1.any() and kept["stretch5000_none"] == []
    # two kept runs with exactly one window between them that is not low
    assert mc.has_one_window_gap(*flags["one_window_gap"])
    # kept runs across each boundary position and its neighbours (1024 among them)
    for p in mc.BOUNDARIES:
        for q in (p - 1, p, p + 1):
            assert any(b < q < e for b, e in kept["straddlers"]), q
    assert any(b < 1024 < e for b, e in kept["stretch5000_first"])
    # the letters X, B, Z and * occur, masked and unmasked
    for letter in (mc.X, mc.B, mc.Z, mc.STAR):
        assert (cases["xbz_star"] == letter).any()
    m = mc.reference_mask(cases["x_run"])[0]
    assert m[cases["x_run"] == mc.X].all() and m[cases["x_run"] == mc.STAR].all() and not m.all()
    # some sequence has a run low at K2 that is not kept beside one that is
    assert any(len(mc.runs_of(f[1])) > len(kept[n]) > 0 for n, f in flags.items())


def test_tables_and_thresholds(swg):
    T, t1, t2 = swg.mask_tables()
    assert (t1, t2) == (1089179, 853250)
    for W in (4, 12, 64):
        T, _, _ = swg.mask_tables(window=W, trigger=1.0, extend=1.5)
        want, _, _ = mc.tables(W, 1.0, 1.5)
        assert np.array_equal(T.astype(np.int64), want)
        c = np.arange(2, W + 1, dtype=np.float64)
        exact = c * np.log2(c) * 65536.0
        integral = exact == np.floor(exact)               # c a power of two: no rounding at all
        frac = exact - np.floor(exact)
        assert (np.abs(frac - 0.5)[~integral] > 1e-6).all(), W


@pytest.mark.parametrize("bad", [dict(window=3), dict(window=65), dict(trigger=-0.1), dict(trigger=2.6, extend=2.5), dict(replace=0),
                                 dict(replace=32), dict(extend=float("nan")), dict(trigger=float("inf"), extend=float("inf"))])
def test_parameter_refusals(swg, bad):
    with pytest.raises(swg.SwgError) as e:
        swg.seg_mask(mc.homopolymer(40), **bad)
    assert e.value.code == swg.SWG_ERR_ARG
    with pytest.raises(swg.SwgError) as e:
        swg.mask_tables(**bad)
    assert e.value.code == swg.SWG_ERR_ARG


def test_short_and_empty_sequences(swg):
    for n in (0, 1, 11):
        assert not swg.seg_mask(mc.homopolymer(n)).any()
    assert swg.seg_mask(mc.homopolymer(12)).all()
    with pytest.raises(swg.SwgError) as e:
        swg.seg_mask(np.array([1] * 11 + [40], dtype=np.int8))
    assert e.value.code == swg.SWG_ERR_RESIDUE


def test_defaults_mask_a_small_share_of_iid_sequences(swg):
    """Measured with this generator (lengths 20..400, numpy seed 1): 1773 of 85423 residues (2.08 %) in 92 of 400 sequences,
    106 kept runs."""
    seqs = mc.iid_database()
    flat, off = mc.flat_of(seqs)
    masked, info = swg.seg_mask_flat(flat, off)
    assert int(off[-1]) == 85423
    assert info == {"residues_masked": 1773, "sequences_masked": 92, "segments": 106}
    assert int((masked != flat).sum()) <= 1773 and set(np.unique(masked[masked != flat]).tolist()) == {mc.X}
    for i in (0, 7, 399):
        s = seqs[i]
        assert np.array_equal(masked[int(off[i]):int(off[i + 1])], mc.apply_mask(s, mc.reference_mask(s)[0]))


def test_db_sequence_reads_the_host_image(swg, cases, tmp_path):
    names = sorted(cases)
    flat, off = mc.flat_of([cases[n] for n in names if len(cases[n]) > 0])
    kept = [n for n in names if len(cases[n]) > 0]
    db = swg.Database(flat, off)
    for i, n in enumerate(kept):
        assert np.array_equal(db.sequence(i), cases[n]), n
    with pytest.raises(swg.SwgError) as e:
        db.sequence(len(kept))
    assert e.value.code == swg.SWG_ERR_ARG
    with pytest.raises(swg.SwgError) as e:
        db.mask_info()
    assert e.value.code == swg.SWG_ERR_STATE
    path = str(tmp_path / "db.swg")
    db.save(path)
    loaded = swg.Database(path=path)
    for i in (0, len(kept) // 2, len(kept) - 1):
        assert np.array_equal(loaded.sequence(i), cases[kept[i]])
    shard = swg.Database(flat, off, shard_rank=1, shard_count=2)      # a shard holds only its own sequences
    held = set(int(v) for v in shard.order())
    missing = next(i for i in range(len(kept)) if i not in held)
    with pytest.raises(swg.SwgError):
        shard.sequence(missing)


def test_end_to_end_case_on_the_cpu(swg, orc):
    """The pinned seed: unmasked, at least 3 decoys among the top 5; masked by the twin, the top 5 is exactly the relatives."""
    c = mc.end_to_end()
    sc = swg.load_scoring("BLOSUM62", -11, -1)
    flat, off = mc.flat_of(c["seqs"])
    plain = orc.score_db(c["query"], flat, off, sc.table(), -11, -1)
    masked_flat, _ = swg.seg_mask_flat(flat, off)
    masked = orc.score_db(c["query"], masked_flat, off, sc.table(), -11, -1)
    top_plain = [i for _, i in mc.top_hits(plain, 5)]
    top_masked = [i for _, i in mc.top_hits(masked, 5)]
    assert sum(i in c["decoys"] for i in top_plain) >= 3
    assert set(top_masked) == c["relatives"]
    assert len({int(masked[i]) for i in top_masked}) == 5           # no ties: the list's order is the scores'
