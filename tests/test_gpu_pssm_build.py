"""GPU (-m gpu): swg_pssm_build / _multi / _multi_pssm -- the paths turned into rows, counted, weighted and scored on the
device.  Truth everywhere is the host twin, swg_pssm_from_paths, fed by what the existing align_hits_multi[_pssm]
returns for the same hits: the int8 PSSM equal in every entry, the unrounded values within 1e-9, info equal (lambda and
Nbar to 1e-12).  Databases hold 64 to 430 sequences of 20 to 300 residues (the 1701-column query has its own two)."""
import functools

import numpy as np
import pytest

import pssm_build_cases as pc
from test_gpu_parity import _reset_options
from test_pssm_build_host import E2E_PINNED, e2e_cpu

pytestmark = pytest.mark.gpu

B62, GAPS = "BLOSUM62", pc.MATRICES["BLOSUM62"]


@pytest.fixture(autouse=True)
def _options(ctx):
    _reset_options(ctx)
    ctx.set_option("pssm_msa_mb", 1024)
    yield
    _reset_options(ctx)
    ctx.set_option("pssm_msa_mb", 1024)


def _hits(indices):
    return [(0, int(i)) for i in indices]


def _twin(swg, ctx, db, sub, flat, off, queries, hits, pssms=None, **kw):
    """The host twin per query, fed by the device's own alignments of the same hits."""
    if pssms is None:
        als = ctx.align_hits_multi(db, queries, hits)
    else:
        als = ctx.align_hits_multi_pssm(db, pssms, hits)
    return als, [swg.pssm_from_paths(sub, q, flat, off, al, want_values=True, **kw) for q, al in zip(queries, als)]


def _assert_same(got, want, what):
    (pssm, values, info), (wp, wv, wi) = got, want
    worst = float(np.abs(values - wv).max())
    print(what, "rows", info["n_rows"], "Nbar", info["n_distinct"], "observed", info["n_observed"], "worst", worst)
    assert np.array_equal(pssm, wp), what
    assert worst <= 1e-9, what
    assert abs(info["lambda"] - wi["lambda"]) <= 1e-12 and abs(info["n_distinct"] - wi["n_distinct"]) <= 1e-12, what
    for key in ("n_rows", "n_observed", "n_clamped"):
        assert info[key] == wi[key], (what, key)


def _check_batch(swg, ctx, db, flat, off, queries, hits, what, sub=None, pssms=None, **kw):
    sub = pc.table(B62) if sub is None else sub
    als, want = _twin(swg, ctx, db, sub, flat, off, queries, hits, pssms=pssms, **kw)
    if pssms is None:
        got = ctx.build_pssm_multi(db, queries, hits, want_values=True, **kw)
    else:
        got = ctx.build_pssm_multi_pssm(db, pssms, queries, hits, want_values=True, **kw)
    for i in range(len(queries)):
        _assert_same((got[0][i], got[1][i], got[2][i]), want[i], "%s[%d]" % (what, i))
    return als, got


def _family_db(seed, lq, n_hits, n_random, **kw):
    q, flat, off, hits = pc.family(seed, lq, n_hits, n_random=n_random, **kw)
    return q, flat, off, hits


# ---- one query ----------------------------------------------------------------------------------------------------------
def test_a_query_of_one_residue(swg, ctx):
    q = np.array([pc.idx("W")], dtype=np.int8)
    rng = np.random.default_rng(1)
    seqs = [np.array([pc.idx(c) for c in s], dtype=np.int8) for s in ("AWA", "GGWG", "W", "KYK")] + [pc.random_seq(rng, 20 + i) for i in range(60)]
    flat, off = pc.pack(seqs)
    ctx.set_scoring(pc.table(B62), *GAPS)
    db = swg.Database(flat, off).upload(ctx)
    _check_batch(swg, ctx, db, flat, off, [q], [_hits([0, 1, 2, 3, 10])], "lq1")
    ctx.set_query(q)                                                  # the same through the context's query
    pssm, values, info = ctx.build_pssm(db, _hits([0, 1, 2, 3, 10]), want_values=True)
    want = ctx.build_pssm_multi(db, [q], [_hits([0, 1, 2, 3, 10])], want_values=True)
    assert np.array_equal(pssm, want[0][0]) and np.array_equal(values, want[1][0]) and info == want[2][0]
    db.close()


def test_lq37_with_24_hits_of_both_gap_kinds(swg, ctx):
    q, flat, off, hits = _family_db(41, 37, 24, 40, gapped=12, flank=8)
    ctx.set_scoring(pc.table(B62), *GAPS)
    db = swg.Database(flat, off).upload(ctx)
    als, _ = _check_batch(swg, ctx, db, flat, off, [q], [_hits(hits)], "lq37")
    ops = "/".join(a["ops"] for a in als[0])
    assert "I" in ops and "D" in ops
    db.close()


def test_lq257_with_300_hits_crosses_the_column_tile_and_256_rows(swg, ctx):
    q, flat, off, hits = _family_db(42, 257, 300, 0, gapped=8, subst=(0.1, 0.7))
    ctx.set_scoring(pc.table(B62), *GAPS)
    db = swg.Database(flat, off).upload(ctx)
    _, got = _check_batch(swg, ctx, db, flat, off, [q], [_hits(hits)], "lq257")
    assert got[2][0]["n_rows"] == 301
    db.close()


@functools.lru_cache(maxsize=None)
def _batch():
    """Queries of 1, 37, 64, 130 and 257 residues over one database of their families and 30 unrelated sequences; the rows
    hold 0, 1, 8, 8 and 5 hits, and sequence `shared` is a hit of two queries."""
    rng = np.random.default_rng(43)
    queries, seqs, rows = [np.array([pc.idx("K")], dtype=np.int8)], [], [[]]
    for lq, n in ((37, 1), (64, 8), (130, 8), (257, 5)):
        q = pc.random_seq(rng, lq)
        first = len(seqs)
        seqs += [pc.relative(rng, q, 0.1 + 0.05 * h, ins=[(lq // 3, 2)] if h % 2 else (), dele=[(lq // 2, 2)] if h % 3 == 0 else (), flank=6)
                 for h in range(8)]
        queries.append(q)
        rows.append(list(range(first, first + n)))
    shared = rows[2][3]
    rows[3][0] = shared                                               # one of the 64-column query's hits, hit by the 130-column one too
    seqs += [pc.random_seq(rng, int(rng.integers(20, 301))) for _ in range(30)]
    flat, off = pc.pack(seqs)
    return queries, flat, off, [_hits(r) for r in rows], shared


def test_a_batch_of_lengths_and_row_sizes(swg, ctx):
    queries, flat, off, hits, shared = _batch()
    assert [len(q) for q in queries] == [1, 37, 64, 130, 257] and [len(h) for h in hits] == [0, 1, 8, 8, 5]
    assert sum(shared in [i for _, i in row] for row in hits) == 2
    ctx.set_scoring(pc.table(B62), *GAPS)
    db = swg.Database(flat, off).upload(ctx)
    _, got = _check_batch(swg, ctx, db, flat, off, queries, hits, "batch")
    rows0 = pc.table(B62)[queries[0].astype(np.int64)].copy()
    rows0[:, 0] = 0
    assert np.array_equal(got[0][0], rows0)                           # no hits: the matrix's own row
    # several chunks (every query alone) and a second call: the same bytes
    ctx.set_option("pssm_msa_mb", 0)
    chunked = ctx.build_pssm_multi(db, queries, hits, want_values=True)
    ctx.set_option("pssm_msa_mb", 1024)
    again = ctx.build_pssm_multi(db, queries, hits, want_values=True)
    for other in (chunked, again):
        for i in range(len(queries)):
            assert other[0][i].tobytes() == got[0][i].tobytes() and other[1][i].tobytes() == got[1][i].tobytes(), i
            assert other[2][i] == got[2][i], i
    # a caller's background and pseudocount
    freq = pc.builtin_freq()
    freq[pc.idx("X")] = 0.5
    _check_batch(swg, ctx, db, flat, off, queries, hits, "batch, freq", freq=freq, pseudocount=3.5)
    db.close()


def test_lq1701_takes_the_tracebacks_class_without_lds(swg, ctx):
    rng = np.random.default_rng(44)
    q = pc.random_seq(rng, 1701)
    seqs = [pc.relative(rng, q, 0.3, lo=700, hi=1000, ins=[(800, 3)], dele=[(900, 2)], flank=0), pc.relative(rng, q, 0.5, lo=0, hi=250, flank=10)]
    seqs += [pc.random_seq(rng, 40) for _ in range(62)]
    flat, off = pc.pack(seqs)
    ctx.set_scoring(pc.table(B62), *GAPS)
    db = swg.Database(flat, off).upload(ctx)
    _check_batch(swg, ctx, db, flat, off, [q], [_hits([0, 1])], "lq1701")
    db.close()


def test_a_view(swg, ctx):
    q, flat, off, hits = _family_db(45, 64, 10, 60)
    ctx.set_scoring(pc.table(B62), *GAPS)
    db = swg.Database(flat, off).upload(ctx)
    view = db.view(ctx, list(range(0, 40)))
    _, got = _check_batch(swg, ctx, view, flat, off, [q], [_hits(hits)], "view")
    whole = ctx.build_pssm_multi(db, [q], [_hits(hits)], want_values=True)
    assert got[0][0].tobytes() == whole[0][0].tobytes() and got[1][0].tobytes() == whole[1][0].tobytes()
    with pytest.raises(swg.SwgError) as e:                            # a hit the view does not select
        ctx.build_pssm_multi(view, [q], [_hits([50])])
    assert e.value.code == swg.SWG_ERR_ARG
    view.close()
    db.close()


def test_the_pssm_form_builds_iteration_two_from_iteration_one(swg, ctx):
    q, flat, off, hits = _family_db(46, 90, 16, 60, subst=(0.2, 0.7), gapped=4)
    sub = pc.table(B62)
    ctx.set_scoring(sub, *GAPS)
    db = swg.Database(flat, off).upload(ctx)
    first = ctx.build_pssm_multi(db, [q], [_hits(hits[:8])])[0][0]
    assert not np.array_equal(first, sub[q.astype(np.int64)])
    _, got = _check_batch(swg, ctx, db, flat, off, [q], [_hits(hits)], "pssm form", pssms=[first])
    ctx.set_query_pssm(first)                                         # and through the context's PSSM query
    pssm, values, info = ctx.build_pssm(db, _hits(hits), query_residues=q, want_values=True)
    assert pssm.tobytes() == got[0][0].tobytes() and values.tobytes() == got[1][0].tobytes() and info == got[2][0]
    with pytest.raises(swg.SwgError) as e:
        ctx.build_pssm(db, _hits(hits))                               # a PSSM query needs its residues
    assert e.value.code == swg.SWG_ERR_ARG and "query_residues" in str(e.value)
    with pytest.raises(ValueError):
        ctx.build_pssm(db, _hits(hits), query_residues=q[:-1])       # as many residues as the PSSM has rows
    db.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone(swg, ctx):
    import ctypes as C
    q, flat, off, hits = _family_db(47, 40, 4, 60)
    ctx.set_scoring(pc.table(B62), *GAPS)
    db = swg.Database(flat, off).upload(ctx)
    good = dict(db=db, queries=[q], hits=[_hits(hits)])

    def refused(code=None, **kw):
        args = dict(good, **kw)
        with pytest.raises(swg.SwgError) as e:
            ctx.build_pssm_multi(args.pop("db"), args.pop("queries"), args.pop("hits"), **args)
        assert e.value.code == (swg.SWG_ERR_ARG if code is None else code), str(e.value)
        return str(e.value)

    assert "not in this database shard" in refused(hits=[_hits([len(off) + 5])])
    assert "pseudocount" in refused(pseudocount=0.0)
    assert "pseudocount" in refused(pseudocount=float("nan"))
    assert "freq" in refused(freq=np.full(32, -1.0))
    assert "freq" in refused(freq=np.r_[1.0, np.ones(31)])
    refused(code=swg.SWG_ERR_RESIDUE, queries=[np.array([1, 0, 3] + [4] * 37, dtype=np.int8)])
    ctx.set_scoring(np.ones((32, 32), dtype=np.int8), *GAPS)         # a matrix without a lambda
    assert "lambda" in refused()
    ctx.set_scoring(pc.table(B62), *GAPS)
    # the raw entry point: outputs untouched by a refusal, NULL outputs with work to do refused
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    qoff = np.array([0, 40], dtype=np.uint64)
    harr = (swg.Hit * 4)(*[swg.Hit(0, i) for i in hits])
    nh = (C.c_size_t * 1)(4)
    out = np.full((40, 32), 77, dtype=np.int8)
    call = lambda pseudo, outp: swg.lib.swg_pssm_build_multi(ctx.handle, db.handle, vp(q), vp(qoff), 1, C.cast(harr, C.c_void_p), 4,
                                                             C.cast(nh, C.c_void_p), None, pseudo, outp, None, None)
    assert call(-2.0, vp(out)) == swg.SWG_ERR_ARG and (out == 77).all()
    assert call(10.0, None) == swg.SWG_ERR_ARG
    assert call(10.0, vp(out)) == swg.SWG_OK and not (out == 77).all()
    host = swg.Database(flat, off)                                    # not resident
    refused(code=swg.SWG_ERR_STATE, db=host)
    host.close()
    assert swg.lib.swg_pssm_build_multi(None, db.handle, vp(q), vp(qoff), 1, None, 0, C.cast(nh, C.c_void_p), None, 10.0, vp(out), None,
                                        None) == swg.SWG_ERR_ARG
    db.close()


# ---- the end-to-end fixture -----------------------------------------------------------------------------------------------
def test_search_build_search_again(swg, ctx):
    e = e2e_cpu()
    sub = pc.table(B62)
    ctx.set_scoring(sub, *GAPS)
    ctx.set_query(e["q"])
    db = swg.Database(e["flat"], e["off"]).upload(ctx)
    hits, n_total, _ = ctx.search_above(db, pc.E2E["include_score"])
    assert [i for _, i in hits] == e["included"] and n_total == len(hits)
    pssm, _, info = ctx.build_pssm(db, hits)
    assert np.array_equal(pssm, e["pssm"]) and info["n_rows"] == 1 + len(hits)
    scores2 = ctx.search_multi_pssm(db, [pssm], k=pc.E2E["top"])
    assert np.array_equal(np.asarray(scores2[0][0]), e["scores2"])
    first = pc.family_in_top(ctx.search(db)[0], e["is_family"], pc.E2E["top"])
    second = pc.family_in_top(np.asarray(scores2[0][0]), e["is_family"], pc.E2E["top"])
    print("family members in the top %d: %d, then %d" % (pc.E2E["top"], first, second))
    assert (first, second) == (E2E_PINNED["first"], E2E_PINNED["second"])
    db.close()
