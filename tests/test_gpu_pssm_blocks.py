"""GPU (-m gpu): swg_pssm_build / _multi / _multi_pssm under options "pssm_blocks" (per-column alignment blocks) and
"pssm_purge" (near-identical hits dropped), in all four combinations.  Truth is the host twin, swg_pssm_from_paths_ex
with the same two options, fed by what align_hits_multi[_pssm] returns for the same hits: the int8 PSSM equal in every
entry, the unrounded values within 1e-9, info equal (lambda and Nbar to 1e-12).  A case aligns once and builds four times.
The capacities of the new kernels (csrc/swg_pssm.hip) are restated here; a case lies either side of each."""
import numpy as np
import pytest

import pssm_blocks_cases as bc
import pssm_build_cases as pc
from test_cli import B62 as B62_FILE, _letters, _run, _write_fasta
from test_gpu_cli_iterations import CALIB, INCLUSION
from test_gpu_parity import _reset_options
from test_gpu_pssm_build import _batch, _hits
from test_pssm_build_host import e2e_cpu

pytestmark = pytest.mark.gpu

B62, GAPS = "BLOSUM62", pc.MATRICES["BLOSUM62"]
COMBOS = ((0, 0), (1, 0), (0, 94), (1, 94))                           # (pssm_blocks, pssm_purge)
TILE = 256          # SWG_PSSM_TILE: columns of a block the blocks kernel counts at a time
SCORE_TILE = 128    # SWG_PSSM_SCORE_TILE: columns of a segment it scores at a time
ROWS_LDS = 1024     # SWG_PSSM_ROWS_LDS: rows whose weights it keeps in LDS; the rows beyond take global memory
NEAR_WORD = 64      # SWG_PSSM_NEAR_WORD: rows s of one wavefront's share of a pair launch (one word of near bits)
NEAR_ROUND = 256    # SWG_PSSM_NEAR_WORD x SWG_PSSM_NEAR_WAVES: rows s a workgroup of the pair launch takes per round
PURGE_PASS = 4096   # 64 lanes x 64 rows: rows whose kept bits the purge's wavefront meets in one pass


def _set(ctx, blocks, purge):
    ctx.set_option("pssm_blocks", blocks)
    ctx.set_option("pssm_purge", purge)


@pytest.fixture(autouse=True)
def _options(ctx):
    _reset_options(ctx)
    ctx.set_option("pssm_msa_mb", 1024)
    _set(ctx, 0, 0)
    yield
    _reset_options(ctx)
    ctx.set_option("pssm_msa_mb", 1024)
    _set(ctx, 0, 0)


def _assert_same(got, want, what):
    (pssm, values, info), (wp, wv, wi) = got, want
    worst = float(np.abs(values - wv).max())
    print(what, "rows", info["n_rows"], "purged", info["n_purged"], "Nbar", info["n_distinct"], "observed", info["n_observed"], "worst", worst)
    assert np.array_equal(pssm, wp), what
    assert worst <= 1e-9, what
    assert abs(info["lambda"] - wi["lambda"]) <= 1e-12 and abs(info["n_distinct"] - wi["n_distinct"]) <= 1e-12, what
    for key in ("n_rows", "n_observed", "n_clamped", "n_purged"):
        assert info[key] == wi[key], (what, key)


def _check(swg, ctx, db, flat, off, queries, hits, what, pssms=None, combos=COMBOS):
    """Every combination against the twin -> (alignments, {combination: what build_pssm_multi[_pssm] returned})."""
    sub = pc.table(B62)
    als = ctx.align_hits_multi(db, queries, hits) if pssms is None else ctx.align_hits_multi_pssm(db, pssms, hits)
    out = {}
    for blocks, purge in combos:
        _set(ctx, blocks, purge)
        if pssms is None:
            got = ctx.build_pssm_multi(db, queries, hits, want_values=True)
        else:
            got = ctx.build_pssm_multi_pssm(db, pssms, queries, hits, want_values=True)
        for i, (q, al) in enumerate(zip(queries, als)):
            want = swg.pssm_from_paths(sub, q, flat, off, al, want_values=True, blocks=bool(blocks), purge=purge)
            _assert_same((got[0][i], got[1][i], got[2][i]), want, "%s[%d] blocks %d purge %d" % (what, i, blocks, purge))
        out[(blocks, purge)] = got
    _set(ctx, 0, 0)
    return als, out


def _with_random(seed, flat, off, n_random=40):
    """The case's sequences followed by unrelated ones: a database of a size the search kernels take."""
    rng = np.random.default_rng(seed)
    seqs = [flat[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]
    return pc.pack(seqs + [pc.random_seq(rng, int(rng.integers(20, 301))) for _ in range(n_random)])


def _same_bytes(a, b, n):
    for i in range(n):
        assert a[0][i].tobytes() == b[0][i].tobytes() and a[1][i].tobytes() == b[1][i].tobytes() and a[2][i] == b[2][i], i


# ---- one query ----------------------------------------------------------------------------------------------------------
def test_a_query_of_one_residue(swg, ctx):
    q = np.array([pc.idx("W")], dtype=np.int8)
    rng = np.random.default_rng(1)
    seqs = [np.array([pc.idx(c) for c in s], dtype=np.int8) for s in ("AWA", "GGWG", "W", "KYK")] + [pc.random_seq(rng, 20 + i) for i in range(60)]
    flat, off = pc.pack(seqs)
    ctx.set_scoring(pc.table(B62), *GAPS)
    db = swg.Database(flat, off).upload(ctx)
    hits = _hits([0, 1, 2, 3, 10])
    _, out = _check(swg, ctx, db, flat, off, [q], [hits], "lq1")
    assert out[(0, 94)][2][0]["n_purged"] >= 3                        # the three that show W (AWA, GGWG, W): identical to the query
    ctx.set_query(q)                                                  # the same through the context's query
    for combo in COMBOS:
        _set(ctx, *combo)
        pssm, values, info = ctx.build_pssm(db, hits, want_values=True)
        want = out[combo]
        assert np.array_equal(pssm, want[0][0]) and np.array_equal(values, want[1][0]) and info == want[2][0]
    db.close()


def test_partial_hits_differ_under_blocks(swg, ctx):
    q, flat, off, hits = pc.family(12, 90, 6, partial=6)
    flat, off = _with_random(2, flat, off)
    ctx.set_scoring(pc.table(B62), *GAPS)
    db = swg.Database(flat, off).upload(ctx)
    als, out = _check(swg, ctx, db, flat, off, [q], [_hits(hits)], "partial")
    assert all(a["q_begin"] > 0 and a["q_end"] < 90 for a in als[0])
    assert not np.array_equal(out[(1, 0)][0][0], out[(0, 0)][0][0])
    db.close()


def test_staggered_extents_make_more_segments_than_rows(swg, ctx):
    q, flat, off, hits = bc.staggered()
    flat, off = _with_random(3, flat, off)
    ctx.set_scoring(pc.table(B62), *GAPS)
    db = swg.Database(flat, off).upload(ctx)
    als, _ = _check(swg, ctx, db, flat, off, [q], [_hits(hits)], "staggered")
    assert bc.segments_of(bc.extents_of(len(q), als[0])) == 2 * len(hits) + 1
    db.close()


def test_two_domains_hit_by_1_and_by_20_rows(swg, ctx):
    q, flat, off, hits = bc.two_domains()
    flat, off = _with_random(4, flat, off)
    ctx.set_scoring(pc.table(B62), *GAPS)
    db = swg.Database(flat, off).upload(ctx)
    als, out = _check(swg, ctx, db, flat, off, [q], [_hits(hits)], "two domains")
    assert (als[0][0]["q_begin"], als[0][0]["q_end"]) == (5, 40) and all((a["q_begin"], a["q_end"]) == (55, 95) for a in als[0][1:])
    sub0 = pc.table(B62)[q.astype(np.int64)]
    alone = np.r_[0:5, 40:55, 95:100]                                 # the columns only row 0 covers: the matrix's row, rescaled
    assert np.array_equal(out[(1, 0)][0][0][alone][:, pc.STD_IDX.astype(np.int64)], sub0[alone][:, pc.STD_IDX.astype(np.int64)])
    db.close()


def test_a_gap_inside_an_extent(swg, ctx):
    q, flat, off, hits = bc.gap_row()
    flat, off = _with_random(5, flat, off)
    ctx.set_scoring(pc.table(B62), *GAPS)
    db = swg.Database(flat, off).upload(ctx)
    als, _ = _check(swg, ctx, db, flat, off, [q], [_hits(hits)], "gap row")
    assert "DD" in als[0][0]["ops"]
    db.close()


def test_lq257_with_300_spanning_hits(swg, ctx):
    """The block is wider than one column tile, a segment wider than two score tiles, the rows more than a wavefront's
    word of near bits and more than one round of the pair launch."""
    q, flat, off, hits = pc.family(42, 257, 300, 0, gapped=8, subst=(0.1, 0.7))
    ctx.set_scoring(pc.table(B62), *GAPS)
    db = swg.Database(flat, off).upload(ctx)
    _, out = _check(swg, ctx, db, flat, off, [q], [_hits(hits)], "lq257")
    assert out[(1, 0)][2][0]["n_rows"] == 301
    db.close()


# ---- either side of every capacity ------------------------------------------------------------------------------------
@pytest.mark.parametrize("lq", [SCORE_TILE, SCORE_TILE + 1, TILE, TILE + 1])
def test_either_side_of_the_column_tiles(swg, ctx, lq):
    q, flat, off, hits = pc.family(60 + lq, lq, 6, n_random=40, gapped=2, flank=0, keep=(0, 1, 2, lq - 3, lq - 2, lq - 1))
    ctx.set_scoring(pc.table(B62), *GAPS)
    db = swg.Database(flat, off).upload(ctx)
    als, _ = _check(swg, ctx, db, flat, off, [q], [_hits(hits)], "lq%d" % lq)
    assert max(a["q_end"] - a["q_begin"] for a in als[0]) == lq      # a block and a segment as wide as the query
    db.close()


def _many_rows(n_hits):
    """A 40-column query and 48 relatives (4 gapped, 10 partial); the list names the first 40 over and over, then the
    last 8 once each -- rows kept at the list's far end -- and the very last again, purged by a kept row next to it."""
    q, flat, off, _ = pc.family(71, 40, 48, n_random=16, gapped=4, partial=10, subst=(0.1, 0.7))
    order = [j % 40 for j in range(max(n_hits - 9, 0))] + list(range(40, 48)) + [47]
    return q, flat, off, order[-n_hits:]


@pytest.mark.parametrize("rows", [NEAR_WORD, NEAR_WORD + 1, NEAR_ROUND, NEAR_ROUND + 1, ROWS_LDS, ROWS_LDS + 1, PURGE_PASS, PURGE_PASS + 1])
def test_either_side_of_the_row_capacities(swg, ctx, rows):
    q, flat, off, order = _many_rows(rows - 1)
    assert len(order) == rows - 1
    ctx.set_scoring(pc.table(B62), *GAPS)
    db = swg.Database(flat, off).upload(ctx)
    _, out = _check(swg, ctx, db, flat, off, [q], [_hits(order)], "rows%d" % rows)
    info = out[(1, 94)][2][0]
    assert info["n_rows"] + info["n_purged"] == rows and info["n_purged"] >= rows - 1 - 48 and info["n_rows"] >= 20
    db.close()


def test_lq1701_takes_the_tracebacks_class_without_lds(swg, ctx):
    rng = np.random.default_rng(44)
    q = pc.random_seq(rng, 1701)
    seqs = [pc.relative(rng, q, 0.3, lo=700, hi=1000, ins=[(800, 3)], dele=[(900, 2)], flank=0), pc.relative(rng, q, 0.5, lo=0, hi=250, flank=10)]
    seqs += [pc.random_seq(rng, 40) for _ in range(62)]
    flat, off = pc.pack(seqs)
    ctx.set_scoring(pc.table(B62), *GAPS)
    db = swg.Database(flat, off).upload(ctx)
    _check(swg, ctx, db, flat, off, [q], [_hits([0, 1, 0])], "lq1701")
    db.close()


# ---- batches ------------------------------------------------------------------------------------------------------------
def test_a_batch_in_chunks_and_twice_gives_the_same_bytes(swg, ctx):
    queries, flat, off, hits, _ = _batch()
    assert [len(q) for q in queries] == [1, 37, 64, 130, 257] and [len(h) for h in hits] == [0, 1, 8, 8, 5]
    hits = [row + row[:2] for row in hits]                            # (repeats: something to purge)
    ctx.set_scoring(pc.table(B62), *GAPS)
    db = swg.Database(flat, off).upload(ctx)
    _, out = _check(swg, ctx, db, flat, off, queries, hits, "batch")
    assert all(i["n_purged"] >= least for i, least in zip(out[(1, 94)][2], [0, 1, 2, 2, 2]))
    for combo in COMBOS:
        _set(ctx, *combo)
        ctx.set_option("pssm_msa_mb", 0)                              # every query a chunk of its own
        chunked = ctx.build_pssm_multi(db, queries, hits, want_values=True)
        ctx.set_option("pssm_msa_mb", 1024)
        again = ctx.build_pssm_multi(db, queries, hits, want_values=True)
        _same_bytes(chunked, out[combo], len(queries))
        _same_bytes(again, out[combo], len(queries))
    db.close()


def test_a_view(swg, ctx):
    q, flat, off, hits = pc.family(45, 64, 10, n_random=60, partial=4)
    ctx.set_scoring(pc.table(B62), *GAPS)
    db = swg.Database(flat, off).upload(ctx)
    view = db.view(ctx, list(range(0, 40)))
    _, got = _check(swg, ctx, view, flat, off, [q], [_hits(hits + hits[:3])], "view")
    _, whole = _check(swg, ctx, db, flat, off, [q], [_hits(hits + hits[:3])], "whole")
    for combo in COMBOS:
        _same_bytes(got[combo], whole[combo], 1)
    view.close()
    db.close()


def test_the_pssm_form(swg, ctx):
    q, flat, off, hits = pc.family(46, 90, 16, n_random=60, subst=(0.2, 0.7), gapped=4, partial=5)
    sub = pc.table(B62)
    ctx.set_scoring(sub, *GAPS)
    db = swg.Database(flat, off).upload(ctx)
    _set(ctx, 1, 94)
    first = ctx.build_pssm_multi(db, [q], [_hits(hits[:8])])[0][0]
    assert not np.array_equal(first, sub[q.astype(np.int64)])
    _, out = _check(swg, ctx, db, flat, off, [q], [_hits(hits + hits[:2])], "pssm form", pssms=[first])
    ctx.set_query_pssm(first)                                         # and through the context's PSSM query
    _set(ctx, 1, 94)
    pssm, values, info = ctx.build_pssm(db, _hits(hits + hits[:2]), query_residues=q, want_values=True)
    want = out[(1, 94)]
    assert pssm.tobytes() == want[0][0].tobytes() and values.tobytes() == want[1][0].tobytes() and info == want[2][0]
    db.close()


# ---- the options ----------------------------------------------------------------------------------------------------------
def test_options_back_to_zero_give_the_bytes_of_a_context_that_never_set_them(swg, ctx):
    queries, flat, off, hits, _ = _batch()
    ctx.set_scoring(pc.table(B62), *GAPS)
    db = swg.Database(flat, off).upload(ctx)
    fresh = swg.Context(0)                                            # options never touched
    fresh.set_scoring(pc.table(B62), *GAPS)
    fdb = swg.Database(flat, off).upload(fresh)
    before = fresh.build_pssm_multi(fdb, queries, hits, want_values=True)
    fdb.close()
    fresh.close()
    _set(ctx, 1, 94)
    changed = ctx.build_pssm_multi(db, queries, hits, want_values=True)
    assert any(changed[0][i].tobytes() != before[0][i].tobytes() for i in range(len(queries)))
    _set(ctx, 0, 0)
    after = ctx.build_pssm_multi(db, queries, hits, want_values=True)
    _same_bytes(after, before, len(queries))
    assert all(i["n_purged"] == 0 for i in after[2])
    db.close()


def test_option_values_are_checked(swg, ctx):
    for key, bad in (("pssm_blocks", (-1, 2)), ("pssm_purge", (49, 101, 1, -94))):
        for v in bad:
            with pytest.raises(swg.SwgError) as e:
                ctx.set_option(key, v)
            assert e.value.code == swg.SWG_ERR_ARG and key in str(e.value)
    for v in (50, 94, 100, 0):
        ctx.set_option("pssm_purge", v)


# ---- the tool -----------------------------------------------------------------------------------------------------------
def test_the_tool_with_psiblocks_and_purge_writes_the_twins_pssm(swg, ctx, tmp_path):
    e = e2e_cpu()
    n = len(e["off"]) - 1
    qf, dbf, out = tmp_path / "q.fa", tmp_path / "db.fa", tmp_path / "it.pssm"
    _write_fasta(str(qf), ["query"], [_letters(swg, e["q"])])
    _write_fasta(str(dbf), ["s%d" % i for i in range(n)], [_letters(swg, e["flat"][int(e["off"][i]):int(e["off"][i + 1])]) for i in range(n)])
    r = _run("--substitution_matrix", B62_FILE, "--gapopen", str(GAPS[0]), "--gapextend", str(GAPS[1]), "--iterations", "2", "--psiblocks",
             "--purge", "94", "--topk", str(pc.E2E["top"]), "--inclusion", str(INCLUSION), "--out_pssm", str(out), "--files", str(qf), str(dbf))
    assert r.returncode == 0, r.stderr[-400:]
    for key, v in CALIB.items():
        ctx.set_option(key, v)
    sub = pc.table(B62)
    ctx.set_scoring(sub, *GAPS)
    ctx.set_query(e["q"])
    db = swg.Database(e["flat"], e["off"]).upload(ctx)
    least = swg.evalue_min_score(ctx.calibrate(), int(e["off"][-1]), INCLUSION)
    included, _, _ = ctx.search_above(db, least, cap=500)
    assert [i for _, i in included] == e["included"]
    al = ctx.align_hits_multi(db, [e["q"]], [included])[0]
    want, _, info = swg.pssm_from_paths(sub, e["q"], e["flat"], e["off"], al, blocks=True, purge=94)
    back, q = swg.read_pssm(str(out), swg.load_scoring("BLOSUM62"))
    assert np.array_equal(back, want) and np.array_equal(q, e["q"])
    print("included", len(included), "rows", info["n_rows"], "purged", info["n_purged"], "entries that differ from the whole-query model's",
          int((want != e["pssm"]).sum()))
    db.close()
