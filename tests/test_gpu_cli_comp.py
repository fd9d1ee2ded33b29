"""GPU (-m gpu): `smith_waterman --iterations 2 --compstats` on a database with planted composition-biased sequences.

The database is 200 unbiased sequences, 6 true relatives of the query (mutated copies between unbiased flanks) and 5
planted sequences biased like the query but unrelated to it: shuffles of a fixed Q/E/K-rich composition.  Without
--compstats iteration 1 includes the five (their raw scores are twice the best unbiased sequence's); with it the entries
that leave are exactly those the numpy model (comp_model.py) predicts from the library's own calibration -- all five
planted ones among them, no relative."""
import re

import numpy as np
import pytest

import comp_cases as cc
import comp_model as cm
import pssm_build_cases as pc
from test_cli import B62, _letters, _run, _write_fasta
from test_gpu_parity import _reset_options

pytestmark = pytest.mark.gpu

GAPS = pc.MATRICES["BLOSUM62"]
INCLUSION = 1e-3
CALIB = {"calib_seqs": 8192, "calib_len": 384, "calib_seed": 1}      # the tool runs on the library's defaults
N_BG, N_REL, N_PLANTED = 200, 6, 5
LEAVES_RX = re.compile(r"iteration 1: entry (\d+) leaves by its composition: score (-?\d+) adjusted to (-?\d+)")


@pytest.fixture(autouse=True)
def _options(ctx):
    _reset_options(ctx)
    for key, v in CALIB.items():
        ctx.set_option(key, v)
    yield
    _reset_options(ctx)
    ctx.set_option("comp_scale", 32)


def world():
    rng = np.random.default_rng([2026, 7])
    q = cc.biased_seq(rng, 200, cc.QEK, 0.4)
    seqs = [cc.background_seq(rng, int(rng.integers(150, 400))) for _ in range(N_BG)]
    relatives = []
    for _ in range(N_REL):
        m = q.copy()
        pick = rng.random(len(q)) < 0.35
        m[pick] = cc.background_seq(rng, int(pick.sum()))
        relatives.append(len(seqs))
        seqs.append(np.concatenate([cc.background_seq(rng, 80), m, cc.background_seq(rng, 80)]))
    planted = []
    for _ in range(N_PLANTED):
        planted.append(len(seqs))
        seqs.append(cc.shuffled_composition(rng, 800, cc.QEK, 0.38))
    order = rng.permutation(len(seqs))                       # (the planted ones are not the last entries of the file)
    place = {int(old): new for new, old in enumerate(order)}
    seqs = [seqs[int(i)] for i in order]
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return dict(q=q, seqs=seqs, flat=np.concatenate(seqs).astype(np.int8), off=off, relatives={place[i] for i in relatives},
                planted={place[i] for i in planted})


def test_iteration_one_drops_what_the_model_predicts(swg, ctx, tmp_path):
    w = world()
    n = len(w["seqs"])
    qf, dbf = tmp_path / "q.fa", tmp_path / "db.fa"
    _write_fasta(str(qf), ["query"], [_letters(swg, w["q"])])
    _write_fasta(str(dbf), ["s%d" % i for i in range(n)], [_letters(swg, s) for s in w["seqs"]])
    base = ["--substitution_matrix", B62, "--gapopen", str(GAPS[0]), "--gapextend", str(GAPS[1]), "--iterations", "2", "--topk", "10",
            "--inclusion", str(INCLUSION)]
    plain = _run(*base, "--files", str(qf), str(dbf))
    adjusted = _run(*base, "--compstats", "--files", str(qf), str(dbf))
    assert plain.returncode == 0 and adjusted.returncode == 0, (plain.stderr[-400:], adjusted.stderr[-400:])
    print(adjusted.stderr)
    # the library, step by step as the tool takes them; the model's prediction from the library's calibration
    sub = pc.table("BLOSUM62")
    ctx.set_scoring(sub, *GAPS)
    ctx.set_query(w["q"])
    db = swg.Database(w["flat"], w["off"]).upload(ctx)
    params = ctx.calibrate()
    residues = int(w["off"][-1])
    least = swg.evalue_min_score(params, residues, INCLUSION)
    included, n_at, _ = ctx.search_above(db, least, cap=500)
    db.close()
    raw = {i for _, i in included}
    assert "iteration 1: %d entries at or above score %d" % (n_at, least) in plain.stderr
    assert "iteration 1: %d entries at or above score %d" % (n_at, least) in adjusted.stderr
    assert "leaves by its composition" not in plain.stderr
    assert w["planted"] <= raw and w["relatives"] <= raw             # without the adjustment all five planted ones are included
    predicted = {}
    for sc, i in included:
        m = cm.adjust(sub, GAPS[0], GAPS[1], w["seqs"][i], query=w["q"])
        print("entry %d: score %d, model ratio16 %d, adjusted %d, E %.3g" % (i, sc, m["ratio16"], m["adj_score"], swg.evalue(params, residues, m["adj_score"])))
        if swg.evalue(params, residues, m["adj_score"]) > INCLUSION:
            predicted[i] = (sc, m["adj_score"])
    left = {int(i): (int(a), int(b)) for i, a, b in LEAVES_RX.findall(adjusted.stderr)}
    assert left == predicted
    assert w["planted"] <= set(left) and not (w["relatives"] & set(left))
    assert "iteration 1: %d of %d entries stay after the composition-based adjustment" % (len(raw) - len(left), len(raw)) in adjusted.stderr
    # the PSSM of iteration 1 is built from other entries, so the two reports differ in their scores
    assert plain.stdout != adjusted.stdout


def test_the_scale_reaches_the_library(swg, ctx, tmp_path):
    """--compstats 1 and --compstats 64: at each scale the entries that leave, and their adjusted scores, are the model's at
    that scale.  The two differ: at F = 1 the table is rounded to whole scores, half of them upwards by a half, which is
    why the default is 32."""
    w = world()
    n = len(w["seqs"])
    qf, dbf = tmp_path / "q.fa", tmp_path / "db.fa"
    _write_fasta(str(qf), ["query"], [_letters(swg, w["q"])])
    _write_fasta(str(dbf), ["s%d" % i for i in range(n)], [_letters(swg, s) for s in w["seqs"]])
    sub = pc.table("BLOSUM62")
    ctx.set_scoring(sub, *GAPS)
    ctx.set_query(w["q"])
    db = swg.Database(w["flat"], w["off"]).upload(ctx)
    params = ctx.calibrate()
    residues = int(w["off"][-1])
    included, _, _ = ctx.search_above(db, swg.evalue_min_score(params, residues, INCLUSION), cap=500)
    db.close()
    got = {}
    for F in (1, 64):
        r = _run("--substitution_matrix", B62, "--gapopen", str(GAPS[0]), "--gapextend", str(GAPS[1]), "--iterations", "2", "--topk", "5",
                 "--inclusion", str(INCLUSION), "--compstats", str(F), "--files", str(qf), str(dbf))
        assert r.returncode == 0, r.stderr[-400:]
        got[F] = {int(i): int(b) for i, a, b in LEAVES_RX.findall(r.stderr)}
        adj = {i: cm.adjust(sub, GAPS[0], GAPS[1], w["seqs"][i], query=w["q"], F=F)["adj_score"] for _, i in included}
        print("F = %d: adjusted scores %s" % (F, adj))
        assert got[F] == {i: a for i, a in adj.items() if swg.evalue(params, residues, a) > INCLUSION}, F
    assert w["planted"] <= set(got[64]) and got[1] != got[64]


# ---- the reports: --evalue, --topk, --tabular, --allqueries -------------------------------------------------------------
TOP_RX = re.compile(r"Top (\d+) hits \(adjusted score, score, entry, name\):")


def _adjusted_blocks(stdout):
    """Every `Top N hits (adjusted score, score, entry, name)` block -> [[(adjusted, score, entry)]]."""
    lines, out = stdout.splitlines(), []
    for at, l in enumerate(lines):
        m = TOP_RX.match(l)
        if m:
            rows = [r.split("\t") for r in lines[at + 1:at + 1 + int(m.group(1))]]
            out.append([(int(r[0]), int(r[1]), int(r[2])) for r in rows])
    return out


def _files_of(swg, w, tmp_path, extra_queries=()):
    n = len(w["seqs"])
    qf, dbf = tmp_path / "q.fa", tmp_path / "db.fa"
    qs = [w["q"]] + list(extra_queries)
    _write_fasta(str(qf), ["query%d" % i for i in range(len(qs))], [_letters(swg, q) for q in qs])
    _write_fasta(str(dbf), ["s%d" % i for i in range(n)], [_letters(swg, s) for s in w["seqs"]])
    return ["--files", str(qf), str(dbf)]


def _ranked(sub, w, q, hits, F=32, keep=None):
    """The model's report of a hit list [(score, entry)]: (adjusted, score, entry) by adjusted score, ties by lower entry."""
    rows = [(cm.adjust(sub, GAPS[0], GAPS[1], w["seqs"][i], query=q, F=F)["adj_score"], sc, i) for sc, i in hits]
    return sorted((r for r in rows if keep is None or keep(r[0])), key=lambda r: (-r[0], r[2]))


def test_evalue_keeps_what_the_model_keeps_and_tabular_prints_it(swg, ctx, tmp_path):
    w = world()
    files = _files_of(swg, w, tmp_path)
    base = ["--substitution_matrix", B62, "--gapopen", str(GAPS[0]), "--gapextend", str(GAPS[1]), "--evalue", str(INCLUSION), "--tabular"]
    plain = _run(*base, *files)
    adjusted = _run(*base, "--compstats", *files)
    assert plain.returncode == 0 and adjusted.returncode == 0, (plain.stderr[-400:], adjusted.stderr[-400:])
    sub = pc.table("BLOSUM62")
    ctx.set_scoring(sub, *GAPS)
    ctx.set_query(w["q"])
    db = swg.Database(w["flat"], w["off"]).upload(ctx)
    params = ctx.calibrate()
    residues = int(w["off"][-1])
    hits, _, _ = ctx.search_above(db, swg.evalue_min_score(params, residues, INCLUSION))
    db.close()
    # without the flag all five planted sequences are within E
    at = plain.stdout.index("Top %d hits (score, entry, name):" % len(hits))
    shown = [int(l.split("\t")[1]) for l in plain.stdout[at:].splitlines()[1:1 + len(hits)]]
    assert shown == [i for _, i in hits] and w["planted"] <= set(shown)
    # with it the kept set is the model's: none of the five, every relative, in the model's order, both scores
    want = _ranked(sub, w, w["q"], hits, keep=lambda a: swg.evalue(params, residues, a) <= INCLUSION)
    (got,) = _adjusted_blocks(adjusted.stdout)
    assert got == want
    kept = {i for _, _, i in got}
    assert not (kept & w["planted"]) and w["relatives"] <= kept and len(kept) < len(hits)
    # the tabular lines: one per kept hit, in that order, with the ADJUSTED E-value, bit score and score
    rows = [l.split("\t") for l in adjusted.stdout.splitlines() if l.startswith("query0\t")]
    assert [r[1] for r in rows] == ["s%d" % i for _, _, i in want]
    for r, (a, sc, i) in zip(rows, want):
        assert int(r[12]) == a != sc
        assert r[10] == "%.3g" % swg.evalue(params, residues, a) and r[11] == "%.1f" % swg.bitscore(params, a), (r, a)


def test_topk_is_ranked_again_and_allqueries_equals_one_by_one(swg, ctx, tmp_path):
    w = world()
    second = cc.background_seq(np.random.default_rng(31), 90)
    third = cc.biased_seq(np.random.default_rng(32), 260, cc.QEK, 0.3)
    K = 12
    base = ["--substitution_matrix", B62, "--gapopen", str(GAPS[0]), "--gapextend", str(GAPS[1]), "--topk", str(K), "--compstats"]
    r = _run(*base, "--allqueries", *_files_of(swg, w, tmp_path, [second, third]))
    assert r.returncode == 0, r.stderr[-400:]
    blocks = _adjusted_blocks(r.stdout)
    assert len(blocks) == 3
    sub = pc.table("BLOSUM62")
    ctx.set_scoring(sub, *GAPS)
    db = swg.Database(w["flat"], w["off"]).upload(ctx)
    reordered = 0
    for q, got in zip([w["q"], second, third], blocks):
        ctx.set_query(q)
        _, hits, _ = ctx.search(db, k=K)
        want = _ranked(sub, w, q, hits)
        assert got == want
        reordered += [i for _, _, i in want] != [i for _, i in hits]
    db.close()
    assert reordered >= 1                                   # (the biased query's planted hits fall behind)
    # the first record alone prints the first block
    one = _run(*base, *_files_of(swg, w, tmp_path))
    assert one.returncode == 0 and _adjusted_blocks(one.stdout) == blocks[:1]
