"""GPU (-m gpu): the `smith_waterman` tool's --evalue E -- three query records against a 300-sequence FASTA database,
each calibrated on the device and cut at its own derived score -- against the Python binding on the same calibration:
the least scores, the hit blocks, and --tabular's thirteen columns, whose evalue and bitscore are the helpers' values."""
import re

import numpy as np
import pytest

from test_cli import B62, _letters, _run, _write_fasta
from test_gpu_cli_above_multi import _records
from test_gpu_parity import _reset_options
from test_pssm_host import write_ascii_pssm

pytestmark = pytest.mark.gpu

K, E, GAPS = 5, 10.0, (-11, -1)
HEAD13 = "# Fields: query, entry, pident, length, mismatch, gapopen, qstart, qend, sstart, send, evalue, bitscore, score"
HEAD11 = "# Fields: query, entry, pident, length, mismatch, gapopen, qstart, qend, sstart, send, score"
SCORING = ("--substitution_matrix", B62, "--gapopen", str(GAPS[0]), "--gapextend", str(GAPS[1]))


@pytest.fixture(autouse=True)
def _options(ctx):
    _reset_options(ctx)
    for key, v in (("calib_seqs", 8192), ("calib_len", 384), ("calib_seed", 1)):
        ctx.set_option(key, v)
    ctx.set_option("autotune", 0)
    yield
    ctx.set_option("autotune", 1)


@pytest.fixture(scope="module")
def case(swg, ctx, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("cli_evalue")
    sc = swg.load_scoring("BLOSUM62")
    qs = [swg.synth_query(0xE0A1 + r, L) for r, L in enumerate((120, 60, 200))]
    flat, off = swg.synth_db(0x5EED0E01, 299, median=250.0, max_len=900)
    seqs = [flat[int(off[i]):int(off[i + 1])] for i in range(299)]
    rng = np.random.default_rng(5)
    rel = qs[0].copy()                                   # a relative of record 0: a hit with a tiny E-value
    rel[rng.random(len(rel)) < 0.3] = qs[1][:1]
    seqs.insert(137, rel)
    names = ["db%d some description" % i for i in range(len(seqs))]
    qf, df = tmp / "queries.fasta", tmp / "db.fasta"
    _write_fasta(qf, ["rec%d" % r for r in range(3)], [_letters(swg, q) for q in qs])
    _write_fasta(df, names, [_letters(swg, s) for s in seqs])
    dflat = np.concatenate(seqs).astype(np.int8)
    doff = np.zeros(len(seqs) + 1, dtype=np.uint64)
    doff[1:] = np.cumsum([len(s) for s in seqs])
    return dict(tmp=tmp, sc=sc, qs=qs, qf=str(qf), df=str(df), names=names, flat=dflat, off=doff)


def _library(swg, ctx, case, db, residues, freq=None):
    """What the tool must arrive at: every record's fit, least score and hits through the binding."""
    ctx.set_scoring(case["sc"], *GAPS)
    fits = ctx.calibrate_multi(case["qs"], freq=freq)
    S = [swg.evalue_min_score(p, residues, E) for p in fits]
    hits, n_total, _ = ctx.search_above_multi(db, case["qs"], S, cap=K)
    return fits, S, hits, n_total


def test_every_record_cut_at_its_own_evalue(swg, ctx, case):
    db = swg.Database(case["flat"], case["off"]).upload(ctx)
    residues = int(case["off"][-1])
    fits, S, hits, n_total = _library(swg, ctx, case, db, residues)
    r = _run(*SCORING, "--allqueries", "--evalue", "%g" % E, "--topk", str(K), "--tabular", "--files", case["qf"], case["df"])
    assert r.returncode == 0, r.stderr
    blocks = _records(r.stdout)
    assert sorted(blocks) == [0, 1, 2]
    for rec in range(3):
        lines, p = blocks[rec], fits[rec]
        assert p["status"] == 0 and S[rec] >= 1
        at = lines.index("Top %d hits (score, entry, name):" % len(hits[rec]))
        assert lines[at - 1] == "Entries at or above %d: %d" % (S[rec], n_total[rec]), (rec, lines[at - 1])
        assert lines[at - 2] == "E-value %g: lambda %.4f, K %.4f, least score %d over %d residues" % (E, p["lambda"], p["K"], S[rec], residues)
        assert lines[at + 1:at + 1 + len(hits[rec])] == ["%d\t%d\t%s" % (s, i, case["names"][i]) for s, i in hits[rec]], rec
        assert not any(l.startswith("Entry #") for l in lines), rec
        rows = lines[lines.index(HEAD13) + 1:][:len(hits[rec])]
        assert len(rows) == len(hits[rec]) > 0, rec
        for row, (s, i) in zip(rows, hits[rec]):
            f = row.split("\t")
            assert len(f) == 13 and f[0] == "rec%d" % rec and f[1] == case["names"][i] and int(f[12]) == s, row
            assert f[10] == "%.3g" % swg.evalue(p, residues, s) and f[11] == "%.1f" % swg.bitscore(p, s), (row, p)
            assert float(f[10]) <= E * 1.001
    assert hits[0][0][1] == 137 and swg.evalue(fits[0], residues, hits[0][0][0]) < 1e-6      # the relative, far below chance
    # without --evalue the table is the eleven columns it always was: the same rows less the two new columns
    lf = case["tmp"] / "scores.txt"
    lf.write_text("".join("%d\n" % s for s in S))
    r11 = _run(*SCORING, "--allqueries", "--minscorelist", str(lf), "--topk", str(K), "--tabular", "--files", case["qf"], case["df"])
    assert r11.returncode == 0, r11.stderr
    want = []
    for line in r.stdout.splitlines():
        if line.startswith("E-value "):
            continue
        f = line.split("\t")
        want.append(HEAD11 if line == HEAD13 else "\t".join(f[:10] + f[12:]) if len(f) == 13 else line)
    strip_time = lambda ls: [l for l in ls if not l.startswith("Total Time:")]
    assert strip_time(r11.stdout.splitlines()) == strip_time(want)
    assert HEAD13 not in r11.stdout and "E-value" not in r11.stdout
    db.close()


def test_one_query_over_listed_entries_with_their_composition(swg, ctx, case):
    """--seqidlist: E counts over the listed entries' residues, --compfromdb draws from their composition; --gpus 1 takes
    the shard-by-shard route to the same report."""
    members = list(range(0, 300, 2)) + [137]
    ids = case["tmp"] / "ids.txt"
    ids.write_text("".join("%d\n" % i for i in members))
    db = swg.Database(case["flat"], case["off"]).upload(ctx)
    view = db.view(ctx, members)
    ctx.set_scoring(case["sc"], *GAPS)
    ctx.set_query(case["qs"][0])
    p = ctx.calibrate(freq=view.composition(ctx))
    S = swg.evalue_min_score(p, view.residues, E)
    hits, n_total, _ = ctx.search_above(view, S)
    outs = []
    for extra in ([], ["--gpus", "1"]):
        r = _run(*SCORING, "--evalue", "%g" % E, "--compfromdb", "--seqidlist", str(ids), *extra, "--files", case["qf"], case["df"])
        assert r.returncode == 0, r.stderr
        lines = r.stdout.splitlines()
        at = lines.index("Top %d hits (score, entry, name):" % len(hits))
        assert lines[at - 1] == "Entries at or above %d: %d" % (S, n_total)
        assert lines[at - 2] == "E-value %g: lambda %.4f, K %.4f, least score %d over %d residues" % (E, p["lambda"], p["K"], S, view.residues)
        assert lines[at + 1:] == ["%d\t%d\t%s" % (s, i, case["names"][i]) for s, i in hits]
        outs.append(lines[at - 2:])
    assert outs[0] == outs[1] and p["lambda"] != ctx.calibrate()["lambda"]
    view.close()
    db.close()


def _check_block(swg, lines, p, S, residues, hits, n_total, names):
    at = lines.index("Top %d hits (score, entry, name):" % len(hits))
    assert lines[at - 1] == "Entries at or above %d: %d" % (S, n_total), lines[at - 1]
    assert lines[at - 2] == "E-value %g: lambda %.4f, K %.4f, least score %d over %d residues" % (E, p["lambda"], p["K"], S, residues), lines[at - 2]
    assert lines[at + 1:at + 1 + len(hits)] == ["%d\t%d\t%s" % (s, i, names[i]) for s, i in hits]


def test_the_gapless_score_and_records_with_their_own_pssms(swg, ctx, case):
    db = swg.Database(case["flat"], case["off"]).upload(ctx)
    residues = int(case["off"][-1])
    ctx.set_scoring(case["sc"], *GAPS)
    # --gapless: the first record, calibrated and searched by its gapless score
    ctx.set_query(case["qs"][0])
    p = ctx.calibrate(gapless=True)
    S = swg.evalue_min_score(p, residues, E)
    hits, n_total, _ = ctx.search_above(db, S, cap=K, gapless=True)
    r = _run(*SCORING, "--gapless", "--evalue", "%g" % E, "--topk", str(K), "--files", case["qf"], case["df"])
    assert r.returncode == 0, r.stderr
    _check_block(swg, r.stdout.splitlines(), p, S, residues, hits, n_total, case["names"])
    assert p["status"] == 0 and p["lambda"] != ctx.calibrate()["lambda"]
    # --pssmlist: every record against its own PSSM
    rng = np.random.default_rng(12)
    pssms, paths = [], []
    for rec, q in enumerate(case["qs"]):
        t20 = rng.integers(-8, 6, size=(32, 20))
        pf = case["tmp"] / ("r%d.pssm" % rec)
        write_ascii_pssm(pf, _letters(swg, q), t20[q.astype(np.int64)])
        pssm, pq = swg.read_pssm(str(pf), case["sc"])
        assert np.array_equal(pq, q)
        pssms.append(pssm)
        paths.append(pf)
    pl = case["tmp"] / "pssms.txt"
    pl.write_text("".join("%s\n" % f for f in paths))
    fits = ctx.calibrate_multi_pssm(pssms)
    Ss = [swg.evalue_min_score(f, residues, E) for f in fits]
    assert all(f["status"] == 0 for f in fits) and min(Ss) >= 1
    rows, totals, _ = ctx.search_above_multi_pssm(db, pssms, Ss, cap=K)
    r = _run(*SCORING, "--allqueries", "--pssmlist", str(pl), "--evalue", "%g" % E, "--topk", str(K), "--files", case["qf"], case["df"])
    assert r.returncode == 0, r.stderr
    blocks = _records(r.stdout)
    for rec in range(3):
        _check_block(swg, blocks[rec], fits[rec], Ss[rec], residues, rows[rec], totals[rec], case["names"])
    db.close()


def test_a_record_without_a_fit_is_refused_by_name(swg, case):
    qf = case["tmp"] / "flat.fasta"
    _write_fasta(qf, ["good one", "stars only"], [_letters(swg, case["qs"][1]), "*" * 40])
    r = _run(*SCORING, "--allqueries", "--evalue", "1", "--topk", "3", "--files", str(qf), case["df"])
    assert r.returncode != 0 and re.search(r"query #1 \(stars only\) has no E-value statistics", r.stderr), r.stderr[:300]
