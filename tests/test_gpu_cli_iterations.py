"""GPU (-m gpu): `smith_waterman --iterations 2` on the end-to-end fixture of test_pssm_build_host.py -- the hit list it
prints is the one pinned with the oracle and the numpy PSSM scorer, and its --out_pssm file holds the library's PSSM."""
import re

import numpy as np
import pytest

import pssm_build_cases as pc
from test_cli import B62, _letters, _run, _write_fasta
from test_gpu_parity import _reset_options
from test_pssm_build_host import e2e_cpu

pytestmark = pytest.mark.gpu

GAPS = pc.MATRICES["BLOSUM62"]
# E = 0.01 is a least score of about 59 for this query and database: between the family's 47 and 64, where the pinned
# inclusion score of 60 cuts (the default, 0.002, is a score of 65)
INCLUSION = 0.01
CALIB = {"calib_seqs": 8192, "calib_len": 384, "calib_seed": 1}      # the tool runs on the library's defaults


@pytest.fixture(autouse=True)
def _options(ctx):
    _reset_options(ctx)
    for key, v in CALIB.items():
        ctx.set_option(key, v)
    yield
    _reset_options(ctx)


def _top_block(stdout):
    lines = stdout.splitlines()
    at = next(i for i, l in enumerate(lines) if re.match(r"Top \d+ hits", l))
    n = int(re.match(r"Top (\d+) hits", lines[at]).group(1))
    return [(int(l.split("\t")[0]), int(l.split("\t")[1])) for l in lines[at + 1:at + 1 + n]]


def test_two_iterations_print_the_pinned_hits_and_write_the_librarys_pssm(swg, orc, ctx, tmp_path):
    e = e2e_cpu()
    n = len(e["off"]) - 1
    qf, dbf, out = tmp_path / "q.fa", tmp_path / "db.fa", tmp_path / "it.pssm"
    _write_fasta(str(qf), ["query"], [_letters(swg, e["q"])])
    _write_fasta(str(dbf), ["s%d" % i for i in range(n)], [_letters(swg, e["flat"][int(e["off"][i]):int(e["off"][i + 1])]) for i in range(n)])
    r = _run("--substitution_matrix", B62, "--gapopen", str(GAPS[0]), "--gapextend", str(GAPS[1]), "--iterations", "2", "--topk", str(pc.E2E["top"]),
             "--inclusion", str(INCLUSION), "--out_pssm", str(out), "--files", str(qf), str(dbf))
    assert r.returncode == 0, r.stderr[-400:]
    print(r.stderr)
    # the library, step by step as the tool takes them
    sub = pc.table("BLOSUM62")
    ctx.set_scoring(sub, *GAPS)
    ctx.set_query(e["q"])
    db = swg.Database(e["flat"], e["off"]).upload(ctx)
    least = swg.evalue_min_score(ctx.calibrate(), int(e["off"][-1]), INCLUSION)
    included, n_at, _ = ctx.search_above(db, least, cap=500)
    assert "iteration 1: %d entries at or above score %d" % (n_at, least) in r.stderr
    assert [i for _, i in included] == e["included"], "the inclusion threshold (score %d) cuts the family elsewhere than the pinned score does" % least
    pssm, _, _ = ctx.build_pssm(db, included)
    assert np.array_equal(pssm, e["pssm"])
    got = _top_block(r.stdout)
    assert got == orc.topk(e["scores2"], pc.E2E["top"])               # the pinned list: the numpy PSSM scorer's, by the CPU alone
    back, q = swg.read_pssm(str(out), swg.load_scoring("BLOSUM62"))
    assert np.array_equal(back, pssm) and np.array_equal(q, e["q"])
    db.close()


def test_an_iteration_that_adds_nothing_ends_the_run(swg, ctx, tmp_path):
    e = e2e_cpu()
    n = len(e["off"]) - 1
    qf, dbf = tmp_path / "q.fa", tmp_path / "db.fa"
    _write_fasta(str(qf), ["query"], [_letters(swg, e["q"])])
    _write_fasta(str(dbf), ["s%d" % i for i in range(n)], [_letters(swg, e["flat"][int(e["off"][i]):int(e["off"][i + 1])]) for i in range(n)])
    r = _run("--substitution_matrix", B62, "--gapopen", str(GAPS[0]), "--gapextend", str(GAPS[1]), "--iterations", "8", "--topk", "5",
             "--inclusion", str(INCLUSION), "--files", str(qf), str(dbf))
    assert r.returncode == 0, r.stderr[-400:]
    print(r.stderr)
    # 30 family members, 24 of them included by the first iteration: the included set can grow three times at the most
    assert "the iterations end here" in r.stderr and "iteration 6:" not in r.stderr
    assert len(_top_block(r.stdout)) == 5
