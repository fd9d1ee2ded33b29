"""GPU (-m gpu): the tool's --gapless output and the --prefilter pipeline (gapless top-N -> swg_search_lists -> --topk
block and --align alignments), on config 1's files (query of 128 residues, 1024 synthetic sequences)."""
import os
import re
import subprocess

import numpy as np
import pytest

import gapless_cases as gc
from conftest import ROOT
from test_cli import B62, ENTRY_RX, _letters, _write_fasta

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "seq-align-gpu_amd", "bin", "smith_waterman")
ALIGN_RX = re.compile(r"^Alignment #(\d+): entry (\d+) score (-?\d+) ", re.MULTILINE)


def _run(*args):
    return subprocess.run([CLI] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)


def _top_block(stdout):
    lines = stdout.splitlines()
    blocks, i = [], 0
    while i < len(lines):
        m = re.match(r"Top (\d+) hits \(score, entry, name\):", lines[i])
        if m:
            blocks.append(lines[i:i + 1 + int(m.group(1))])
        i += 1
    return blocks


def test_cli_gapless_and_prefilter(swg, orc, tmp_path):
    sc = swg.load_scoring("BLOSUM62")
    flat, off = swg.synth_db(0x5EED0001, 1024)
    n = len(off) - 1
    queries = [swg.synth_query(0x5EED0001, 128), swg.synth_query(77, 90), swg.synth_query(78, 200)]
    seqs = [_letters(swg, flat[int(off[i]):int(off[i + 1])]) for i in range(n)]
    names = ["db%d" % i for i in range(n)]
    qf, qf3, df = tmp_path / "query.fasta", tmp_path / "queries.fasta", tmp_path / "db.fasta"
    _write_fasta(qf, ["query1"], [_letters(swg, queries[0])])
    _write_fasta(qf3, ["q%d" % i for i in range(3)], [_letters(swg, q) for q in queries])
    _write_fasta(df, names, seqs)
    base = ["--substitution_matrix", B62, "--gapopen", "-10", "--gapextend", "-1"]

    # --gapless: the Entry stream holds the gapless scores, the --topk block their order
    r = _run(*base, "--gapless", "--topk", "10", "--files", str(qf), str(df))
    assert r.returncode == 0, r.stderr
    want = gc.oracle_gapless(orc, queries[0], flat, off, sc.table())
    got = {int(m.group(1)): int(m.group(2)) for m in ENTRY_RX.finditer(r.stdout)}
    assert got == {i: int(v) for i, v in enumerate(want)}
    assert _top_block(r.stdout)[0][1:] == ["%d\t%d\t%s" % (s, i, names[i]) for s, i in gc.expected_hits(want, 10)]

    # --prefilter with every entry as a candidate: exactly the --topk block of the plain run, and no Entry stream
    full = _run(*base, "--topk", "10", "--files", str(qf), str(df))
    assert full.returncode == 0, full.stderr
    gapped = {int(m.group(1)): int(m.group(2)) for m in ENTRY_RX.finditer(full.stdout)}
    r = _run(*base, "--prefilter", str(n), "--topk", "10", "--timing", "--files", str(qf), str(df))
    assert r.returncode == 0, r.stderr
    assert _top_block(r.stdout) == _top_block(full.stdout) and "Entry #" not in r.stdout
    assert "prefilter" in r.stderr
    # 50 candidates: every printed hit carries the full search's score of its entry
    r = _run(*base, "--prefilter", "50", "--topk", "10", "--files", str(qf), str(df))
    assert r.returncode == 0, r.stderr
    block = _top_block(r.stdout)[0]
    assert len(block) == 11
    for line in block[1:]:
        s, i, _ = line.split("\t")
        assert gapped[int(i)] == int(s), line

    # every record of a query file, with alignments
    r = _run(*base, "--allqueries", "--prefilter", "50", "--topk", "5", "--align", "--files", str(qf3), str(df))
    assert r.returncode == 0, r.stderr
    blocks = _top_block(r.stdout)
    assert len(blocks) == 3 and "Entry #" not in r.stdout
    al = [(int(a), int(e), int(s)) for a, e, s in ALIGN_RX.findall(r.stdout)]
    assert len(al) == 15
    for qi, q in enumerate(queries):
        truth = orc.score_db(q, flat, off, sc.table(), -10, -1)
        for rank, line in enumerate(blocks[qi][1:]):
            s, i, _ = line.split("\t")
            assert int(truth[int(i)]) == int(s), (qi, line)
            assert al[qi * 5 + rank] == (rank, int(i), int(s)), (qi, rank)
