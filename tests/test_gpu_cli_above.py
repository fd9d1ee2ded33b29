"""GPU (-m gpu): the `smith_waterman` tool's --minscore S on BASELINE config 1 -- a 128-aa query against a 1k-sequence
synthetic database -- against the oracle: every entry at or above S, best first (ties by entry number), in --topk's
block; alone, with --tabular, cut by --topk K, aligned, and through the shard-by-shard route of --gpus."""
import re

import numpy as np
import pytest

from test_cli import B62, _letters, _run, _write_fasta

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def config1(swg, orc, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("cli_above")
    sc = swg.load_scoring("BLOSUM62")
    q = swg.synth_query(0x5EED0001, 128)
    flat, off = swg.synth_db(0x5EED0001, 1024)
    keep = np.random.default_rng(1).permutation(1024)[:1003]
    seqs = [_letters(swg, flat[int(off[i]):int(off[i + 1])]) for i in keep]
    names = ["db%d some description" % i for i in range(len(seqs))]
    qf, df = tmp / "query.fasta", tmp / "db.fasta"
    _write_fasta(qf, ["query1"], [_letters(swg, q)])
    _write_fasta(df, names, seqs)
    truth = np.array([orc.pair(q, swg.letters_to_indices(s), sc.table(), -2, -1) for s in seqs], dtype=np.int64)
    return {"qf": str(qf), "df": str(df), "names": names, "seqs": seqs, "q": q, "truth": truth, "table": sc.table()}


def _expected(truth, S):
    return [(-s, i) for s, i in sorted((-int(v), i) for i, v in enumerate(truth) if v >= S)]


def _block(stdout, n):
    lines = stdout.splitlines()
    at = lines.index("Top %d hits (score, entry, name):" % n)
    return lines, at, lines[at + 1:at + 1 + n]


def test_minscore_alone_and_cut_by_topk(swg, config1):
    truth, names = config1["truth"], config1["names"]
    S = int(np.sort(truth)[-40])                       # the 40th best score: ties come with it
    exp = _expected(truth, S)
    assert 40 <= len(exp) < len(truth)
    r = _run("--substitution_matrix", B62, "--minscore", str(S), "--files", config1["qf"], config1["df"])
    assert r.returncode == 0, r.stderr
    lines, at, block = _block(r.stdout, len(exp))
    assert block == ["%d\t%d\t%s" % (s, i, names[i]) for s, i in exp]
    assert lines[at - 1] == "Entries at or above %d: %d" % (S, len(exp)) and lines[at - 2] == "Total Entries: %d" % len(truth)
    assert "Entry #" not in r.stdout and len(lines) == at + 1 + len(exp)
    # the best 7 of them; the count is still all of them
    r = _run("--substitution_matrix", B62, "--minscore", str(S), "--topk", "7", "--files", config1["qf"], config1["df"])
    assert r.returncode == 0, r.stderr
    lines, at, block = _block(r.stdout, 7)
    assert block == ["%d\t%d\t%s" % (s, i, names[i]) for s, i in exp[:7]]
    assert lines[at - 1] == "Entries at or above %d: %d" % (S, len(exp))
    # above every score: an empty block
    r = _run("--substitution_matrix", B62, "--minscore", str(int(truth.max()) + 1), "--files", config1["qf"], config1["df"])
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines()[-2:] == ["Entries at or above %d: 0" % (int(truth.max()) + 1), "Top 0 hits (score, entry, name):"]


def test_minscore_tabular(swg, orc, config1):
    truth, names, seqs, q = config1["truth"], config1["names"], config1["seqs"], config1["q"]
    S = int(np.sort(truth)[-12])
    exp = _expected(truth, S)
    r = _run("--substitution_matrix", B62, "--minscore", str(S), "--tabular", "--files", config1["qf"], config1["df"])
    assert r.returncode == 0, r.stderr
    lines, at, block = _block(r.stdout, len(exp))
    assert block == ["%d\t%d\t%s" % (s, i, names[i]) for s, i in exp]
    rows = lines[lines.index("# Fields: query, entry, pident, length, mismatch, gapopen, qstart, qend, sstart, send, score") + 1:]
    assert len(rows) == len(exp)
    for row, (s, i) in zip(rows, exp):
        f = row.split("\t")
        want_sc, (qb, qe, db_, de), ops = orc.pair_trace(q, swg.letters_to_indices(seqs[i]), config1["table"], -2, -1)
        assert f[0] == "query1" and f[1] == names[i] and int(f[10]) == s == want_sc, row
        assert (int(f[6]), int(f[7]), int(f[8]), int(f[9])) == (qb + 1, qe, db_ + 1, de) and int(f[3]) == len(ops), row


def test_minscore_through_the_shards_route(swg, config1):
    """--gpus 1: the shard-by-shard route (one device here) gives the single-GPU block, and aligns its hits."""
    truth, names = config1["truth"], config1["names"]
    S = int(np.sort(truth)[-5])
    exp = _expected(truth, S)
    r = _run("--substitution_matrix", B62, "--gpus", "1", "--minscore", str(S), "--align", "--files", config1["qf"], config1["df"])
    assert r.returncode == 0, r.stderr
    lines, at, block = _block(r.stdout, len(exp))
    assert block == ["%d\t%d\t%s" % (s, i, names[i]) for s, i in exp]
    heads = [l for l in lines if l.startswith("Alignment #")]
    assert [tuple(int(x) for x in re.match(r"Alignment #\d+: entry (\d+) score (-?\d+) ", h).groups()) for h in heads] == [(i, s) for s, i in exp]
