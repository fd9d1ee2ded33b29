"""GPU (-m gpu): the `smith_waterman` tool's --allqueries --minscorelist F --topk K -- three query records against a small
FASTA database, each at its own least score -- against the oracle: every record's `Entries at or above` line and hit
block, plain, with --tabular, with --pssmlist, with --gapless and over --seqidlist's entries with --align and --bounds; a
list with too few lines fails and names the line."""
import re

import numpy as np
import pytest

import gapless_cases as gc
from test_cli import B62, _letters, _run, _write_fasta
from test_pssm_host import write_ascii_pssm

pytestmark = pytest.mark.gpu

K = 7


@pytest.fixture(scope="module")
def case(swg, orc, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("cli_above_multi")
    sc = swg.load_scoring("BLOSUM62")
    flat, off = swg.synth_db(0x5EED0001, 1024)
    keep = np.random.default_rng(2).permutation(1024)[:403]
    seqs = [_letters(swg, flat[int(off[i]):int(off[i + 1])]) for i in keep]
    names = ["db%d some description" % i for i in range(len(seqs))]
    qs = [swg.synth_query(0x5EED0D00 + r, L) for r, L in enumerate((128, 60, 90))]
    qf, df = tmp / "queries.fasta", tmp / "db.fasta"
    _write_fasta(qf, ["rec%d" % r for r in range(3)], [_letters(swg, q) for q in qs])
    _write_fasta(df, names, seqs)
    idx = [swg.letters_to_indices(s) for s in seqs]
    truths = [np.array([orc.pair(q, s, sc.table(), -2, -1) for s in idx], dtype=np.int64) for q in qs]
    # the 5th best (fewer hits than K), the 20th best (K cuts the list), above the best (no hit)
    S = [int(np.sort(truths[0])[-5]), int(np.sort(truths[1])[-20]), int(truths[2].max()) + 1]
    lf = tmp / "scores.txt"
    lf.write_text("".join("%d\n" % s for s in S))
    return dict(tmp=tmp, sc=sc, qf=str(qf), df=str(df), lf=str(lf), names=names, seqs=seqs, idx=idx, qs=qs, truths=truths, S=S)


def _expected(truth, S, members=None):
    members = range(len(truth)) if members is None else members
    return [(-s, i) for s, i in sorted((-int(truth[i]), i) for i in members if truth[i] >= S)]


def _records(stdout):
    """--allqueries stdout -> {record: its lines}."""
    blocks, cur = {}, None
    for line in stdout.splitlines():
        m = re.match(r"Query #(\d+): ", line)
        if m:
            cur = int(m.group(1))
            blocks[cur] = []
        elif cur is not None:
            blocks[cur].append(line)
    return blocks


def _check_records(case, stdout, truths, members=None):
    blocks = _records(stdout)
    assert sorted(blocks) == [0, 1, 2]
    counts = []
    for r, truth in enumerate(truths):
        exp = _expected(truth, case["S"][r], members)
        lines = blocks[r]
        at = lines.index("Top %d hits (score, entry, name):" % min(K, len(exp)))
        assert lines[at - 1] == "Entries at or above %d: %d" % (case["S"][r], len(exp)), (r, lines[at - 1])
        assert lines[at - 2] == "Total Entries: %d" % (len(truth) if members is None else len(members))
        assert lines[at + 1:at + 1 + min(K, len(exp))] == ["%d\t%d\t%s" % (s, i, case["names"][i]) for s, i in exp[:K]], r
        assert not any(l.startswith("Entry #") for l in lines), r
        counts.append(len(exp))
    return blocks, counts


def test_every_record_at_its_own_score(swg, case):
    r = _run("--substitution_matrix", B62, "--allqueries", "--minscorelist", case["lf"], "--topk", str(K), "--files", case["qf"], case["df"])
    assert r.returncode == 0, r.stderr
    _, counts = _check_records(case, r.stdout, case["truths"])
    assert 0 < counts[0] < K < counts[1] and counts[2] == 0


def test_tabular(swg, orc, case):
    r = _run("--substitution_matrix", B62, "--allqueries", "--minscorelist", case["lf"], "--topk", str(K), "--tabular", "--files", case["qf"],
             case["df"])
    assert r.returncode == 0, r.stderr
    blocks, _ = _check_records(case, r.stdout, case["truths"])
    head = "# Fields: query, entry, pident, length, mismatch, gapopen, qstart, qend, sstart, send, score"
    for rec in (0, 1):
        exp = _expected(case["truths"][rec], case["S"][rec])[:K]
        lines = blocks[rec]
        rows = lines[lines.index(head) + 1:][:len(exp)]
        assert len(rows) == len(exp)
        for row, (s, i) in zip(rows, exp):
            f = row.split("\t")
            want_sc, (qb, qe, db_, de), ops = orc.pair_trace(case["qs"][rec], case["idx"][i], case["sc"].table(), -2, -1)
            assert f[0] == "rec%d" % rec and f[1] == case["names"][i] and int(f[10]) == s == want_sc, row
            assert (int(f[6]), int(f[7]), int(f[8]), int(f[9])) == (qb + 1, qe, db_ + 1, de) and int(f[3]) == len(ops), row
    assert head not in blocks[2]                               # (no hit: no table)


def test_pssmlist(swg, orc, case):
    """Every record's PSSM scores a position by its residue through a table of the record's own, so the oracle checks it."""
    tmp, sc = case["tmp"], case["sc"]
    rng = np.random.default_rng(11)
    truths, paths = [], []
    for r, q in enumerate(case["qs"]):
        t20 = rng.integers(-6, 9, size=(32, 20))
        pf = tmp / ("r%d.pssm" % r)
        write_ascii_pssm(pf, _letters(swg, q), t20[q.astype(np.int64)])
        pssm, pq = swg.read_pssm(str(pf), sc)
        assert np.array_equal(pq, q)
        subp = np.zeros((32, 32), dtype=np.int8)
        subp[q.astype(np.int64)] = pssm
        assert np.array_equal(subp[q.astype(np.int64)], pssm)
        truths.append(np.array([orc.pair(q, s, subp, -2, -1) for s in case["idx"]], dtype=np.int64))
        paths.append(pf)
    S = [int(np.sort(truths[0])[-5]), int(np.sort(truths[1])[-20]), int(truths[2].max()) + 1]
    lf, pl = tmp / "pssm_scores.txt", tmp / "pssms.txt"
    lf.write_text("".join("%d\n" % s for s in S))
    pl.write_text("".join("%s\n" % p for p in paths))
    r = _run("--substitution_matrix", B62, "--allqueries", "--pssmlist", str(pl), "--minscorelist", str(lf), "--topk", str(K), "--files",
             case["qf"], case["df"])
    assert r.returncode == 0, r.stderr
    _check_records(dict(case, S=S), r.stdout, truths)


def test_gapless(swg, orc, case):
    truths = [np.array([orc.pair(q, s, case["sc"].table(), *gc.PRICED_OUT) for s in case["idx"]], dtype=np.int64) for q in case["qs"]]
    S = [int(np.sort(truths[0])[-5]), int(np.sort(truths[1])[-20]), int(truths[2].max()) + 1]
    lf = case["tmp"] / "gapless_scores.txt"
    lf.write_text("".join("%d\n" % s for s in S))
    r = _run("--substitution_matrix", B62, "--allqueries", "--gapless", "--minscorelist", str(lf), "--topk", str(K), "--files", case["qf"],
             case["df"])
    assert r.returncode == 0, r.stderr
    _check_records(dict(case, S=S), r.stdout, truths)


def test_listed_entries_aligned_and_bounded(swg, case):
    """--seqidlist: every record's count and hits are those of the listed entries; --align and --bounds report exactly
    each record's hits, in order, with their scores."""
    members = list(range(0, len(case["seqs"]), 2))
    ids = case["tmp"] / "ids.txt"
    ids.write_text("".join("%d\n" % i for i in members))
    for flag, rx in (("--align", r"Alignment #\d+: entry (\d+) score (-?\d+) "), ("--bounds", r"Bounds #\d+: entry (\d+) score (-?\d+) ")):
        r = _run("--substitution_matrix", B62, "--allqueries", "--seqidlist", str(ids), "--minscorelist", case["lf"], "--topk", str(K), flag,
                 "--files", case["qf"], case["df"])
        assert r.returncode == 0, r.stderr
        blocks, counts = _check_records(case, r.stdout, case["truths"], members)
        assert counts[0] > 0 and counts[1] > K
        for rec in range(3):
            exp = _expected(case["truths"][rec], case["S"][rec], members)[:K]
            got = [tuple(int(x) for x in re.match(rx, l).groups()) for l in blocks[rec] if re.match(rx, l)]
            assert got == [(i, s) for s, i in exp], (flag, rec)


def test_a_list_with_too_few_lines_names_the_line(swg, case):
    short = case["tmp"] / "short.txt"
    short.write_text("%d\n%d\n" % (case["S"][0], case["S"][1]))
    r = _run("--substitution_matrix", B62, "--allqueries", "--minscorelist", str(short), "--topk", str(K), "--files", case["qf"], case["df"])
    assert r.returncode != 0 and "--minscorelist %s line 3 is missing" % short in r.stderr, r.stderr[:300]
