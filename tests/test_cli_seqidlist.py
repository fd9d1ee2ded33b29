"""`smith_waterman --seqidlist FILE`: only the listed database entries are searched and reported (a view of the
resident database).  The list's checks and the help text need no GPU; the GPU case is BASELINE config 1's files
through the tool with a list, against the oracle."""
import re

import numpy as np
import pytest

from test_cli import B62, ENTRY_RX, _letters, _run, _write_fasta


def _small_files(tmp_path):
    q = tmp_path / "q.fa"
    q.write_text(">q\nACDEFGHIKL\n")
    d = tmp_path / "d.fa"
    d.write_text("".join(">s%d\nACDEFGHIKLMNPQ\n" % i for i in range(5)))
    return q, d


def test_help_names_the_flag(swg):
    r = _run("--help")
    assert r.returncode != 0 and "--seqidlist <file>" in r.stderr and "Entry #n" in r.stderr


@pytest.mark.parametrize("text,line,what", [("0\n3\n5\n", 3, "5"), ("# all of them\n\n1\n  2  # two\n-1\n", 5, "-1"),
                                            ("4\nfour\n", 2, "four"), ("1 2\n", 1, "1 2")])
def test_a_number_outside_the_database_is_a_usage_error(swg, tmp_path, text, line, what):
    q, d = _small_files(tmp_path)
    lst = tmp_path / "ids.txt"
    lst.write_text(text)
    r = _run("--substitution_matrix", B62, "--seqidlist", str(lst), "--files", str(q), str(d))
    assert r.returncode != 0 and "usage:" in r.stderr
    assert "--seqidlist %s line %d: '%s' is not an entry number of this database (0..4)" % (lst, line, what) in r.stderr


def test_list_file_errors(swg, tmp_path):
    q, d = _small_files(tmp_path)
    r = _run("--substitution_matrix", B62, "--seqidlist", str(tmp_path / "none.txt"), "--files", str(q), str(d))
    assert r.returncode != 0 and "couldn't open the entry list" in r.stderr
    r = _run("--substitution_matrix", B62, "--files", str(q), str(d), "--seqidlist")
    assert r.returncode != 0 and "Unknown argument without parameter: --seqidlist" in r.stderr


@pytest.mark.gpu
def test_cli_config1_with_a_list_against_oracle(swg, orc, tmp_path):
    sc = swg.load_scoring("BLOSUM62")
    q = swg.synth_query(0x5EED0001, 128)
    flat, off = swg.synth_db(0x5EED0001, 1024)
    seqs = [_letters(swg, flat[int(off[i]):int(off[i + 1])]) for i in range(1024)]
    names = ["db%d" % i for i in range(1024)]
    qf, df = tmp_path / "query.fasta", tmp_path / "db.fasta"
    _write_fasta(qf, ["query1"], [_letters(swg, q)])
    _write_fasta(df, names, seqs)
    want = orc.score_db(q, flat, off, sc.table(), -2, -1)
    rng = np.random.default_rng(4)
    sel = rng.choice(1024, size=200, replace=False)
    lst = tmp_path / "ids.txt"
    lst.write_text("# survivors of a prefilter\n" + "".join("%d\n" % i for i in sel) + "\n%d  # twice\n" % sel[0])
    listed = sorted(int(i) for i in sel)
    exp = [(-s, i) for s, i in sorted((-int(want[i]), i) for i in listed)[:5]]

    def check(r, n_align):
        assert r.returncode == 0, r.stderr
        got = [(int(m.group(1)), int(m.group(2))) for m in ENTRY_RX.finditer(r.stdout)]
        assert got == [(i, int(want[i])) for i in listed]                 # the listed entries only, in entry order
        assert "Total Entries: %d" % len(listed) in r.stdout
        lines = r.stdout.splitlines()
        top = lines[lines.index("Top 5 hits (score, entry, name):") + 1:][:5]
        assert [tuple(int(x) for x in t.split("\t")[:2]) for t in top] == exp
        al = [l for l in lines if l.startswith("Alignment #")]
        assert len(al) == n_align
        for l, (s_, i_) in zip(al, exp):
            m = re.match(r"Alignment #\d+: entry (\d+) score (-?\d+) query (\d+)\.\.(\d+) entry (\d+)\.\.(\d+)$", l)
            sc_, co, _ = orc.pair_trace(q, flat[int(off[i_]):int(off[i_ + 1])], sc.table(), -2, -1)
            assert (int(m.group(1)), int(m.group(2))) == (i_, s_) and sc_ == s_
            assert tuple(int(x) for x in m.groups()[2:]) == co

    pk = tmp_path / "db.swg"                   # (written in passing: the WHOLE database, the list does not cut the file)
    check(_run("--substitution_matrix", B62, "--seqidlist", str(lst), "--topk", "5", "--align", "--savedb", str(pk), "--files",
               str(qf), str(df)), 5)
    check(_run("--substitution_matrix", B62, "--seqidlist", str(lst), "--topk", "5", "--align", "--gpus", "1", "--files",
               str(qf), str(df)), 5)
    # a packed database, and every record of the query file: the same listed entries per query
    check(_run("--substitution_matrix", B62, "--seqidlist", str(lst), "--topk", "5", "--align", "--packed", "--files",
               str(qf), str(pk)), 5)
    q2 = swg.synth_query(77, 61)
    qf2 = tmp_path / "queries.fasta"
    _write_fasta(qf2, ["query1", "second"], [_letters(swg, q), _letters(swg, q2)])
    r = _run("--substitution_matrix", B62, "--seqidlist", str(lst), "--allqueries", "--files", str(qf2), str(df))
    assert r.returncode == 0, r.stderr
    blocks = re.split(r"^Query #\d+: .*$", r.stdout, flags=re.MULTILINE)
    for qq, text in ((q, blocks[1]), (q2, blocks[2])):
        w = orc.score_db(qq, flat, off, sc.table(), -2, -1)
        assert [(int(m.group(1)), int(m.group(2))) for m in ENTRY_RX.finditer(text)] == [(i, int(w[i])) for i in listed]
