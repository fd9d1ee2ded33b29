"""`smith_waterman --allqueries --candidates FILE`: every query record against its own database entries, all records in
one pass (swg_search_lists).  The file's checks, the usage errors and the help text need no GPU; the GPU case runs four
query records with lists against a 1 024-sequence synthetic FASTA and compares what is printed with the oracle."""
import re

import numpy as np
import pytest

from test_cli import B62, ENTRY_RX, _letters, _run, _write_fasta


def _small_files(tmp_path):
    q = tmp_path / "q.fa"
    q.write_text(">q0\nACDEFGHIKL\n>q1\nMNPQRSTVWY\n>q2\nACDMNPQ\n")
    d = tmp_path / "d.fa"
    d.write_text("".join(">s%d\nACDEFGHIKLMNPQ\n" % i for i in range(5)))
    return q, d


def test_help_names_the_flag(swg):
    r = _run("--help")
    assert r.returncode != 0 and "--candidates <file>" in r.stderr and "query_record_number entry_number" in r.stderr


@pytest.mark.parametrize("extra,what", [
    ((), "give --allqueries"),
    (("--allqueries", "--gpus", "1"), "one GPU"),
    (("--allqueries", "--seqidlist", "IDS"), "--candidates and --seqidlist do not combine"),
    (("--pssm", "PSSM"), "--candidates"),
])
def test_usage_errors(swg, tmp_path, extra, what):
    q, d = _small_files(tmp_path)
    lst = tmp_path / "cand.txt"
    lst.write_text("0 1\n")
    ids = tmp_path / "ids.txt"
    ids.write_text("1\n")
    extra = tuple(str(ids) if e == "IDS" else str(tmp_path / "none.pssm") if e == "PSSM" else e for e in extra)
    r = _run("--substitution_matrix", B62, "--candidates", str(lst), *extra, "--files", str(q), str(d))
    assert r.returncode != 0 and "usage:" in r.stderr and what in r.stderr


@pytest.mark.parametrize("text,line,what,kind", [
    ("0 1\n2 4\n3 0\n", 3, "3", "query"),
    ("# pairs\n\n1 2\n  2   3  # fine\n-1 2\n", 5, "-1", "query"),
    ("0 5\n", 1, "5", "entry"),
    ("1 1\n2 four\n", 2, "four", "entry"),
    ("1\n", 1, "", "entry"),
    ("0 1 2\n", 1, "1 2", "entry"),
])
def test_a_number_outside_the_files_is_a_usage_error(swg, tmp_path, text, line, what, kind):
    q, d = _small_files(tmp_path)
    lst = tmp_path / "cand.txt"
    lst.write_text(text)
    r = _run("--substitution_matrix", B62, "--allqueries", "--candidates", str(lst), "--files", str(q), str(d))
    assert r.returncode != 0 and "usage:" in r.stderr
    tail = ("is not a query record number of this query file (0..2)" if kind == "query"
            else "is not an entry number of this database (0..4)")
    assert "--candidates %s line %d: '%s' %s" % (lst, line, what, tail) in r.stderr


def test_list_file_errors(swg, tmp_path):
    q, d = _small_files(tmp_path)
    r = _run("--substitution_matrix", B62, "--allqueries", "--candidates", str(tmp_path / "none.txt"), "--files", str(q), str(d))
    assert r.returncode != 0 and "couldn't open the candidate list" in r.stderr
    r = _run("--substitution_matrix", B62, "--allqueries", "--files", str(q), str(d), "--candidates")
    assert r.returncode != 0 and "Unknown argument without parameter: --candidates" in r.stderr


@pytest.mark.gpu
def test_cli_four_records_with_lists_against_oracle(swg, orc, tmp_path):
    sc = swg.load_scoring("BLOSUM62")
    flat, off = swg.synth_db(0x5EED0001, 1024)
    seqs = [_letters(swg, flat[int(off[i]):int(off[i + 1])]) for i in range(1024)]
    qs = [swg.synth_query(0x5EED0001, 128), swg.synth_query(78, 61), swg.synth_query(79, 200), swg.synth_query(80, 33)]
    qf, df = tmp_path / "queries.fasta", tmp_path / "db.fasta"
    _write_fasta(qf, ["query%d" % i for i in range(4)], [_letters(swg, q) for q in qs])
    _write_fasta(df, ["db%d" % i for i in range(1024)], seqs)
    want = [orc.score_db(q, flat, off, sc.table(), -2, -1) for q in qs]
    rng = np.random.default_rng(14)
    lists = [rng.choice(1024, size=150, replace=False), rng.choice(1024, size=7, replace=False), np.zeros(0, dtype=np.int64),
             rng.choice(1024, size=301, replace=False)]
    lines = [(qi, int(e)) for qi, l in enumerate(lists) for e in l] + [(0, int(lists[0][0]))]      # one pair twice
    order = rng.permutation(len(lines))                       # records interleaved: the file need not be grouped
    lst = tmp_path / "cand.txt"
    lst.write_text("# survivors of a prefilter, per query\n\n" + "".join("%d %d\n" % lines[i] for i in order) + "  # end\n")
    pk = tmp_path / "db.swg"

    def check(r, names):
        assert r.returncode == 0, r.stderr
        blocks = re.split(r"^Query #\d+: .*$", r.stdout, flags=re.MULTILINE)
        assert len(blocks) == 5
        for qi, text in enumerate(blocks[1:]):
            listed = sorted(int(i) for i in lists[qi])
            got = [(int(m.group(1)), int(m.group(2))) for m in ENTRY_RX.finditer(text)]
            assert got == [(i, int(want[qi][i])) for i in listed], qi             # its own entries only, in entry order
            assert "Total Entries: %d\n" % len(listed) in text
            exp = [(-s, i) for s, i in sorted((-int(want[qi][i]), i) for i in listed)[:5]]
            tl = text.splitlines()
            top = tl[tl.index("Top %d hits (score, entry, name):" % len(exp)) + 1:][:len(exp)]
            assert [tuple(int(x) for x in t.split("\t")[:2]) for t in top] == exp, qi
            if names:
                assert [t.split("\t")[2] for t in top] == ["db%d" % i for _, i in exp]
            al = [l for l in tl if l.startswith("Alignment #")]
            assert len(al) == len(exp)
            for l, (s_, i_) in zip(al, exp):
                m = re.match(r"Alignment #\d+: entry (\d+) score (-?\d+) ", l)
                assert (int(m.group(1)), int(m.group(2))) == (i_, s_)

    check(_run("--substitution_matrix", B62, "--allqueries", "--candidates", str(lst), "--topk", "5", "--align", "--savedb", str(pk),
               "--files", str(qf), str(df)), True)
    check(_run("--substitution_matrix", B62, "--allqueries", "--candidates", str(lst), "--topk", "5", "--align", "--packed", "--files",
               str(qf), str(pk)), False)
