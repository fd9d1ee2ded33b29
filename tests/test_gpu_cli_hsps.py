"""GPU (-m gpu): the `smith_waterman` tool's --maxhsps N / --hspscore S on the repeat case that is checkable by hand
(hsps_cases.REPEAT_EXPECTED): a unit of 7 distinct residues three times over against itself, +3 / -2, gaps -4 / -1,
alignments of at least 10 -- five of them, as --tabular lines, --align blocks and --bounds lines; the output without
--maxhsps, which must not depend on this feature; and --allqueries against the single-query runs."""
import pytest

import hsps_cases as hc
from test_cli import _letters, _run, _write_fasta

pytestmark = pytest.mark.gpu

LETTERS = "ARNDCQEGHILKMFPSTWYVBZX*"


@pytest.fixture(scope="module")
def repeat(swg, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("cli_hsps")
    mat = tmp / "match3_mismatch2.txt"
    rows = ["# +3 / -2", "   " + "  ".join(LETTERS)]
    rows += [a + " " + " ".join("%2d" % (3 if a == b else -2) for b in LETTERS) for a in LETTERS]
    mat.write_text("\n".join(rows) + "\n")
    seq = _letters(swg, hc.repeat_cases()[0]["query"])
    other = _letters(swg, hc.REPEAT_UNIT[::-1]) * 2 + _letters(swg, hc.REPEAT_UNIT)       # one unit in common, at its end
    qf, df, q2 = tmp / "q.fa", tmp / "db.fa", tmp / "q2.fa"
    _write_fasta(qf, ["rep"], [seq])
    _write_fasta(q2, ["rep", "other"], [seq, other])
    _write_fasta(df, ["decoy", "rep3 a repeat protein"], ["WWWWWWWWWWWWYYYYYYYYYYYY", seq])
    return {"mat": str(mat), "qf": str(qf), "q2": str(q2), "df": str(df), "seq": seq}


def run(repeat, *args, queries="qf"):
    r = _run("--substitution_matrix", repeat["mat"], "--gapopen", "-4", "--gapextend", "-1", *args, "--files", repeat[queries], repeat["df"])
    assert r.returncode == 0, r.stderr
    return r.stdout


def after(stdout, head):
    lines = stdout.splitlines()
    return lines[lines.index(head) + 1:]


FIELDS = "# Fields: query, entry, pident, length, mismatch, gapopen, qstart, qend, sstart, send, score"


def tab_lines(expected, query="rep", entry="rep3 a repeat protein"):
    return ["%s\t%s\t100.00\t%d\t0\t0\t%d\t%d\t%d\t%d\t%d" % (query, entry, n, qb + 1, qe, db + 1, de, sc) for sc, qb, qe, db, de, n in expected]


def test_tabular_prints_the_five_lines(repeat):
    out = run(repeat, "--topk", "1", "--maxhsps", "6", "--hspscore", "10", "--tabular")
    assert after(out, FIELDS) == tab_lines(hc.REPEAT_EXPECTED)
    assert "Top 1 hits (score, entry, name):\n63\t1\trep3 a repeat protein\n" in out
    # the cap, and the score (whose default is --minscore's)
    assert after(run(repeat, "--topk", "1", "--maxhsps", "2", "--hspscore", "10", "--tabular"), FIELDS) == tab_lines(hc.REPEAT_EXPECTED[:2])
    assert after(run(repeat, "--minscore", "22", "--maxhsps", "6", "--tabular"), FIELDS) == tab_lines(hc.REPEAT_EXPECTED[:3])
    assert after(run(repeat, "--minscore", "22", "--maxhsps", "6", "--hspscore", "1", "--tabular"), FIELDS)[:5] == tab_lines(hc.REPEAT_EXPECTED)


def test_align_prints_five_blocks(repeat):
    out = run(repeat, "--topk", "1", "--maxhsps", "6", "--hspscore", "10", "--align")
    lines = after(out, "63\t1\trep3 a repeat protein")
    want = []
    for sc, qb, qe, db, de, n in hc.REPEAT_EXPECTED:
        want += ["Alignment #0: entry 1 score %d query %d..%d entry %d..%d" % (sc, qb, qe, db, de), repeat["seq"][qb:qe], repeat["seq"][db:de], ""]
    assert lines == want


def test_bounds_prints_five_lines(repeat):
    out = run(repeat, "--topk", "1", "--maxhsps", "6", "--hspscore", "10", "--bounds")
    assert after(out, "63\t1\trep3 a repeat protein") == [
        "Bounds #0: entry 1 score %d query %d..%d entry %d..%d length %d" % e for e in hc.REPEAT_EXPECTED]


@pytest.mark.parametrize("report", ["--align", "--bounds", "--tabular"])
def test_one_hsp_at_score_one_prints_what_the_report_prints_without(repeat, report):
    """Without --maxhsps the output is the report's own (the existing CLI tests pin those bytes); with --maxhsps 1
    --hspscore 1 it is the same text, hit for hit."""
    plain = run(repeat, "--topk", "1", report)
    one = run(repeat, "--topk", "1", report, "--maxhsps", "1", "--hspscore", "1")
    strip = lambda s: [l for l in s.splitlines() if not l.startswith("Total Time:")]      # noqa: E731
    assert strip(one) == strip(plain)
    assert strip(run(repeat, "--topk", "1", report)) == strip(plain)


def test_allqueries_is_consistent_with_single_query_runs(repeat, tmp_path):
    both = run(repeat, "--allqueries", "--topk", "1", "--maxhsps", "6", "--hspscore", "7", "--tabular", queries="q2")
    blocks = both.split("Query #1: other\n")
    assert len(blocks) == 2
    first = run(repeat, "--topk", "1", "--maxhsps", "6", "--hspscore", "7", "--tabular")
    assert after(blocks[0], FIELDS) == after(first, FIELDS) == tab_lines(hc.REPEAT_EXPECTED)
    # the second record alone: a query file of its own
    q = tmp_path / "other.fa"
    rec = open(repeat["q2"]).read().split(">other\n")[1]
    q.write_text(">other\n" + rec)
    alone = _run("--substitution_matrix", repeat["mat"], "--gapopen", "-4", "--gapextend", "-1", "--topk", "1", "--maxhsps", "6", "--hspscore", "7",
                 "--tabular", "--files", str(q), repeat["df"])
    assert alone.returncode == 0, alone.stderr
    got = after(blocks[1], FIELDS)
    assert got == after(alone.stdout, FIELDS) and len(got) == 3        # its one unit against each of the entry's three
    assert [l.split("\t")[-1] for l in got] == ["21", "21", "21"]


def test_evalue_gives_each_line_its_own_evalue_and_bitscore(repeat):
    out = run(repeat, "--evalue", "10", "--maxhsps", "6", "--hspscore", "10", "--tabular")
    head = "# Fields: query, entry, pident, length, mismatch, gapopen, qstart, qend, sstart, send, evalue, bitscore, score"
    rows = [l.split("\t") for l in after(out, head)]
    assert [r[:10] for r in rows] == [l.split("\t")[:10] for l in tab_lines(hc.REPEAT_EXPECTED)]
    assert [int(r[12]) for r in rows] == [e[0] for e in hc.REPEAT_EXPECTED]
    ev, bits = [float(r[10]) for r in rows], [float(r[11]) for r in rows]
    assert ev[0] < ev[1] == ev[2] < ev[3] == ev[4] and bits[0] > bits[1] == bits[2] > bits[3] == bits[4]
