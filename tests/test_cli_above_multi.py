"""CPU: the `smith_waterman` tool's --allqueries --minscorelist F --topk K (every record's entries at or above its own
score: swg_search_above_multi) -- the usage errors the tool can tell before it needs a device.  What it prints is checked
on the GPU (tests/test_gpu_cli_above_multi.py)."""
import pytest

from test_cli import B62, _run


@pytest.fixture()
def files(tmp_path):
    q = tmp_path / "q.fa"
    q.write_text(">q0\nACDEFGHIKL\n>q1\nLKIHGFEDCA\n")
    lst = tmp_path / "scores.txt"
    lst.write_text("10\n12\n")
    return str(q), str(lst)


def test_minscorelist_needs_allqueries_and_topk(swg, files):
    q, lst = files
    r = _run("--substitution_matrix", B62, "--minscorelist", lst, "--topk", "5", "--files", q, q)
    assert r.returncode != 0 and "usage:" in r.stderr and "--minscorelist" in r.stderr and "give --allqueries" in r.stderr
    r = _run("--substitution_matrix", B62, "--allqueries", "--minscorelist", lst, "--files", q, q)
    assert r.returncode != 0 and "usage:" in r.stderr and "--minscorelist" in r.stderr and "give --topk K" in r.stderr
    r = _run("--substitution_matrix", B62, "--allqueries", "--topk", "5", "--files", q, q, "--minscorelist")
    assert r.returncode != 0 and "Unknown argument without parameter: --minscorelist" in r.stderr


@pytest.mark.parametrize("extra", [["--candidates", "c.txt"], ["--prefilter", "10"], ["--gpus", "2"]])
def test_minscorelist_does_not_combine(swg, files, extra):
    q, lst = files
    r = _run("--substitution_matrix", B62, "--allqueries", "--minscorelist", lst, "--topk", "5", *extra, "--files", q, q)
    assert r.returncode != 0 and "usage:" in r.stderr, r.stderr[:200]
    assert "--minscorelist" in r.stderr.split("usage:")[0] or "--allqueries work with one GPU" in r.stderr, r.stderr[:300]


def test_minscorelist_with_minscore(swg, files):
    """Both at once is a usage error (the list needs --allqueries, which --minscore refuses: either message names the clash)."""
    q, lst = files
    r = _run("--substitution_matrix", B62, "--allqueries", "--minscorelist", lst, "--minscore", "10", "--topk", "5", "--files", q, q)
    assert r.returncode != 0 and "usage:" in r.stderr
    assert "--minscorelist does not combine with --minscore" in r.stderr or "--minscore reports one query's hits" in r.stderr


def test_the_old_refusal_is_unchanged(swg, files):
    q, _ = files
    r = _run("--substitution_matrix", B62, "--minscore", "10", "--allqueries", "--files", q, q)
    assert r.returncode != 0
    assert "--minscore reports one query's hits: it does not combine with --allqueries, --candidates or --prefilter" in r.stderr


@pytest.mark.parametrize("text,line,what", [
    ("10\n", 2, "is missing"),                      # too few lines: the first one that is not there
    ("10\n12\n14\n", 3, "2 records"),               # too many
    ("10\n0\n", 2, "'0' is not a least score"),     # below 1
    ("x\n12\n", 1, "'x' is not a least score"),
    ("10\n\n12\n", 2, "'' is not a least score"),   # an empty line is a line
    ("10\n1.5\n", 2, "'1.5' is not a least score"),
])
def test_the_list_itself(swg, files, tmp_path, text, line, what):
    """A wrong number of lines or a bad value: an error that names the line, before any device is needed."""
    q, _ = files
    lst = tmp_path / "bad.txt"
    lst.write_text(text)
    r = _run("--substitution_matrix", B62, "--allqueries", "--minscorelist", str(lst), "--topk", "5", "--files", q, q)
    assert r.returncode != 0 and "--minscorelist %s line %d" % (lst, line) in r.stderr and what in r.stderr, r.stderr[:300]
    r = _run("--substitution_matrix", B62, "--allqueries", "--minscorelist", str(tmp_path / "none.txt"), "--topk", "5", "--files", q, q)
    assert r.returncode != 0 and "couldn't open the score list" in r.stderr


def test_help_names_the_option(swg):
    r = _run("--help")
    assert "--minscorelist <file>" in r.stderr and "--minscore <S>" in r.stderr
