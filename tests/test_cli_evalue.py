"""CPU: the `smith_waterman` tool's --evalue E and --compfromdb -- their argument errors.  What they print is checked on
the GPU (tests/test_gpu_cli_evalue.py)."""
import pytest

from test_cli import B62, _run


@pytest.fixture()
def files(tmp_path):
    q = tmp_path / "q.fa"
    q.write_text(">q\nACDEFGHIKL\n")
    return str(q)


@pytest.mark.parametrize("value", ["0", "-1", "-1e-5", "x", "1e-3x", "", "nan", "inf"])
def test_evalue_must_be_a_number_above_zero(swg, files, value):
    r = _run("--substitution_matrix", B62, "--evalue", value, "--files", files, files)
    assert r.returncode != 0 and "Invalid --evalue argument" in r.stderr and "usage:" in r.stderr, (value, r.stderr[:200])


def test_evalue_needs_its_argument(swg, files):
    r = _run("--substitution_matrix", B62, "--files", files, files, "--evalue")
    assert r.returncode != 0 and "Unknown argument without parameter: --evalue" in r.stderr


@pytest.mark.parametrize("extra", [["--minscore", "12"], ["--allqueries", "--minscorelist", "nowhere.txt", "--topk", "3"]])
def test_evalue_is_exclusive_with_a_given_score(swg, files, extra):
    r = _run("--substitution_matrix", B62, "--evalue", "10", *extra, "--files", files, files)
    assert r.returncode != 0 and "--evalue derives the least score itself" in r.stderr and "usage:" in r.stderr, r.stderr[:200]


@pytest.mark.parametrize("extra", [["--prefilter", "10", "--topk", "5"], ["--allqueries", "--candidates", "nowhere.txt", "--topk", "3"]])
def test_evalue_does_not_combine_with_candidate_lists(swg, files, extra):
    r = _run("--substitution_matrix", B62, "--evalue", "10", *extra, "--files", files, files)
    assert r.returncode != 0 and "--evalue does not combine with --candidates or --prefilter" in r.stderr


def test_every_record_needs_topk(swg, files):
    r = _run("--substitution_matrix", B62, "--allqueries", "--evalue", "10", "--files", files, files)
    assert r.returncode != 0 and "--allqueries --evalue reports up to --topk K hits per record" in r.stderr


def test_compfromdb_needs_evalue(swg, files):
    r = _run("--substitution_matrix", B62, "--compfromdb", "--files", files, files)
    assert r.returncode != 0 and "--compfromdb chooses the background of --evalue's calibration" in r.stderr
    r = _run("--substitution_matrix", B62, "--compfromdb", "--minscore", "4", "--files", files, files)
    assert r.returncode != 0 and "give --evalue E" in r.stderr


def test_evalue_stands_in_for_topk_and_is_in_the_help(swg, files):
    for flag in ("--align", "--bounds", "--tabular"):
        r = _run("--substitution_matrix", B62, flag, "--evalue", "5", "--files", files, files)
        assert "give --topk K" not in r.stderr and "usage:" not in r.stderr, (flag, r.stderr[:200])
    r = _run("--help")
    assert "--evalue <E>" in r.stderr and "--compfromdb" in r.stderr
