"""CPU: the `smith_waterman` tool's --minscore S (every entry that scores at least S: swg_search_above) -- its argument
errors.  What it prints is checked on the GPU (tests/test_gpu_cli_above.py)."""
import pytest

from test_cli import B62, _run


@pytest.fixture()
def files(tmp_path):
    q = tmp_path / "q.fa"
    q.write_text(">q\nACDEFGHIKL\n")
    return str(q)


@pytest.mark.parametrize("value", ["0", "-5", "x", "12x", "", "1.5", "99999999999"])
def test_minscore_values_below_one_or_not_a_number_are_usage_errors(swg, files, value):
    r = _run("--substitution_matrix", B62, "--minscore", value, "--files", files, files)
    assert r.returncode != 0 and "Invalid --minscore argument" in r.stderr and "usage:" in r.stderr, (value, r.stderr[:200])


def test_minscore_needs_its_argument(swg, files):
    r = _run("--substitution_matrix", B62, "--files", files, files, "--minscore")
    assert r.returncode != 0 and "Unknown argument without parameter: --minscore" in r.stderr


@pytest.mark.parametrize("extra", [["--allqueries"], ["--prefilter", "10", "--topk", "5"]])
def test_minscore_does_not_combine_with_batches(swg, files, extra):
    r = _run("--substitution_matrix", B62, "--minscore", "10", *extra, "--files", files, files)
    assert r.returncode != 0 and "--minscore reports one query's hits" in r.stderr


def test_minscore_stands_in_for_topk(swg, files):
    """--align, --bounds and --tabular ask for --topk K unless --minscore names the hits: with it the parser lets them
    through (and the run then fails for want of a GPU, or succeeds on one)."""
    for flag in ("--align", "--bounds", "--tabular"):
        r = _run("--substitution_matrix", B62, flag, "--files", files, files)
        assert r.returncode != 0 and "give --topk K" in r.stderr, flag
        r = _run("--substitution_matrix", B62, flag, "--minscore", "5", "--files", files, files)
        assert "give --topk K" not in r.stderr and "usage:" not in r.stderr, (flag, r.stderr[:200])
    r = _run("--help")
    assert "--minscore <S>" in r.stderr
