"""CPU: the `smith_waterman` tool's --maxhsps N and --hspscore S (several alignments per reported hit: swg_align_hsps*) --
their argument errors and the help text.  What they print is checked on the GPU (tests/test_gpu_cli_hsps.py)."""
import pytest

from test_cli import B62, _run


@pytest.fixture()
def files(tmp_path):
    q = tmp_path / "q.fa"
    q.write_text(">q\nACDEFGHIKL\n")
    return str(q)


def base(files, *args):
    return _run("--substitution_matrix", B62, *args, "--files", files, files)


@pytest.mark.parametrize("value", ["0", "65", "-1", "x", "3x", "", "2.5", "99999999999"])
def test_maxhsps_outside_1_to_64_is_a_usage_error(swg, files, value):
    r = base(files, "--topk", "3", "--tabular", "--maxhsps", value)
    assert r.returncode != 0 and "Invalid --maxhsps argument" in r.stderr and "usage:" in r.stderr, (value, r.stderr[:200])


@pytest.mark.parametrize("value", ["0", "-4", "x", "", "1.5", "99999999999"])
def test_hspscore_below_one_is_a_usage_error(swg, files, value):
    r = base(files, "--topk", "3", "--tabular", "--maxhsps", "4", "--hspscore", value)
    assert r.returncode != 0 and "Invalid --hspscore argument" in r.stderr and "usage:" in r.stderr, (value, r.stderr[:200])


@pytest.mark.parametrize("flag", ["--maxhsps", "--hspscore"])
def test_both_need_their_argument(swg, files, flag):
    r = _run("--substitution_matrix", B62, "--files", files, files, flag)
    assert r.returncode != 0 and "Unknown argument without parameter: " + flag in r.stderr


def test_maxhsps_needs_a_report_to_act_on(swg, files):
    r = base(files, "--topk", "3", "--maxhsps", "4")
    assert r.returncode != 0 and "--maxhsps N reports up to N alignments per hit of --align, --bounds or --tabular" in r.stderr
    assert "usage:" in r.stderr


@pytest.mark.parametrize("extra", [["--gapless"], ["--gpus", "2"], ["--iterations", "2"], ["--allqueries", "--candidates", "c.txt"],
                                   ["--prefilter", "10"]])
def test_maxhsps_does_not_combine(swg, files, extra):
    for report in ("--align", "--bounds", "--tabular"):
        r = base(files, "--topk", "3", report, "--maxhsps", "4", *extra)
        assert r.returncode != 0 and "usage:" in r.stderr, (report, extra)
        assert "--maxhsps does not combine with --gapless, --gpus, --iterations, --candidates or --prefilter" in r.stderr, (report, extra)


def test_hspscore_needs_maxhsps(swg, files):
    r = base(files, "--topk", "3", "--tabular", "--hspscore", "20")
    assert r.returncode != 0 and "--hspscore is the least score of --maxhsps' alignments: give --maxhsps N" in r.stderr


def test_accepted_combinations_pass_the_parser(swg, files):
    """(the run then fails for want of a GPU, or succeeds on one)"""
    for args in (["--topk", "3", "--align"], ["--minscore", "5", "--bounds"], ["--topk", "2", "--tabular", "--allqueries"],
                 ["--topk", "2", "--evalue", "10", "--tabular"]):
        r = base(files, *args, "--maxhsps", "64", "--hspscore", "1")
        assert "usage:" not in r.stderr, (args, r.stderr[:200])


def test_help_names_both_flags(swg):
    r = _run("--help")
    assert "--maxhsps <N>" in r.stderr and "--hspscore <S>" in r.stderr
