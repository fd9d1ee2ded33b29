"""CPU: the `smith_waterman` tool's --iterations N, --inclusion E, --maxincluded M and --out_pssm F -- their argument
errors, every one raised before a device is opened.  What an iterated search prints is checked on the GPU
(tests/test_gpu_cli_iterations.py)."""
import pytest

from test_cli import B62, _run


@pytest.fixture()
def files(tmp_path):
    q = tmp_path / "q.fa"
    q.write_text(">q\nACDEFGHIKL\n>r\nACDEFGHIKL\n")
    return str(q)


@pytest.mark.parametrize("value", ["1", "0", "-3", "x", "2.5", ""])
def test_iterations_must_be_two_or_more(swg, files, value):
    r = _run("--substitution_matrix", B62, "--iterations", value, "--topk", "3", "--files", files, files)
    assert r.returncode != 0 and "Invalid --iterations argument: the number of searches, 2 or more" in r.stderr and "usage:" in r.stderr, r.stderr[:200]


@pytest.mark.parametrize("extra,named", [
    (["--allqueries"], "--allqueries"),
    (["--gpus", "2"], "--gpus N > 1"),
    (["--allqueries", "--candidates", "nowhere.txt"], "--allqueries"),
    (["--prefilter", "10"], "--prefilter"),
    (["--gapless"], "--gapless"),
])
def test_iterations_refuses_what_it_cannot_iterate(swg, files, extra, named):
    r = _run("--substitution_matrix", B62, "--iterations", "2", "--topk", "3", *extra, "--files", files, files)
    assert r.returncode != 0 and "--iterations" in r.stderr and named in r.stderr and "usage:" in r.stderr, r.stderr[:300]
    assert r.stderr.startswith("Error: --iterations")                 # (the first thing said: no device was asked for)


def test_candidates_are_refused_by_name(swg, files, tmp_path):
    # (--candidates needs --allqueries, which --iterations refuses first; the message for --candidates alone is in the source's order)
    r = _run("--substitution_matrix", B62, "--iterations", "2", "--topk", "3", "--candidates", "nowhere.txt", "--files", files, files)
    assert r.returncode != 0 and "--candidates" in r.stderr and "usage:" in r.stderr


@pytest.mark.parametrize("extra,message", [
    (["--inclusion", "0"], "Invalid --inclusion argument"),
    (["--inclusion", "nan"], "Invalid --inclusion argument"),
    (["--maxincluded", "0"], "Invalid --maxincluded argument"),
])
def test_bad_values(swg, files, extra, message):
    r = _run("--substitution_matrix", B62, "--iterations", "2", "--topk", "3", *extra, "--files", files, files)
    assert r.returncode != 0 and message in r.stderr and "usage:" in r.stderr


@pytest.mark.parametrize("extra", [["--inclusion", "0.01"], ["--maxincluded", "10"], ["--out_pssm", "x.pssm"]])
def test_the_iteration_flags_need_iterations(swg, files, extra):
    r = _run("--substitution_matrix", B62, "--topk", "3", *extra, "--files", files, files)
    assert r.returncode != 0 and "give --iterations N" in r.stderr and "usage:" in r.stderr


def test_compfromdb_is_accepted_and_the_flags_are_in_the_help(swg, files):
    r = _run("--substitution_matrix", B62, "--iterations", "2", "--compfromdb", "--topk", "3", "--files", files, files)
    assert "give --evalue E" not in r.stderr and "usage:" not in r.stderr
    r = _run("--help")
    for flag in ("--iterations <N>", "--inclusion <E>", "--maxincluded <M>", "--out_pssm <file>"):
        assert flag in r.stderr, flag
