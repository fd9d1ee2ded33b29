"""CPU: the `smith_waterman` tool's --psiblocks and --purge P -- their argument errors, every one raised before a device is
opened.  What they make of an iterated search is checked on the GPU (tests/test_gpu_pssm_blocks.py)."""
import pytest

from test_cli import B62, _run


@pytest.fixture()
def files(tmp_path):
    q = tmp_path / "q.fa"
    q.write_text(">q\nACDEFGHIKL\n>r\nACDEFGHIKL\n")
    return str(q)


@pytest.mark.parametrize("extra,named", [(["--psiblocks"], "--psiblocks"), (["--purge", "94"], "--purge"), (["--purge", "94", "--psiblocks"], "--psiblocks")])
def test_either_flag_needs_iterations(swg, files, extra, named):
    r = _run("--substitution_matrix", B62, "--topk", "3", *extra, "--files", files, files)
    assert r.returncode != 0 and r.stderr.startswith("Error: " + named) and "give --iterations N" in r.stderr and "usage:" in r.stderr, r.stderr[:300]


@pytest.mark.parametrize("value", ["49", "101", "0", "-94", "x", "94.5", ""])
def test_purge_takes_50_to_100(swg, files, value):
    r = _run("--substitution_matrix", B62, "--iterations", "2", "--purge", value, "--topk", "3", "--files", files, files)
    assert r.returncode != 0 and "Invalid --purge argument" in r.stderr and "50 to 100" in r.stderr and "usage:" in r.stderr, r.stderr[:300]


def test_the_flags_are_accepted_with_iterations_and_are_in_the_help(swg, files):
    r = _run("--substitution_matrix", B62, "--iterations", "2", "--psiblocks", "--purge", "94", "--topk", "3", "--files", files, files)
    assert "usage:" not in r.stderr and "--purge" not in r.stderr and "--psiblocks" not in r.stderr, r.stderr[:300]
    r = _run("--substitution_matrix", B62, "--iterations", "2", "--topk", "3", "--files", files, files, "--psiblocks")   # flag-only: last position too
    assert "usage:" not in r.stderr
    r = _run("--help")
    for flag in ("--psiblocks", "--purge <P>"):
        assert flag in r.stderr, flag
