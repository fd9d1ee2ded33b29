"""CPU: the `smith_waterman` tool's masking options -- what the parser accepts and what it refuses by name, before a GPU
is needed (--maskdb [W,K1,K2], --softmask, --maskquery)."""
from test_cli import B62, _run

BASE = ("--substitution_matrix", B62)


def _files(tmp_path):
    q = tmp_path / "q.fa"
    q.write_text(">q\nACDEFGHIKLMNPQRSTVWY\n")
    return ("--files", str(q), str(q))


def test_refusals_by_name(swg, tmp_path):
    files = _files(tmp_path)
    r = _run(*BASE, "--softmask", "--topk", "3", *files)
    assert r.returncode != 0 and "--softmask" in r.stderr and "give --prefilter N" in r.stderr
    r = _run(*BASE, "--maskdb", "--gpus", "2", *files)
    assert r.returncode != 0 and "--maskdb works with one GPU" in r.stderr and "--gpus N > 1" in r.stderr
    r = _run(*BASE, "--softmask", "--prefilter", "5", "--topk", "3", "--gpus", "2", *files)
    assert r.returncode != 0 and "usage:" in r.stderr
    pssm = tmp_path / "q.pssm"
    pssm.write_text("")
    r = _run(*BASE, "--maskquery", "--pssm", str(pssm), *files)
    assert r.returncode != 0 and "--maskquery" in r.stderr and "--pssm" in r.stderr
    r = _run(*BASE, "--maskquery", "--allqueries", "--pssmlist", str(pssm), *files)
    assert r.returncode != 0 and "--maskquery" in r.stderr
    for bad in ("3,2.2,2.5", "65,2.2,2.5", "12,2.6,2.5", "12,-1,2.5", "12,2.2", "12,2.2,2.5,1", "12,a,b", "12,2.2,2.5x"):
        r = _run(*BASE, "--maskdb", bad, *files)
        assert r.returncode != 0 and "Invalid --maskdb argument" in r.stderr, bad


def test_accepted_spellings(swg, tmp_path):
    """The parameters are optional and the three options are flags: valid in the last position, and in front of another
    option.  (Whether the run then finds a GPU is not this test's matter.)"""
    files = _files(tmp_path)
    for args in (("--maskdb",), ("--maskdb", "12,2.2,2.5"), ("--maskdb", "4,0.9,1.6"), ("--maskdb", "64,3,3.9"), ("--maskquery",),
                 ("--maskdb", "--maskquery"), ("--prefilter", "5", "--topk", "3", "--softmask"),
                 ("--prefilter", "5", "--topk", "3", "--maskdb", "16,2.0,2.4", "--softmask")):
        for r in (_run(*BASE, *args, *files), _run(*BASE, *files, *args)):
            assert "Invalid --maskdb" not in r.stderr and "Unknown argument" not in r.stderr and "usage:" not in r.stderr, (args, r.stderr)
    r = _run("--help")
    assert "--maskdb [W,K1,K2]" in r.stderr and "--softmask" in r.stderr and "--maskquery" in r.stderr
