"""CPU: the `smith_waterman` tool's --translatedb [CODE] -- what the parser accepts and what it refuses by name, before a
GPU is needed."""
from test_cli import B62, _run

BASE = ("--substitution_matrix", B62)


def _files(tmp_path):
    q = tmp_path / "q.fa"
    q.write_text(">q\nACDEFGHIKLMNPQRSTVWY\n")
    db = tmp_path / "nt.fa"
    db.write_text(">contig\nATGGCTTGTGATGAATTTGGTCATATTAAACTTATGAATCCTCAACGTTCTACTGTTTGGTATTAA\n")
    return ("--files", str(q), str(db))


def test_refusals_by_name(swg, tmp_path):
    files = _files(tmp_path)
    some = tmp_path / "some.txt"
    some.write_text("0\n")
    refused = {
        "--gpus": ("--topk", "3", "--gpus", "2"),
        "--savedb": ("--topk", "3", "--savedb", str(tmp_path / "out.swg")),
        "--seqidlist": ("--topk", "3", "--seqidlist", str(some)),
        "--candidates": ("--topk", "3", "--allqueries", "--candidates", str(some)),
        "--prefilter": ("--topk", "3", "--prefilter", "5"),
        "--softmask": ("--topk", "3", "--softmask"),
        "--iterations": ("--topk", "3", "--iterations", "2"),
        "--compstats": ("--topk", "3", "--compstats"),
        "--maxhsps": ("--topk", "3", "--tabular", "--maxhsps", "2"),
    }
    for name, args in refused.items():
        for r in (_run(*BASE, "--translatedb", *args, *files), _run(*BASE, *args, "--translatedb", "4", *files)):
            assert r.returncode != 0 and "usage:" in r.stderr, name
            assert "--translatedb" in r.stderr.split("usage:")[0] and name in r.stderr.split("usage:")[0], (name, r.stderr[:300])
    # the plain Entry stream has nothing of the reference's to mirror
    r = _run(*BASE, "--translatedb", *files)
    assert r.returncode != 0 and "--translatedb" in r.stderr.split("usage:")[0] and "--topk K" in r.stderr.split("usage:")[0]
    for bad in ("7", "0", "12", "-1"):
        r = _run(*BASE, "--translatedb", bad, "--topk", "3", *files)
        assert r.returncode != 0 and "Invalid --translatedb argument" in r.stderr, bad


def test_accepted_spellings(swg, tmp_path):
    """The code is optional and the option is a flag: valid in the last position, and in front of another option.  (Whether
    the run then finds a GPU is not this test's matter.)"""
    files = _files(tmp_path)
    for args in (("--topk", "3", "--translatedb"), ("--topk", "3", "--translatedb", "4"), ("--translatedb", "--topk", "3"),
                 ("--translatedb", "11", "--topk", "3", "--tabular"), ("--translatedb", "--minscore", "30", "--bounds"),
                 ("--translatedb", "--evalue", "10", "--compfromdb"), ("--translatedb", "--maskdb", "--topk", "2", "--align"),
                 ("--translatedb", "2", "--allqueries", "--topk", "2")):
        for r in (_run(*BASE, *args, *files), _run(*BASE, *files, *args)):
            assert "Invalid --translatedb" not in r.stderr and "Unknown argument" not in r.stderr and "usage:" not in r.stderr, (args, r.stderr)
    r = _run("--help")
    assert "--translatedb [CODE]" in r.stderr and "sframe" in r.stderr and "residues / 3" in r.stderr
