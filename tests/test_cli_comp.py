"""CPU: `smith_waterman --compstats [F]` -- argument handling.  The flag adjusts the scores of reported hits (--topk,
--evalue, --tabular, --minscore, --iterations); where no hit is reported there is nothing to adjust, and it
is refused with a usage message that says so."""
from test_cli import B62, _run


def _files(tmp_path):
    q = tmp_path / "q.fa"
    q.write_text(">q\nACDEFGHIKL\n")
    return ["--files", str(q), str(q)]


def test_compstats_is_refused_where_there_is_nothing_to_adjust(swg, tmp_path):
    """The plain `Entry #n` stream reports no hits: nothing to adjust.  And beside the reports it has no form for."""
    files = _files(tmp_path)
    for flag in (["--compstats"], ["--compstats", "16"]):
        r = _run("--substitution_matrix", B62, *flag, *files)
        assert r.returncode != 0 and "usage:" in r.stderr and "nothing to adjust" in r.stderr and "--topk K" in r.stderr, (flag, r.stderr[-300:])
        assert "Unknown argument" not in r.stderr
    for extra in (["--gapless"], ["--gpus", "2"], ["--prefilter", "50"], ["--maxhsps", "3", "--bounds"]):
        r = _run("--substitution_matrix", B62, "--topk", "5", "--compstats", *extra, *files)
        assert r.returncode != 0 and "usage:" in r.stderr and "--compstats does not combine" in r.stderr, (extra, r.stderr[-300:])


def test_the_scale_is_optional_and_bounded(swg, tmp_path):
    files = _files(tmp_path)
    for bad in ("0", "65", "-3", "1000"):
        r = _run("--substitution_matrix", B62, "--iterations", "2", "--topk", "5", "--compstats", bad, *files)
        assert r.returncode != 0 and "Invalid --compstats argument" in r.stderr and "1 to 64" in r.stderr, (bad, r.stderr[-300:])
        assert "Unknown argument" not in r.stderr
    # flag alone or with a scale, in every report it has a form for: parsed (the run then fails for want of a GPU)
    for mode in (["--topk", "5"], ["--topk", "5", "--evalue", "1e-3"], ["--topk", "5", "--evalue", "1e-3", "--tabular"], ["--minscore", "40"],
                 ["--iterations", "2", "--topk", "5"], ["--allqueries", "--topk", "5"]):
        for flag in (["--compstats"], ["--compstats", "1"], ["--compstats", "64"]):
            r = _run("--substitution_matrix", B62, *mode, *flag, *files)
            assert "usage:" not in r.stderr and "Unknown argument" not in r.stderr, (mode, flag, r.stderr[-300:])


def test_help_says_what_stays_unadjusted(swg):
    r = _run("--help")
    text = r.stderr + r.stdout
    assert "--compstats [F]" in text and "unadjusted" in text and "--inclusion" in text and "adjusted score, score, entry, name" in text
