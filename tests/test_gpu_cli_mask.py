"""GPU (-m gpu): the `smith_waterman` tool's masking options on the end-to-end case of the masking tests (decoys that
share only a Q/E-rich run with the query, relatives of its other part): --maskdb's hit list is the oracle's on the
twin-masked database, --savedb then writes the masked image, --softmask --prefilter reports what the Python calls
compose, --maskquery searches the twin-masked query."""
import numpy as np
import pytest

import mask_cases as mc
from test_cli import B62, _letters, _run, _write_fasta
from test_gpu_parity import _reset_options

pytestmark = pytest.mark.gpu

SCORING = ("--substitution_matrix", B62, "--gapopen", "-11", "--gapextend", "-1")


@pytest.fixture(autouse=True)
def _options(ctx):
    _reset_options(ctx)
    ctx.set_option("autotune", 0)
    yield
    ctx.set_option("autotune", 1)


@pytest.fixture(scope="module")
def case(swg, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("cli_mask")
    c = mc.end_to_end()
    names = ["db%d" % i for i in range(len(c["seqs"]))]
    qf, df = tmp / "query.fasta", tmp / "db.fasta"
    _write_fasta(qf, ["query"], [_letters(swg, c["query"])])
    _write_fasta(df, names, [_letters(swg, s) for s in c["seqs"]])
    flat, off = mc.flat_of(c["seqs"])
    return dict(c, tmp=tmp, qf=str(qf), df=str(df), names=names, flat=flat, off=off, sc=swg.load_scoring("BLOSUM62", -11, -1))


def _hit_block(stdout, names=None):
    lines = stdout.splitlines()
    at = next(i for i, l in enumerate(lines) if l.startswith("Top ") and "hits" in l)
    n = int(lines[at].split()[1])
    out = []
    for l in lines[at + 1:at + 1 + n]:
        s, i, name = (l.split("\t") + [""])[:3]
        if names is not None:
            assert name == names[int(i)]
        out.append((int(s), int(i)))
    return out


def test_maskdb_reports_the_relatives_and_saves_the_masked_image(swg, ctx, orc, case):
    masked_flat, counts = swg.seg_mask_flat(case["flat"], case["off"])
    want = orc.score_db(case["query"], masked_flat, case["off"], case["sc"].table(), -11, -1)
    saved = str(case["tmp"] / "masked.swg")
    r = _run(*SCORING, "--maskdb", "--topk", "5", "--timing", "--savedb", saved, "--files", case["qf"], case["df"])
    assert r.returncode == 0, r.stderr
    hits = _hit_block(r.stdout, case["names"])
    assert hits == mc.top_hits(want, 5) and {i for _, i in hits} == case["relatives"]
    assert "masked %d residues in %d of %d entries (%d regions; window 12, 2.2 / 2.5 bits)" % (
        counts["residues_masked"], counts["sequences_masked"], len(case["seqs"]), counts["segments"]) in r.stderr
    assert "[timing] mask the database" in r.stderr and "ms of kernels" in r.stderr and "for the host image" in r.stderr
    # every Entry line is the masked database's score
    import re
    got = {int(i): int(s) for i, s in re.findall(r"Entry\s+#(\d+):\s*score:\s*([+-]?\d+)", r.stdout)}
    assert got == {i: int(v) for i, v in enumerate(want)}
    # without the option: the decoys
    r0 = _run(*SCORING, "--topk", "5", "--files", case["qf"], case["df"])
    assert r0.returncode == 0 and sum(i in case["decoys"] for _, i in _hit_block(r0.stdout)) >= 3
    # the saved image is the masked one: loaded as it is, it reports the same hits
    loaded = swg.Database(path=saved)
    for i in (0, 100, len(case["seqs"]) - 1):
        assert np.array_equal(loaded.sequence(i), masked_flat[int(case["off"][i]):int(case["off"][i + 1])])
    r2 = _run(*SCORING, "--packed", "--topk", "5", "--files", case["qf"], saved)
    assert r2.returncode == 0 and _hit_block(r2.stdout) == hits
    # explicit parameters: those of the twin
    w4, _ = swg.seg_mask_flat(case["flat"], case["off"], window=16, trigger=2.0, extend=2.4)
    want4 = orc.score_db(case["query"], w4, case["off"], case["sc"].table(), -11, -1)
    r3 = _run(*SCORING, "--maskdb", "16,2.0,2.4", "--topk", "7", "--files", case["qf"], case["df"])
    assert r3.returncode == 0 and _hit_block(r3.stdout) == mc.top_hits(want4, 7)


def test_softmask_is_what_the_python_calls_compose(swg, ctx, case):
    ctx.set_scoring(case["sc"].table(), -11, -1)
    ctx.set_query(case["query"])
    db = swg.Database(case["flat"], case["off"]).upload(ctx)
    masked = db.mask(ctx)
    for n in (8, 40):
        _, cand, _ = ctx.search_gapless(masked, want_scores=False, k=n)
        _, hits, _ = ctx.search_lists(db, [case["query"]], [[i for _, i in cand]], k=5, want_scores=False)
        r = _run(*SCORING, "--softmask", "--prefilter", str(n), "--topk", "5", "--files", case["qf"], case["df"])
        assert r.returncode == 0, r.stderr
        assert _hit_block(r.stdout, case["names"]) == hits[0], n
        # hard masking differs: the gapped stage reads the masked copy too
        _, hard, _ = ctx.search_lists(masked, [case["query"]], [[i for _, i in cand]], k=5, want_scores=False)
        r = _run(*SCORING, "--maskdb", "--prefilter", str(n), "--topk", "5", "--files", case["qf"], case["df"])
        assert r.returncode == 0 and _hit_block(r.stdout) == hard[0], n
    masked.close()
    db.close()


def test_maskquery_searches_the_masked_query(swg, ctx, case):
    ctx.set_scoring(case["sc"].table(), -11, -1)
    m = swg.seg_mask(case["query"])
    assert m[60:90].any()                                        # the Q/E stretch is what gets masked
    ctx.set_query(mc.apply_mask(case["query"], m))
    db = swg.Database(case["flat"], case["off"]).upload(ctx)
    _, hits, _ = ctx.search(db, want_scores=False, k=5)
    r = _run(*SCORING, "--maskquery", "--topk", "5", "--files", case["qf"], case["df"])
    assert r.returncode == 0, r.stderr
    assert _hit_block(r.stdout, case["names"]) == hits
    assert {i for _, i in hits} == case["relatives"]            # masking the query alone removes the decoys as well
    db.close()
