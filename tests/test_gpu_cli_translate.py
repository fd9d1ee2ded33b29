"""GPU (-m gpu): `smith_waterman --translatedb` on a small nucleotide FASTA with a protein planted in each of the six
frames: the hits name the nucleotide records and their frames, --tabular prints nucleotide coordinates (1-based, inclusive,
start above end on a minus frame) and the sframe column, and --evalue counts over the nucleotide residues / 3."""
import re

import numpy as np
import pytest

import translate_cases as tc
from test_cli import B62, _run, _write_fasta
from test_gpu_parity import _reset_options

pytestmark = pytest.mark.gpu

FRAMES = ("+1", "+2", "+3", "-1", "-2", "-3")


@pytest.fixture(autouse=True)
def _options(ctx):
    _reset_options(ctx)
    yield
    _reset_options(ctx)


@pytest.fixture(scope="module")
def fasta(tmp_path_factory):
    """The six planted records among 30 random ones; record 2 i + 1 of the file is planted record i."""
    d = tmp_path_factory.mktemp("translate_cli")
    plant = tc.planted()
    rng = np.random.default_rng(9)
    names, seqs, where = [], [], {}
    for i in range(36):
        if i % 2 == 1 and i // 2 < 6:
            where[i // 2] = len(seqs)
            names.append("planted%d" % (i // 2))
            seqs.append(plant["records"][i // 2])
        else:
            names.append("random%d" % i)
            seqs.append(tc.random_nt(rng, int(rng.integers(40, 700)), "ACGT" * 6 + "N"))
    qf, dbf = d / "q.fa", d / "nt.fa"
    _write_fasta(str(qf), ["protein"], [plant["query"]])
    _write_fasta(str(dbf), names, seqs)
    return dict(q=str(qf), db=str(dbf), plant=plant, where=where, names=names, seqs=seqs)


def _args(fasta, *more):
    return ("--substitution_matrix", B62, "--gapopen", "-11", "--gapextend", "-1", "--translatedb", *more, "--files", fasta["q"], fasta["db"])


def _expected(fasta):
    """(entry, frame label, sstart, send) of every planted record."""
    out = {}
    for rec, frame, nb, ne in fasta["plant"]["plants"]:
        out[fasta["where"][rec]] = (FRAMES[frame], nb + 1, ne) if frame < 3 else (FRAMES[frame], ne, nb + 1)
    return out


def test_topk_tabular_prints_records_frames_and_nucleotide_coordinates(swg, ctx, fasta):
    r = _run(*_args(fasta, "--topk", "6", "--tabular"))
    assert r.returncode == 0, r.stderr[-400:]
    assert "translated 36 entries into 216 frames" in r.stderr
    lines = r.stdout.splitlines()
    assert not any(l.startswith("Entry #") for l in lines) and "Total Entries: 216" in lines
    at = lines.index("Top 6 hits (score, entry, frame, name):")
    want = _expected(fasta)
    top = [l.split("\t") for l in lines[at + 1:at + 7]]
    assert sorted((int(t[1]), t[2]) for t in top) == sorted((e, w[0]) for e, w in want.items())
    assert all(t[3] == fasta["names"][int(t[1])] for t in top) and len({t[0] for t in top}) == 1
    hdr = next(i for i, l in enumerate(lines) if l.startswith("# Fields:"))
    assert lines[hdr].endswith("sstart, send, score, sframe")
    rows = [l.split("\t") for l in lines[hdr + 1:hdr + 7]]
    lq = len(fasta["plant"]["query"])
    seen = {}
    for row in rows:
        assert row[0] == "protein" and (row[2], int(row[3]), int(row[4]), int(row[5])) == ("100.00", lq, 0, 0)
        assert (int(row[6]), int(row[7])) == (1, lq)
        entry = fasta["names"].index(row[1])
        seen[entry] = (row[11], int(row[8]), int(row[9]))
        assert (int(row[8]) > int(row[9])) == row[11].startswith("-")
    assert seen == want


def test_bounds_and_align_name_the_frame(swg, ctx, fasta):
    want = _expected(fasta)
    r = _run(*_args(fasta, "--topk", "6", "--bounds"))
    assert r.returncode == 0, r.stderr[-400:]
    got = {}
    for m in re.finditer(r"Bounds #\d+: entry (\d+) frame ([+-]\d) score \d+ query 0\.\.\d+ entry (\d+)\.\.(\d+) length (\d+)", r.stdout):
        got[int(m.group(1))] = (m.group(2), int(m.group(3)), int(m.group(4)))
    assert got == want
    r = _run(*_args(fasta, "--topk", "6", "--align"))
    assert r.returncode == 0, r.stderr[-400:]
    blocks = re.findall(r"Alignment #\d+: entry (\d+) frame ([+-]\d) score \d+ query \d+\.\.\d+ frame residues \d+\.\.\d+\n(\S+)\n(\S+)\n", r.stdout)
    assert sorted((int(e), f) for e, f, _, _ in blocks) == sorted((e, w[0]) for e, w in want.items())
    assert all(a == b == fasta["plant"]["query"] for _, _, a, b in blocks)       # the frame's protein letters
    # --maskdb masks the translation (the AT-only flanks translate to low-complexity protein, and the widening by the
    # window reaches a few residues into the planted one): the same six records and frames still lead
    r = _run(*_args(fasta, "--topk", "6", "--maskdb", "--allqueries"))
    assert r.returncode == 0, r.stderr[-400:]
    assert "translated 36 entries into 216 frames" in r.stderr and re.search(r"masked [1-9]\d* residues in \d+ of 216 entries", r.stderr)
    lines = r.stdout.splitlines()
    at = lines.index("Top 6 hits (score, entry, frame, name):")
    assert sorted((int(l.split("\t")[1]), l.split("\t")[2]) for l in lines[at + 1:at + 7]) == sorted((e, w[0]) for e, w in want.items())


def test_evalue_counts_over_the_nucleotides_by_three(swg, ctx, fasta):
    r = _run(*_args(fasta, "--evalue", "1e-20", "--tabular"))
    assert r.returncode == 0, r.stderr[-400:]
    residues = sum(len(s) for s in fasta["seqs"]) // 3
    m = re.search(r"E-value 1e-20: lambda ([0-9.]+), K ([0-9.]+), least score (\d+) over (\d+) residues", r.stdout)
    assert m and int(m.group(4)) == residues
    lines = r.stdout.splitlines()
    hdr = next(i for i, l in enumerate(lines) if l.startswith("# Fields:"))
    assert lines[hdr].endswith("send, evalue, bitscore, score, sframe")
    rows = [l.split("\t") for l in lines[hdr + 1:] if l.startswith("protein\t")]
    assert len(rows) == 6 and {row[13] for row in rows} == set(FRAMES)
    # one E-value again from the library: the tool's calibration is the library's with its default options
    sc = swg.load_scoring("BLOSUM62", -11, -1)
    ctx.set_scoring(sc.table(), -11, -1)
    ctx.set_query(tc.indices(fasta["plant"]["query"]))
    params = ctx.calibrate()
    assert abs(params["lambda"] - float(m.group(1))) < 1e-4
    score = int(rows[0][12])
    want = swg.evalue(params, residues, score)
    assert float(rows[0][10]) == pytest.approx(want, rel=6e-3, abs=0)                   # (printed with three significant digits)
    assert swg.evalue(params, 2 * residues, score) != pytest.approx(want, rel=0.2, abs=0)  # ... and not over the six frames' residues
