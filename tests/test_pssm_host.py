"""Position-specific queries, host side (no GPU): swg_pssm_load on PSI-BLAST's ASCII PSSM layout, the CLI's --pssm
argument checks, and a numpy restatement of the three-state recurrence with a per-position score column,
pinned here against the oracle so that the GPU tests can use it for PSSMs the oracle cannot express."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CLI = os.path.join(ROOT, "seq-align-gpu_amd", "bin", "smith_waterman")
B62 = os.path.join(ROOT, "seq-align-gpu_amd", "data", "BLOSUM62.txt")
PSIBLAST_COLS = "ARNDCQEGHILKMFPSTWYV"


def letters(swg, idx):
    return "".join(chr(swg.lib.swg_index_letter(int(v))) for v in idx)


def write_ascii_pssm(path, query_letters, scores, cols=PSIBLAST_COLS, gz=False, first_pos=1):
    """A PSSM file in the layout of psiblast -out_ascii_pssm: a blank line and a sentence, the 40-letter header (score
    columns, then the weighted-percentage columns), per position `pos letter 20 scores 20 percentages info weight`,
    a blank line and the Lambda/K footer.  scores: int[lq, 20] in the order of cols."""
    lines = ["", "Last position-specific scoring matrix computed, weighted observed percentages rounded down, "
             "information per position, and relative weight of gapless real matches to pseudocounts",
             "           " + " ".join("%3s" % c for c in cols) + " " + " ".join("%3s" % c for c in cols)]
    rng = np.random.default_rng(len(query_letters))
    for i, (ch, row) in enumerate(zip(query_letters, scores)):
        pct = rng.integers(0, 100, size=20)
        lines.append("%5d %s  " % (first_pos + i, ch) + " ".join("%3d" % int(v) for v in row) + "  " +
                     " ".join("%3d" % int(v) for v in pct) + "  %.2f %.2f" % (rng.random() * 3, rng.random()))
    lines += ["", "                      K         Lambda", "Standard Ungapped    0.1340     0.3177",
              "Standard Gapped      0.0410     0.2670", "PSI Ungapped         0.1360     0.3191",
              "PSI Gapped           0.0410     0.2670", ""]
    op = gzip.open if gz else open
    with op(str(path), "wt") as f:
        f.write("\n".join(lines))


def expected_pssm(swg, sub, query_letters, scores, cols=PSIBLAST_COLS):
    """What swg_pssm_load must return: named columns from the file, the rest from sub[query residue]."""
    q = swg.letters_to_indices(query_letters)
    p = sub[q.astype(np.int64)].astype(np.int8)
    p[:, 0] = 0
    for c, ch in enumerate(cols):
        p[:, swg.lib.swg_letter_index(ord(ch))] = scores[:, c]
    return p, q


def sw_numpy(pssm, flat, offsets, gap_open, gap_extend):
    """SURVEY A.1 with a per-position score column: cell (j, i) scores pssm[i][d[j]].  Vectorised over the sequences
    (small sizes only); -> int32 scores in database order."""
    pssm = np.asarray(pssm, dtype=np.int64)
    offsets = np.asarray(offsets, dtype=np.int64)
    n, lq = len(offsets) - 1, pssm.shape[0]
    lens = np.diff(offsets)
    L = int(lens.max()) if n else 0
    D = np.zeros((n, max(L, 1)), dtype=np.int64)
    for k in range(n):
        D[k, :lens[k]] = flat[offsets[k]:offsets[k + 1]]
    go, ge = gap_open + gap_extend, gap_extend
    H = np.zeros((lq + 1, n), dtype=np.int64)
    A = np.zeros_like(H)
    B = np.zeros_like(H)
    best = np.zeros(n, dtype=np.int64)
    for j in range(L):
        S = pssm[:, D[:, j]]                      # [lq, n]
        live = j < lens
        hd, ad, bd = H[:-1].copy(), A[:-1].copy(), B[:-1].copy()   # row j-1, columns i-1
        Hn = np.zeros_like(H)
        An = np.zeros_like(H)
        Bn = np.zeros_like(H)
        An[1:] = np.maximum(np.maximum(H[1:] + go, A[1:] + ge), np.maximum(B[1:] + go, 0))
        Hn[1:] = np.maximum(np.maximum(hd + S, ad + S), np.maximum(bd + S, 0))
        for i in range(1, lq + 1):                # the left dependency runs along the row
            Bn[i] = np.maximum(np.maximum(Hn[i - 1] + go, An[i - 1] + go), np.maximum(Bn[i - 1] + ge, 0))
        best = np.where(live, np.maximum(best, Hn.max(axis=0)), best)
        H, A, B = Hn, An, Bn
    return best.astype(np.int32)


def _load(swg, path, sc):
    return swg.read_pssm(str(path), sc)


def test_pssm_load_round_trip(swg, tmp_path):
    sc = swg.load_scoring("BLOSUM62")
    sub = sc.table()
    rng = np.random.default_rng(1)
    ql = "MKTAYIAKQRQISFVKSHFSRQLEERLGLIEVQAPILSRVGDGTQDNLSGAEKAVQVKVKALPDAQFEVVHSLAKWKRQTLGQHDFSAGEGLYTHMKALRPDEDRLSPLHSVYVDQWDWERVMGDGERQFSTLKSTVEAIWAGIKATEAAVSEEFGLAPFLPDQIHFVHSQELLSRYPDLDAKGRERAIAKDLGAVFLVGIGGKLSDGHRHDVRAPDYDDWSTPSELGHAGLNGDILVWNPVLEDAFELSSMGIRVDADTLKHQLALTGDEDRLELEWHQALLRGEMPQTIGGGIGQSRLTMLLLQLPHIGQVQAGVWPAACRESVPALL"
    scores = rng.integers(-128, 128, size=(len(ql), 20))
    scores[0, :2] = (-128, 127)
    for gz in (False, True):
        path = tmp_path / ("q.pssm" + (".gz" if gz else ""))
        write_ascii_pssm(path, ql, scores, gz=gz)
        pssm, q = _load(swg, path, sc)
        want, wq = expected_pssm(swg, sub, ql, scores)
        assert pssm.shape == (len(ql), 32) and pssm.dtype == np.int8
        assert np.array_equal(q, wq)
        assert np.array_equal(pssm, want)
        assert (pssm[:, 0] == 0).all()


def test_pssm_load_unnamed_columns_from_matrix(swg, tmp_path):
    """A header that names fewer residues (here 20 columns in another order, without W but with X): every code it
    does not name, W, B, Z, '*' ... included, is the matrix's score against the position's residue."""
    sc = swg.load_scoring("BLOSUM62")
    sub = sc.table()
    cols = "XARNDCQEGHILKMFPSTYV"
    ql = "ACDWXBZ*"
    scores = np.arange(len(ql) * 20).reshape(len(ql), 20) % 50 - 25
    write_ascii_pssm(tmp_path / "p", ql, scores, cols=cols)
    pssm, q = _load(swg, tmp_path / "p", sc)
    want, _ = expected_pssm(swg, sub, ql, scores, cols=cols)
    assert np.array_equal(pssm, want)
    iw, ib = swg.lib.swg_letter_index(ord("W")), swg.lib.swg_letter_index(ord("B"))
    assert all(pssm[i, iw] == sub[q[i], iw] and pssm[i, ib] == sub[q[i], ib] for i in range(len(ql)))


@pytest.mark.parametrize("case", ["no_header", "too_large", "too_small", "gap", "bad_residue", "short_line", "empty"])
def test_pssm_load_errors(swg, tmp_path, case):
    sc = swg.load_scoring("BLOSUM62")
    ql = "ACDEFGHIK"
    scores = np.zeros((len(ql), 20), dtype=np.int64)
    path = tmp_path / "bad.pssm"
    write_ascii_pssm(path, ql, scores)
    lines = path.read_text().split("\n")
    line = 6                                                              # 1-based: the 3rd position's line
    if case == "no_header":
        lines[2] = " ".join(PSIBLAST_COLS[:19])                            # 19 letters: no line qualifies
        line = None
    else:
        if case == "too_large":
            lines[line - 1] = lines[line - 1].replace("  0", "128", 1)
        elif case == "too_small":
            lines[line - 1] = lines[line - 1].replace("  0", "-129", 1)
        elif case == "gap":
            lines[line - 1] = "    5" + lines[line - 1][5:]
        elif case == "bad_residue":
            lines[line - 1] = lines[line - 1][:6] + "1" + lines[line - 1][7:]
        elif case == "short_line":
            lines[line - 1] = lines[line - 1][:20]
        elif case == "empty":
            lines = lines[:3] + [""] + lines[3:]
            line = None
    path.write_text("\n".join(lines))
    with pytest.raises(swg.SwgError) as e:
        _load(swg, path, sc)
    assert e.value.code == swg.SWG_ERR_IO
    assert str(path) in str(e.value)
    if line is not None:
        assert "line %d)" % line in str(e.value), str(e.value)


def test_pssm_load_missing_file(swg, tmp_path):
    with pytest.raises(swg.SwgError) as e:
        _load(swg, tmp_path / "none.pssm", swg.load_scoring("BLOSUM62"))
    assert e.value.code == swg.SWG_ERR_IO


def test_set_query_pssm_shape_checks(swg):
    """The Python binding refuses anything but an (lq, 32) array before it reaches the library."""
    for bad in (np.zeros(32, dtype=np.int8), np.zeros((4, 31), dtype=np.int8), np.full((2, 32), 200)):
        with pytest.raises(ValueError):
            swg._pssm(bad)


def test_abi_exports_pssm(swg):
    for name in ("swg_set_query_pssm", "swg_group_set_query_pssm", "swg_pssm_load", "swg_pssm_free"):
        assert name in swg.ABI_SYMBOLS and hasattr(swg.lib, name)


@pytest.mark.parametrize("gaps", [(-2, -1), (-10, -1), (0, -1), (-3, 1)])
def test_numpy_restatement_matches_oracle(swg, orc, gaps):
    """sw_numpy on sub[q] equals the oracle on (q, sub); on a 31-column PSSM it equals the oracle on the synthetic
    (q', sub') that PSSM is (the trick the GPU tests rest on)."""
    sc = swg.load_scoring("BLOSUM62")
    sub = sc.table()
    q = swg.synth_query(7, 40)
    flat, off = swg.synth_db(11, 48, median=40.0, sigma_ln=0.5, min_len=1, max_len=90)
    want = orc.score_db(q, flat, off, sub, *gaps)
    assert np.array_equal(sw_numpy(sub[q.astype(np.int64)], flat, off, *gaps), want)
    rng = np.random.default_rng(5)
    cols = rng.integers(-128, 128, size=(31, 32)).astype(np.int8)
    qp = rng.integers(1, 32, size=33).astype(np.int8)
    subp = np.zeros((32, 32), dtype=np.int8)
    subp[1:] = cols
    pssm = subp[qp.astype(np.int64)]
    assert np.array_equal(sw_numpy(pssm, flat, off, *gaps), orc.score_db(qp, flat, off, subp, *gaps))


def test_cli_pssm_argument_checks(swg, tmp_path):
    """--pssm's own errors need no GPU: a missing value, --allqueries, an unreadable file, a PSSM that does not spell
    the query record (case aside)."""
    q = tmp_path / "q.fa"
    q.write_text(">q\nacdefg\n")
    db = tmp_path / "d.fa"
    db.write_text(">d\nACDEFG\n")

    def run(*a):
        return subprocess.run([CLI, "--substitution_matrix", B62] + list(a), stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, text=True, timeout=120)

    r = run("--files", str(q), str(db), "--pssm")
    assert r.returncode != 0 and "Unknown argument without parameter: --pssm" in r.stderr
    good = tmp_path / "good.pssm"
    write_ascii_pssm(good, "ACDEFG", np.zeros((6, 20), dtype=np.int64))
    r = run("--allqueries", "--pssm", str(good), "--files", str(q), str(db))
    assert r.returncode != 0 and "--allqueries" in r.stderr and "usage:" in r.stderr
    r = run("--pssm", str(tmp_path / "none.pssm"), "--files", str(q), str(db))
    assert r.returncode != 0 and "PSSM" in r.stderr
    for other in ("ACDEFH", "ACDEF", "ACDEFGA"):
        bad = tmp_path / ("bad_%d.pssm" % len(other))
        write_ascii_pssm(bad, other, np.zeros((len(other), 20), dtype=np.int64))
        r = run("--pssm", str(bad), "--files", str(q), str(db))
        assert r.returncode != 0 and "does not spell the query" in r.stderr, r.stderr
