"""CPU: the host side of swg_align_stats and its batch forms (no GPU): the ABI and the binding, NULL arguments, and the
command-line tool's --tabular flag checks, which are reported before any device is touched."""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import ROOT

CLI = os.path.join(ROOT, "seq-align-gpu_amd", "bin", "smith_waterman")
B62 = os.path.join(ROOT, "seq-align-gpu_amd", "data", "BLOSUM62.txt")
NEW_SYMBOLS = ("swg_align_stats", "swg_align_stats_multi", "swg_align_stats_multi_pssm")


def test_stats_abi_and_binding(swg):
    for name in NEW_SYMBOLS:
        assert hasattr(swg.lib, name), name
        assert name in swg.ABI_SYMBOLS, name
    for name in ("align_stats", "align_stats_multi", "align_stats_multi_pssm"):
        assert callable(getattr(swg.Context, name, None)), name
    assert C.sizeof(swg.AlignCounts) == 16
    assert [f for f, _ in swg.AlignCounts._fields_] == ["n_ident", "n_match", "n_gap_open", "n_gap"]
    assert swg.lib.swg_abi_version() == 3          # functions and a struct were added, no struct changed


def test_stats_declared_in_the_public_header():
    text = open(os.path.join(ROOT, "include", "swg.h")).read()
    for name in NEW_SYMBOLS:
        assert "int %s(swg_ctx *ctx, const swg_db *db," % name in text, name
    assert "} swg_align_counts;" in text and "swg_align_counts *counts);" in text
    for field in ("n_ident", "n_match", "n_gap_open", "n_gap"):
        assert "uint32_t %s;" % field in text, field
    assert "consensus" in text                     # the PSSM identity rule is part of the contract
    assert "#define SWG_ABI_VERSION 3" in text


def test_stats_null_arguments(swg):
    q = np.ones(4, dtype=np.int8)
    off = np.array([0, 4], dtype=np.uint64)
    nh = (C.c_size_t * 1)(0)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)                                    # noqa: E731
    calls = {
        "swg_align_stats": lambda: swg.lib.swg_align_stats(None, None, None, 0, None, None),
        "swg_align_stats_multi": lambda: swg.lib.swg_align_stats_multi(None, None, vp(q), vp(off), 1, None, 0,
                                                                      C.cast(nh, C.c_void_p), None, None),
        "swg_align_stats_multi_pssm": lambda: swg.lib.swg_align_stats_multi_pssm(None, None, None, None, 0, None, 0, None, None, None),
    }
    for name, call in calls.items():
        assert call() == swg.SWG_ERR_ARG, name
        assert name in swg.lib.swg_global_error().decode(), name


def _run(*a):
    return subprocess.run([CLI, "--substitution_matrix", B62] + [str(x) for x in a], stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, text=True, timeout=120)


def test_cli_tabular_flag_checks(swg, tmp_path):
    q = tmp_path / "q.fa"
    q.write_text(">q\nACDEFG\n")
    db = tmp_path / "d.fa"
    db.write_text(">d\nACDEFGKLMNP\n")
    r = _run("--tabular", "--files", q, db)
    assert r.returncode != 0 and "usage:" in r.stderr and "--tabular reports one tabular line for each of the --topk hits" in r.stderr, r.stderr
    r = _run("--topk", 3, "--tabular", "--align", "--files", q, db)
    assert r.returncode != 0 and "usage:" in r.stderr and "does not combine with --align" in r.stderr, r.stderr
    r = _run("--topk", 3, "--tabular", "--bounds", "--files", q, db)
    assert r.returncode != 0 and "usage:" in r.stderr and "does not combine with --bounds" in r.stderr, r.stderr
    r = _run("--topk", 3, "--tabular", "--gapless", "--files", q, db)
    assert r.returncode != 0 and "usage:" in r.stderr and "does not combine with --gapless" in r.stderr, r.stderr
    r = _run("--topk", 3, "--tabular", "--gpus", 2, "--files", q, db)
    assert r.returncode != 0 and "usage:" in r.stderr and "--tabular works with one GPU" in r.stderr, r.stderr
    # the flag is in the usage text, and takes no parameter (valid in last position)
    r = _run("--help")
    assert "--tabular" in r.stderr and "# Fields: query, entry, pident, length, mismatch, gapopen" in r.stderr
    r = _run("--files", q, db, "--tabular")
    assert "Unknown argument" not in r.stderr and "give --topk K" in r.stderr, r.stderr
