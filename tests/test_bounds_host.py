"""CPU: the host side of swg_align_bounds and its batch forms (no GPU): the ABI and the binding, NULL arguments, and the
command-line tool's --bounds flag checks, which are reported before any device is touched."""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import ROOT

CLI = os.path.join(ROOT, "seq-align-gpu_amd", "bin", "smith_waterman")
B62 = os.path.join(ROOT, "seq-align-gpu_amd", "data", "BLOSUM62.txt")
NEW_SYMBOLS = ("swg_align_bounds", "swg_align_bounds_multi", "swg_align_bounds_multi_pssm")


def test_bounds_abi_and_binding(swg):
    for name in NEW_SYMBOLS:
        assert hasattr(swg.lib, name), name
        assert name in swg.ABI_SYMBOLS, name
    for name in ("align_bounds", "align_bounds_multi", "align_bounds_multi_pssm", "debug_bounds_last"):
        assert callable(getattr(swg.Context, name, None)), name
    assert hasattr(swg.lib, "swg_debug_bounds_last")
    assert swg.lib.swg_abi_version() == 3          # functions were added, no struct changed


def test_bounds_declared_in_the_public_header():
    text = open(os.path.join(ROOT, "include", "swg.h")).read()
    for name in NEW_SYMBOLS:
        assert "int %s(swg_ctx *ctx, const swg_db *db," % name in text, name
    assert "#define SWG_ABI_VERSION 3" in text


def test_bounds_null_arguments(swg):
    q = np.ones(4, dtype=np.int8)
    off = np.array([0, 4], dtype=np.uint64)
    nh = (C.c_size_t * 1)(0)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)                                    # noqa: E731
    calls = {
        "swg_align_bounds": lambda: swg.lib.swg_align_bounds(None, None, None, 0, None),
        "swg_align_bounds_multi": lambda: swg.lib.swg_align_bounds_multi(None, None, vp(q), vp(off), 1, None, 0,
                                                                        C.cast(nh, C.c_void_p), None),
        "swg_align_bounds_multi_pssm": lambda: swg.lib.swg_align_bounds_multi_pssm(None, None, None, None, 0, None, 0, None, None),
    }
    for name, call in calls.items():
        assert call() == swg.SWG_ERR_ARG, name
        assert name in swg.lib.swg_global_error().decode(), name
    out = np.zeros(4, dtype=np.uint32)
    assert swg.lib.swg_debug_bounds_last(None, vp(out)) == swg.SWG_ERR_ARG
    assert "swg_debug_bounds_last" in swg.lib.swg_global_error().decode()


def _run(*a):
    return subprocess.run([CLI, "--substitution_matrix", B62] + [str(x) for x in a], stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, text=True, timeout=120)


def test_cli_bounds_flag_checks(swg, tmp_path):
    q = tmp_path / "q.fa"
    q.write_text(">q\nACDEFG\n")
    db = tmp_path / "d.fa"
    db.write_text(">d\nACDEFGKLMNP\n")
    r = _run("--bounds", "--files", q, db)
    assert r.returncode != 0 and "usage:" in r.stderr and "--bounds reports the alignment coordinates of the --topk hits" in r.stderr, r.stderr
    r = _run("--topk", 3, "--bounds", "--align", "--files", q, db)
    assert r.returncode != 0 and "usage:" in r.stderr and "does not combine with --align" in r.stderr, r.stderr
    r = _run("--topk", 3, "--bounds", "--gapless", "--files", q, db)
    assert r.returncode != 0 and "usage:" in r.stderr and "does not combine with --gapless" in r.stderr, r.stderr
    r = _run("--topk", 3, "--bounds", "--gpus", 2, "--files", q, db)
    assert r.returncode != 0 and "usage:" in r.stderr and "--bounds works with one GPU" in r.stderr, r.stderr
    # the flag is in the usage text, and takes no parameter (valid in last position)
    r = _run("--help")
    assert "--bounds" in r.stderr and "length N" in r.stderr
    r = _run("--files", q, db, "--bounds")
    assert "Unknown argument" not in r.stderr and "give --topk K" in r.stderr, r.stderr
