"""Batches of position-specific queries, host side (no GPU): swg_search_multi_pssm is exported and refuses a NULL
context, and the CLI's --pssmlist argument checks (flag combinations, the list itself, every PSSM it names) are
reported before any device is touched."""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import ROOT
from test_pssm_host import write_ascii_pssm

CLI = os.path.join(ROOT, "seq-align-gpu_amd", "bin", "smith_waterman")
B62 = os.path.join(ROOT, "seq-align-gpu_amd", "data", "BLOSUM62.txt")


def test_abi_exports_search_multi_pssm(swg):
    assert "swg_search_multi_pssm" in swg.ABI_SYMBOLS and hasattr(swg.lib, "swg_search_multi_pssm")
    assert hasattr(swg.Context, "search_multi_pssm")


def test_search_multi_pssm_null_context(swg):
    pssm = np.zeros((4, 32), dtype=np.int8)
    off = np.array([0, 4], dtype=np.uint64)
    rc = swg.lib.swg_search_multi_pssm(None, None, pssm.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p), 1,
                                       None, None, 0, None, None)
    assert rc == swg.SWG_ERR_ARG
    assert b"swg_search_multi_pssm" in swg.lib.swg_global_error()


def _files(tmp_path, records=("acdefg", "KLMNP", "WYVAC")):
    q = tmp_path / "q.fa"
    q.write_text("".join(">r%d\n%s\n" % (i, s) for i, s in enumerate(records)))
    db = tmp_path / "d.fa"
    db.write_text(">d\nACDEFGKLMNP\n")
    paths = []
    for i, s in enumerate(records):
        p = tmp_path / ("r%d.pssm" % i)
        write_ascii_pssm(p, s.upper(), np.zeros((len(s), 20), dtype=np.int64))
        paths.append(p)
    lst = tmp_path / "list.txt"
    lst.write_text("".join("%s\n" % p for p in paths))
    return q, db, paths, lst


def _run(*a):
    return subprocess.run([CLI, "--substitution_matrix", B62] + [str(x) for x in a], stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, text=True, timeout=120)


def test_cli_pssmlist_flag_checks(tmp_path):
    """--pssmlist needs --allqueries, and takes neither --pssm nor --gpus: usage errors, as the other flag checks."""
    q, db, paths, lst = _files(tmp_path)
    r = _run("--files", q, db, "--pssmlist")
    assert r.returncode != 0 and "Unknown argument without parameter: --pssmlist" in r.stderr
    r = _run("--pssmlist", lst, "--files", q, db)
    assert r.returncode != 0 and "usage:" in r.stderr and "--allqueries" in r.stderr, r.stderr
    r = _run("--allqueries", "--pssmlist", lst, "--pssm", paths[0], "--files", q, db)
    assert r.returncode != 0 and "usage:" in r.stderr and "--pssm" in r.stderr, r.stderr
    r = _run("--allqueries", "--pssmlist", lst, "--gpus", "2", "--files", q, db)
    assert r.returncode != 0 and "usage:" in r.stderr and "--pssmlist" in r.stderr, r.stderr
    # --pssm with --allqueries stays refused as before
    r = _run("--allqueries", "--pssm", paths[0], "--files", q, db)
    assert r.returncode != 0 and "--pssm scores one query: it does not combine with --allqueries" in r.stderr


def test_cli_pssmlist_list_errors(tmp_path):
    """The list and the PSSMs it names are checked before the search: a missing list, a wrong number of entries, an
    unreadable PSSM, a PSSM that does not spell its record -- each error names the list entry or the record."""
    q, db, paths, lst = _files(tmp_path)
    r = _run("--allqueries", "--pssmlist", tmp_path / "none.txt", "--files", q, db)
    assert r.returncode != 0 and "PSSM list" in r.stderr and "none.txt" in r.stderr, r.stderr
    short = tmp_path / "short.txt"
    short.write_text("%s\n\n%s\n" % (paths[0], paths[1]))                 # (blank lines name nothing)
    r = _run("--allqueries", "--pssmlist", short, "--files", q, db)
    assert r.returncode != 0 and "names 2 PSSMs for 3 query records" in r.stderr, r.stderr
    missing = tmp_path / "missing.txt"
    missing.write_text("%s\n%s\n%s\n" % (paths[0], tmp_path / "none.pssm", paths[2]))
    r = _run("--allqueries", "--pssmlist", missing, "--files", q, db)
    assert r.returncode != 0 and "PSSM list entry 2 (query record #1)" in r.stderr, r.stderr
    swapped = tmp_path / "swapped.txt"
    swapped.write_text("%s\n%s\n%s\n" % (paths[0], paths[2], paths[1]))
    r = _run("--allqueries", "--pssmlist", swapped, "--files", q, db)
    assert r.returncode != 0 and "does not spell query record #1" in r.stderr and str(paths[2]) in r.stderr, r.stderr
    longer = tmp_path / "longer.pssm"
    write_ascii_pssm(longer, "WYVACA", np.zeros((6, 20), dtype=np.int64))
    bad = tmp_path / "bad.txt"
    bad.write_text("%s\n%s\n%s\n" % (paths[0], paths[1], longer))
    r = _run("--allqueries", "--pssmlist", bad, "--files", q, db)
    assert r.returncode != 0 and "does not spell query record #2" in r.stderr, r.stderr
