"""CPU: the host half of the six-frame translation -- swg_codon_table, swg_translate_seq (the twin of the device kernel)
against the string model of translate_cases.py, and the arithmetic of swg_translate_hit / swg_translate_coords."""
import ctypes as C
import os

import numpy as np
import pytest

import translate_cases as tc
from conftest import ROOT

NEW = ("swg_codon_table", "swg_translate_seq", "swg_translate_flat", "swg_translate_hit", "swg_translate_coords", "swg_db_translate",
       "swg_db_translate_info")
CODES = {str(k): dict(code=k, letters=v) for k, v in tc.TABLES.items()}
CODES["custom"] = dict(code=tc.table_indices(tc.CUSTOM), letters=tc.CUSTOM)


def _frames(swg, s, code=1, unknown=24):
    return swg.translate_seq(tc.indices(s), code=code, unknown=unknown)


def _equal(got, want_letters):
    return len(got) == 6 and all(np.array_equal(g, tc.indices(w)) for g, w in zip(got, want_letters))


def test_abi_and_binding(swg):
    text = open(os.path.join(ROOT, "include", "swg.h")).read()
    for name in NEW:
        assert name in swg.ABI_SYMBOLS and hasattr(swg.lib, name), name
        assert " %s(" % name in text, name
    assert swg.lib.swg_abi_version() == 3          # functions and structs were added, no struct changed
    assert C.sizeof(swg.TranslateParams) == 65 and C.sizeof(swg.TranslateInfo) == 112
    assert swg.TRANSLATE_TILE_CODONS >= 64 and swg.TRANSLATE_TILE_CODONS % 4 == 0
    for method in ("translate", "translate_info"):
        assert callable(getattr(swg.Database, method, None)), method
    for fn in ("codon_table", "translate_seq", "translate_hit", "translate_coords"):
        assert callable(getattr(swg, fn, None)), fn


def test_the_seven_tables(swg):
    for ncbi, letters in tc.TABLES.items():
        assert np.array_equal(swg.codon_table(ncbi), tc.table_indices(letters)), ncbi
    for bad in (0, 7, 10, 12, -1):
        with pytest.raises(swg.SwgError) as e:
            swg.codon_table(bad)
        assert e.value.code == swg.SWG_ERR_ARG


@pytest.mark.parametrize("name", sorted(CODES))
def test_every_codon_in_every_frame(swg, name):
    code, letters = CODES[name]["code"], CODES[name]["letters"]
    seen = [set() for _ in range(6)]
    for cname, s in tc.codon_cases().items():
        assert _equal(_frames(swg, s, code), tc.model(s, letters)), cname
        rc = tc.revcomp(s)
        for g in range(6):
            strand, f = (s, g) if g < 3 else (rc, g - 3)
            seen[g] |= {strand[a:a + 3] for a in range(f, len(strand) - 2, 3)}
    assert all(sg == set(tc.ALL_CODONS) for sg in seen)      # the cases do hold all 64 in each of the six


@pytest.mark.parametrize("name", sorted(CODES))
def test_random_sequences_against_the_model(swg, name):
    code, letters = CODES[name]["code"], CODES[name]["letters"]
    rng = np.random.default_rng(77)
    for trial in range(300):
        s = tc.random_nt(rng, int(rng.integers(0, 201)), "ACGTUNRY*")
        assert _equal(_frames(swg, s, code), tc.model(s, letters)), (trial, s)


def test_structural_cases_against_the_model(swg):
    for name, s in tc.structural_cases(swg.TRANSLATE_TILE_CODONS).items():
        assert _equal(_frames(swg, s), tc.model(s)), name


def test_u_is_t_and_non_bases_are_unknown(swg):
    assert _equal(_frames(swg, "AUGUUUUAA"), tc.model("ATGTTTTAA"))
    assert [swg.lib.swg_index_letter(int(v)) for v in _frames(swg, "AUGUUUUAA")[0]] == [ord(c) for c in "MF*"]
    for pos in range(3):
        for nb in "NRYKMSWBDHV*X":
            s = list("GCTGCTGCT")
            s[3 + pos] = nb
            got = _frames(swg, "".join(s))
            assert got[0].tolist() == tc.indices("AXA").tolist(), (pos, nb)          # GCN is not resolved
            assert got[3].tolist() == tc.indices("SXS").tolist(), (pos, nb)
            other = _frames(swg, "".join(s), unknown=2)
            assert other[0].tolist() == [1, 2, 1] and other[3].tolist() == [19, 2, 19]
    assert all(f.size == 0 for f in _frames(swg, ""))
    assert [f.size for f in _frames(swg, "ACGT")] == [1, 1, 0, 1, 1, 0]


def test_flat_equals_one_by_one(swg):
    rng = np.random.default_rng(5)
    seqs = [tc.random_nt(rng, int(n), "ACGTN") for n in rng.integers(0, 90, size=200)]
    flat, off = tc.flat_of(seqs)
    out, out_off = swg.translate_flat(flat, off, code=4)
    assert out_off.size == 6 * len(seqs) + 1 and int(out_off[-1]) == out.size
    for i, s in enumerate(seqs):
        for g, want in enumerate(tc.model(s, tc.TABLES[4])):
            assert np.array_equal(out[int(out_off[6 * i + g]):int(out_off[6 * i + g + 1])], tc.indices(want)), (i, g)


def test_bad_tables_are_refused(swg):
    for entry in (0, 32, -1):
        t = swg.codon_table(1).copy()
        t[17] = entry
        with pytest.raises(swg.SwgError) as e:
            swg.translate_seq(tc.indices("ACGTACGT"), code=t)
        assert e.value.code == swg.SWG_ERR_ARG and "swg_translate_seq" in str(e.value)
    for unknown in (0, 32):
        with pytest.raises(swg.SwgError) as e:
            swg.translate_seq(tc.indices("ACGTACGT"), unknown=unknown)
        assert e.value.code == swg.SWG_ERR_ARG


def test_hit_and_coords(swg):
    for index in (0, 1, 5, 6, 7, 6 * 123456 + 4, 0xFFFFFFEF):
        assert swg.translate_hit(index) == (index // 6, index % 6)
    for L in range(0, 41):
        for frame in range(6):
            cons = tc.consumed(L, frame)
            n = len(cons)
            assert n == len(tc.model("A" * L)[frame])
            for b in range(n):
                for e in range(b + 1, n + 1):
                    nb, ne = swg.translate_coords(frame, L, b, e)
                    assert nb < ne and set(range(nb, ne)) == set().union(*cons[b:e]), (L, frame, b, e)
            for b, e in ((0, n + 1), (n, n + 1), (0, 0), (n, n), (2, 1)):       # past the frame's end, or empty
                with pytest.raises(swg.SwgError) as err:
                    swg.translate_coords(frame, L, b, e)
                assert err.value.code == swg.SWG_ERR_ARG
        for f in range(3):                                                       # the two strands tile from opposite ends
            n = len(tc.consumed(L, f))
            if n:
                assert swg.translate_coords(f, L, 0, n) == (f, f + 3 * n)
                assert swg.translate_coords(3 + f, L, 0, n) == (L - f - 3 * n, L - f)
                for k in range(n):
                    assert swg.translate_coords(f, L, k, k + 1)[0] - f == L - f - swg.translate_coords(3 + f, L, k, k + 1)[1]
    for frame in (-1, 6):
        with pytest.raises(swg.SwgError):
            swg.translate_coords(frame, 30, 0, 1)
