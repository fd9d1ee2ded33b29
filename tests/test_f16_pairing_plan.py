"""The packed-f16 cells' two pairings of the sequences' profile words (v_perm_b32, or v_pk_fma_f16 on a (score, 1.0)
profile of twice the size), as the cost model assigns them on the host (swg_debug_plan_f16: no device involved)."""
import pytest

import swg_loader


@pytest.fixture(scope="module")
def swg():
    return swg_loader.load()


def _plans(swg, seed, n, lq, pairs, **kw):
    if kw:
        q = swg.synth_query(seed, lq)
        flat, off, _ = swg.synth_db(seed, n, query=q, **kw)
    else:
        flat, off = swg.synth_db(seed, n)
    db = swg.Database(flat, off)
    try:
        return {fp: db.debug_plan(lq, f16_pair=fp) for fp in pairs}
    finally:
        db.close()


def test_config4_takes_the_fma_pairing(swg):
    p = _plans(swg, 0x5EED0004, 1250000, 3000, (0, 1, 2))
    auto, perm, fma = p[0], p[1], p[2]
    # 16 lanes x 32 columns, six passes: the doubled profile (64 KB) and twelve wavefronts' records fit one workgroup per CU
    assert (auto["fma"], auto["K"], auto["G"], auto["passes"]) == (1, 32, 16, 6), auto
    assert auto["lds_bytes"] <= 160 * 1024 and auto["W"] * auto["workgroups"] == 12 * 256, auto
    assert fma == auto
    assert (perm["fma"], perm["K"], perm["G"], perm["W"], perm["passes"]) == (0, 32, 16, 4, 6), perm
    assert perm["lds_bytes"] <= 160 * 1024
    assert auto["est_us"] < perm["est_us"]


def test_wide_groups_at_32_columns_keep_the_perm_pairing(swg):
    # config 5's f16 geometry: 64 lanes x 32 columns would need a 256 KB profile with the fma pairing
    p = _plans(swg, 0x5EED0005, 100000, 8192, (0, 2), fraction=0.01, subst=0.05)
    for fp, pl in p.items():
        assert (pl["fma"], pl["K"], pl["G"]) == (0, 32, 64), (fp, pl)
        assert pl["lds_bytes"] <= 160 * 1024


def test_every_plan_fits_its_lds(swg):
    flat, off = swg.synth_db(0x5EED0003, 50000)
    db = swg.Database(flat, off)
    try:
        for lq in (40, 128, 367, 500, 1000, 2300, 3000, 5000):
            for fp in (0, 1, 2):
                pl = db.debug_plan(lq, f16_pair=fp)
                assert pl["lds_bytes"] <= 160 * 1024, (lq, fp, pl)
                if fp == 1:
                    assert pl["fma"] == 0 and pl["long_fma"] == 0, (lq, pl)
    finally:
        db.close()
