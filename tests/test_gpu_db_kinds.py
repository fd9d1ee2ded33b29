"""GPU (-m gpu): every call family on every kind of database handle (tests/db_kinds_cases.py: KINDS x FAMILIES).

include/swg.h promises that every call which takes a swg_db takes a root, a shard swg_db_pack kept, a shard cut elsewhere,
a view, a masked copy and a loaded image unchanged, and that the answers of a sharded run are the whole database's after
a merge.  A shard is where a kernel or its read-out can go wrong with no root-only test noticing: order[] holds indices
far above count, every by-index table has total_count entries, the bins' lengths jump, a shard may hold only the global
order's partial last bin, or nothing at all, and re-runs on wider cells travel through the slot-to-index map.

Every answer must equal the CPU's truth restricted to the handle's members -- integers, strings and keys exactly; the
values and the info record of a built PSSM within test_gpu_pssm_build._assert_same's bounds, the only tolerances here.
Outputs are pre-filled (db_kinds_cases: 0x5A), so what a call must not write is part of each comparison."""
import numpy as np
import pytest

import db_kinds_cases as dk
from test_gpu_parity import _reset_options
from test_gpu_pssm_build import _assert_same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(swg, orc):
    """One context for the module: autotune off, every other option at its default."""
    c = swg.Context(0)
    _reset_options(c)
    c.set_option("autotune", 0)
    e = dk.Env(swg, c)
    c.set_scoring(e.w["sub"], *dk.GAPS)
    yield e
    c.close()


def _check_handle(e, kind, db):
    w = e.w
    members = kind.members(w)
    assert db.count == len(members) and db.total_count == kind.n_total, kind.name
    order = db.order().astype(np.int64)
    assert np.array_equal(np.sort(order), kind.g(members)), kind.name
    back = {int(kind.g(i)): int(i) for i in members}
    assert (np.diff(w["lens"][[back[int(o)] for o in order]]) <= 0).all(), kind.name      # the parent's sorted order, kept
    assert db.residues == int(w["lens"][members].sum()), kind.name
    if kind.masked and not kind.view:
        info, base = db.mask_info(), kind.base_members(w)
        assert (info["residues_masked"], info["sequences_masked"], info["segments"]) == \
            (int(w["masked_residues"][base].sum()), int((w["masked_residues"][base] > 0).sum()), int(w["mask_segments"][base].sum())), info


def _close(chain):
    for d in reversed(chain):
        d.close()


@pytest.mark.parametrize("kind", list(dk.KINDS))
def test_every_family_on(env, kind, tmp_path):
    kind = dk.KINDS[kind]
    db, chain = kind.open(env.swg, env.ctx, env.w, tmp_path)
    try:
        _check_handle(env, kind, db)
        cells = 0
        for family in dk.FAMILIES:
            where = "%s / %s" % (kind.name, family.name)
            want = dk.expected(family, kind)
            dk.same(family.run(env, kind, db), want, where, _assert_same)
            cells += 1
            if not family.takes_hits:
                continue
            # a hit the handle does not hold, and a valid index that a view does not select: refused, outputs untouched,
            # and the next valid call gives the right answer
            for what, bad in (("outside", kind.outside(env.w)), ("unselected", kind.unselected(env.w))):
                if bad is not None:
                    dk.same(family.run(env, kind, db, bad), dk.refused_arg(env.swg), "%s, one hit %s (%d)" % (where, what, bad), _assert_same)
                    dk.same(family.run(env, kind, db), want, "%s after the refusal" % where, _assert_same)
        assert cells == len(dk.FAMILIES)
    finally:
        _close(chain)


def test_cut_elsewhere_gives_what_rank1of3_gives(env, tmp_path):
    """Index for index after the remap: the call's own answers compared, not each with the truth."""
    rank1, cut = dk.KINDS["rank1of3"], dk.KINDS["cut_elsewhere"]
    db1, chain1 = rank1.open(env.swg, env.ctx, env.w, tmp_path)
    db2, chain2 = cut.open(env.swg, env.ctx, env.w, tmp_path)
    try:
        assert np.array_equal(np.sort(db2.order().astype(np.int64)), cut.g(np.sort(db1.order().astype(np.int64))))
        for family in dk.FAMILIES:
            dk.same(family.run(env, cut, db2), dk.remap(family.run(env, rank1, db1), cut), "cut_elsewhere == rank1of3 / " + family.name, _assert_same)
    finally:
        _close(chain2)
        _close(chain1)


def _merge(swg, parts, want, where):
    """The ranks' answers merged as a sharded run merges them -> compared with the whole database's expected answer."""
    if isinstance(want, dk.ByIndex):
        written = sum((p.arr != dk.FILL32).astype(np.int64) for p in parts)
        assert (written == 1).all(), (where, "entries not written by exactly one rank", np.nonzero(written != 1))
        merged = np.full_like(want.arr, dk.FILL32)
        for p in parts:
            merged = np.where(p.arr != dk.FILL32, p.arr, merged)
        dk.same(dk.ByIndex(merged), want, where, None)
    elif isinstance(want, list) and all(isinstance(x, dk.H) for x in want) and all(isinstance(x, dk.H) for p in parts for x in p):
        keys = np.array([swg.hit_key(h.score, h.index) for p in parts for h in p], dtype=np.uint64)
        merged = swg.topk_merge_keys(keys, max(len(want), 1)) if len(keys) else []
        assert [dk.H(*h) for h in merged] == want, (where, merged, want)
        assert [swg.hit_key(*h) for h in merged] == sorted((swg.hit_key(*h) for h in merged), reverse=True), where
    elif isinstance(want, dict):
        if "n_total" in want and isinstance(want["n_total"], int):         # a thresholded search: the union is the list, nothing more
            assert sum(len(p["hits"]) for p in parts) == len(want["hits"]), where
        elif "n_total" in want:                                            # its batch form: row by row
            for i, row in enumerate(want["hits"]):
                assert sum(len(p["hits"][i]) for p in parts) == len(row), (where, i)
        for k in want:
            if k == "rescored":                                            # some rank holds what reaches the ceiling
                assert any(p[k] for p in parts) == want[k], where
                continue
            _merge(swg, [p[k] for p in parts], want[k], "%s.%s" % (where, k))
    elif isinstance(want, (list, tuple)):
        for n, x in enumerate(want):
            _merge(swg, [p[n] for p in parts], x, "%s[%d]" % (where, n))
    elif isinstance(want, bool):
        assert all(parts) == want, where
    elif isinstance(want, np.ndarray) and want.dtype == np.int32:          # scores parallel to a candidate list: position by position
        _merge(swg, [dk.ByIndex(p) for p in parts], dk.ByIndex(want), where)
    elif isinstance(want, np.ndarray):
        assert np.array_equal(sum(parts[1:], parts[0]), want), (where, parts, want)      # residue counts: they add up
    else:
        assert sum(parts) == want, (where, parts, want)                 # n_total, residues: they add up


@pytest.mark.parametrize("count", [3, 7])
def test_ranks_merge_to_the_whole(env, count, tmp_path):
    w, whole = env.w, dk.KINDS["whole"]
    families = [f for f in dk.FAMILIES if f.name in dk.MERGED]         # every family with a search result, and the composition
    answers, masks, counts = [], [], []
    for r in range(count):
        kind = dk.Kind("rank%dof%d" % (r, count), (r, count))
        db, chain = kind.open(env.swg, env.ctx, w, tmp_path)
        try:
            _check_handle(env, kind, db)
            counts.append(db.count)
            answers.append([f.run(env, kind, db) for f in families])
            masked = db.mask(env.ctx)
            chain.append(masked)
            masks.append(masked.mask_info())
        finally:
            _close(chain)
    assert sum(counts) == dk.N and (count != 7 or counts[5:] == [37, 0])
    for n, f in enumerate(families):
        _merge(env.swg, [a[n] for a in answers], dk.expected(f, whole), "%d ranks / %s" % (count, f.name))
    for key in ("residues_masked", "sequences_masked", "segments"):
        assert sum(m[key] for m in masks) == w["mask_totals"][key], (key, masks)
