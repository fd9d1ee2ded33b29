"""GPU (-m gpu): swg_db_composition -- the residue counts of a resident database, view or shard against numpy.bincount,
exactly; the padding bytes that fill a sequence up to whole dwords are never counted."""
import numpy as np
import pytest

import gapless_cases as gc

pytestmark = pytest.mark.gpu


def _db(n, seed, lengths=None):
    rng = np.random.default_rng(seed)
    lengths = lengths if lengths is not None else rng.integers(1, 90, size=n)
    seqs = [rng.integers(1, 32, size=int(l)).astype(np.int8) for l in lengths]
    return seqs, gc.pack(seqs)


def _want(seqs, sel=None):
    sel = range(len(seqs)) if sel is None else sel
    picked = [seqs[i] for i in sel]
    return np.bincount(np.concatenate(picked), minlength=32).astype(np.uint64) if picked else np.zeros(32, dtype=np.uint64)


def test_lengths_around_a_dword(swg, ctx):
    """Sequences of 1..5 residues (every remainder modulo 4) and one of 300 (several rounds of a wavefront)."""
    seqs, (flat, off) = _db(6, 1, lengths=[1, 2, 3, 4, 5, 300])
    db = swg.Database(flat, off).upload(ctx)
    counts = db.composition(ctx)
    assert np.array_equal(counts, _want(seqs)) and counts[0] == 0 and int(counts.sum()) == db.residues == len(flat)
    db.close()


def test_two_bins_a_view_and_a_shard(swg, ctx):
    seqs, (flat, off) = _db(129, 2)
    db = swg.Database(flat, off).upload(ctx)
    counts = db.composition(ctx)
    assert np.array_equal(counts, _want(seqs)) and counts[0] == 0 and int(counts.sum()) == len(flat)
    assert np.array_equal(db.composition(ctx), counts)
    # a view of every third sequence walks its own slots over the parent's bytes
    third = list(range(0, 129, 3))
    view = db.view(ctx, third)
    got = view.composition(ctx)
    assert np.array_equal(got, _want(seqs, third)) and got[0] == 0 and int(got.sum()) == view.residues
    empty = db.view(ctx, [])
    assert not empty.composition(ctx).any()
    empty.close()
    view.close()
    db.close()


def test_shards_add_up(swg, ctx):
    seqs, (flat, off) = _db(300, 3)
    parts = []
    for rank in range(2):
        shard = swg.Database(flat, off, shard_rank=rank, shard_count=2).upload(ctx)
        held = np.sort(shard.order()[shard.order() != 0xFFFFFFFF]).tolist()
        got = shard.composition(ctx)
        assert np.array_equal(got, _want(seqs, held)) and got[0] == 0 and int(got.sum()) == shard.residues, rank
        assert 0 < len(held) < 300
        parts.append(got)
        shard.close()
    assert np.array_equal(parts[0] + parts[1], _want(seqs))


def test_a_database_that_is_not_resident(swg, ctx):
    _, (flat, off) = _db(10, 4)
    db = swg.Database(flat, off)
    with pytest.raises(swg.SwgError) as e:
        db.composition(ctx)
    assert e.value.code == swg.SWG_ERR_STATE
    db.close()
