"""Views (swg_db_view), host side: which sorted ranks of a database a list of original indices selects.  No GPU: the
test hook swg_debug_view_ranks runs the selection the view is built from, and numpy restates it -- the rank of an
original index is its position in topk_cases.sorted_order (length descending, stable), the selection is the set of those
ranks, ascending, which keeps the parent's order."""
import ctypes as C

import numpy as np
import pytest

import topk_cases as tc


def _db(swg, n=1000, seed=0x71E3, **kw):
    flat, off = swg.synth_db(seed, n, min_len=1, max_len=600)
    return swg.Database(flat, off, **kw), off


def _want(off, indices):
    """Ranks of the distinct listed indices in the whole database's sorted order, ascending."""
    order = tc.sorted_order(off)
    rank_of = np.empty(len(order), dtype=np.int64)
    rank_of[order] = np.arange(len(order))
    return np.unique(rank_of[np.asarray(indices, dtype=np.int64)])


def test_abi_exports_views(swg):
    for name in ("swg_db_view", "swg_group_select"):
        assert name in swg.ABI_SYMBOLS and hasattr(swg.lib, name), name
    assert hasattr(swg.lib, "swg_debug_view_ranks")
    assert callable(getattr(swg.Database, "view", None)) and callable(getattr(swg.Group, "select", None))


def test_shuffled_lists_with_duplicates(swg):
    db, off = _db(swg)
    rng = np.random.default_rng(5)
    for size in (2, 127, 128, 129, 700):
        ix = rng.choice(1000, size=size, replace=False)
        ix = rng.permutation(np.concatenate([ix, ix[: size // 2], ix[:1]]))       # duplicates, any order
        got = db.debug_view_ranks(ix)
        assert np.array_equal(got, _want(off, ix)), size
        assert np.array_equal(db.order()[got], tc.sorted_order(off)[got])         # ranks are slots of the packed database
    db.close()


def test_single_all_and_empty(swg):
    db, off = _db(swg, n=333)
    for i in (0, 332, 17):
        assert np.array_equal(db.debug_view_ranks([i]), _want(off, [i]))
    assert np.array_equal(db.debug_view_ranks(np.arange(333)[::-1]), np.arange(333))
    assert db.debug_view_ranks(np.zeros(0, dtype=np.uint32)).size == 0
    n = C.c_size_t(99)
    assert swg.lib.swg_debug_view_ranks(db.handle, None, 0, None, C.byref(n)) == swg.SWG_OK and n.value == 0
    db.close()


def test_sharded_database_drops_other_shards_indices(swg):
    flat, off = swg.synth_db(0x71E4, 1000, min_len=1, max_len=600)
    rng = np.random.default_rng(6)
    ix = rng.choice(1000, size=400, replace=False)
    ix = np.concatenate([ix, ix[:50]])
    distinct = set(int(v) for v in ix)
    total = 0
    for r in range(3):
        shard = swg.Database(flat, off, r, 3)
        mine = shard.order()
        got = shard.debug_view_ranks(ix)
        # the slots of this shard whose sequence is listed, ascending
        want = np.nonzero(np.isin(mine, ix))[0]
        assert np.array_equal(got, want), r
        assert set(int(v) for v in mine[got]) <= distinct
        total += got.size
        shard.close()
    assert total == len(distinct)


def test_out_of_range_index_is_an_argument_error(swg):
    db, _ = _db(swg, n=100)
    for bad in ([100], [3, 4, 0xFFFFFFFF], [99, 100]):
        with pytest.raises(swg.SwgError) as e:
            db.debug_view_ranks(bad)
        assert e.value.code == swg.SWG_ERR_ARG and "outside the database" in str(e.value)
    assert db.debug_view_ranks([99]).size == 1
    # a shard counts the WHOLE database's indices: one of another shard is in range, one past the total is not
    flat, off = swg.synth_db(0x71E5, 300, min_len=1, max_len=200)
    shard = swg.Database(flat, off, 1, 3)
    assert shard.total_count == 300
    with pytest.raises(swg.SwgError) as e:
        shard.debug_view_ranks([300])
    assert e.value.code == swg.SWG_ERR_ARG
    shard.close()
    db.close()
