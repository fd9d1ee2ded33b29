"""Candidate lists (swg_search_lists), host side: the job table a batch of per-query lists becomes.  No GPU: the test hook
swg_debug_list_jobs runs swg_list_jobs, and numpy restates it -- segment i is the distinct slots of the database that
list i selects, ascending (the database is sorted by length, so that is longest first), an odd segment ends in an empty
slot (~0), and row i's pairs are [prefix[i], prefix[i + 1]) with prefix[i + 1] = prefix[i] + ceil(|S_i| / 2)."""
import ctypes as C

import numpy as np
import pytest

import topk_cases as tc

EMPTY = 0xFFFFFFFF
N = 1000


@pytest.fixture(scope="module")
def db_off(swg):
    flat, off = swg.synth_db(0x715A, N, min_len=1, max_len=600)
    db = swg.Database(flat, off)
    yield db, off
    db.close()


def _want(slot_of, lists):
    """The job table restated: slot_of[index] = the database's slot of an original index, -1 = not held."""
    slots, prefix = [], [0]
    for l in lists:
        s = slot_of[np.asarray(l, dtype=np.int64)]
        s = np.unique(s[s >= 0])
        slots.extend(int(v) for v in s)
        if len(s) & 1:
            slots.append(EMPTY)
        prefix.append(len(slots) // 2)
    return np.array(slots, dtype=np.uint32), np.array(prefix, dtype=np.uint64)


def _slot_of_whole(off):
    order = tc.sorted_order(off)
    slot_of = np.empty(len(order), dtype=np.int64)
    slot_of[order] = np.arange(len(order))
    return slot_of


def _check(db, slot_of, lists, label):
    slots, prefix = db.debug_list_jobs(lists)
    w_slots, w_prefix = _want(slot_of, lists)
    assert np.array_equal(prefix, w_prefix), label
    assert np.array_equal(slots, w_slots), label
    return slots, prefix


def test_abi_exports_lists(swg):
    for name in ("swg_search_lists", "swg_search_lists_pssm"):
        assert name in swg.ABI_SYMBOLS and hasattr(swg.lib, name), name
    assert hasattr(swg.lib, "swg_debug_list_jobs")
    for name in ("search_lists", "search_lists_pssm"):
        assert callable(getattr(swg.Context, name, None)), name
    assert callable(getattr(swg.Database, "debug_list_jobs", None))
    assert swg.lib.swg_abi_version() == 3


def test_list_sizes_around_a_pair_and_a_bin(swg, db_off):
    db, off = db_off
    slot_of = _slot_of_whole(off)
    rng = np.random.default_rng(11)
    sizes = (0, 1, 2, 3, 127, 128, 129)
    lists = [rng.choice(N, size=s, replace=False) for s in sizes]
    slots, prefix = _check(db, slot_of, lists, "sizes")
    # the empty row has an empty range; an odd list ends in the empty slot and nowhere else is one
    assert prefix[0] == prefix[1] == 0
    for i, s in enumerate(sizes):
        seg = slots[2 * int(prefix[i]):2 * int(prefix[i + 1])]
        assert len(seg) == s + (s & 1), s
        assert np.all(seg[:s] != EMPTY) and (s % 2 == 0 or seg[-1] == EMPTY), s
        assert np.all(np.diff(seg[:s].astype(np.int64)) > 0), s              # ascending slots = longest first
        lens = np.diff(off.astype(np.int64))[tc.sorted_order(off)[seg[:s]]]
        assert np.all(np.diff(lens) <= 0), s


def test_shuffled_lists_with_duplicates_identical_lists_and_everything(swg, db_off):
    db, off = db_off
    slot_of = _slot_of_whole(off)
    rng = np.random.default_rng(12)
    pick = rng.choice(N, size=301, replace=False)
    dups = rng.permutation(np.concatenate([pick, pick[:150], pick[:1]]))
    same = rng.choice(N, size=77, replace=False)
    lists = [dups, same, same.copy(), np.arange(N)[::-1], np.zeros(0, dtype=np.uint32), same[::-1]]
    slots, prefix = _check(db, slot_of, lists, "shapes")
    seg = lambda i: slots[2 * int(prefix[i]):2 * int(prefix[i + 1])]
    assert len(seg(0)) == 302 and seg(0)[-1] == EMPTY                           # 301 distinct: duplicates collapse
    assert np.array_equal(seg(1), seg(2)) and np.array_equal(seg(1), seg(5))    # a sequence appears once per query
    assert np.array_equal(seg(3), np.arange(N, dtype=np.uint32))                # everything: the database's own order
    assert prefix[4] == prefix[5]


def test_a_shard_drops_foreign_indices(swg):
    flat, off = swg.synth_db(0x715B, N, min_len=1, max_len=600)
    shard = swg.Database(flat, off, shard_rank=1, shard_count=3)
    mine = shard.order()
    slot_of = np.full(N, -1, dtype=np.int64)
    slot_of[mine] = np.arange(len(mine))
    rng = np.random.default_rng(13)
    foreign = np.setdiff1d(np.arange(N), mine)
    lists = [rng.choice(N, size=200, replace=False), foreign[:40], np.concatenate([foreign[:5], mine[:3]]), mine[::-1]]
    slots, prefix = _check(shard, slot_of, lists, "shard")
    assert prefix[1] == prefix[2]                                               # a list of other shards' sequences: empty here
    assert prefix[3] - prefix[2] == 2 and slots[2 * int(prefix[3]) - 1] == EMPTY
    assert 0 < prefix[1] < 100
    shard.close()


def test_index_beyond_the_database_is_an_argument_error(swg, db_off):
    db, _ = db_off
    for lists in ([[N]], [[1, 2], [], [5, N + 7, 3]], [[0xFFFFFFFF]]):
        with pytest.raises(swg.SwgError) as e:
            db.debug_list_jobs(lists)
        assert e.value.code == swg.SWG_ERR_ARG and "outside the database" in str(e.value)
    with pytest.raises(swg.SwgError) as e:
        db.debug_list_jobs([[1, 2], [], [5, N + 7, 3]])
    assert "query 2" in str(e.value) and "entry 1" in str(e.value)              # the message names the query and the entry
    assert db.debug_list_jobs([[N - 1]])[0].size == 2
    n = C.c_size_t(9)
    assert swg.lib.swg_debug_list_jobs(db.handle, None, None, 0, None, 0, C.byref(n), None) == swg.SWG_OK and n.value == 0


def test_workgroups_are_dealt_by_work(swg, db_off):
    """Every row with pairs gets a workgroup, none more than its pairs keep busy, the grid stays within the chip's
    resident workgroups, rows with the most token blocks come first and empty rows get none."""
    db, off = db_off
    lens_sorted = np.diff(off.astype(np.int64))[tc.sorted_order(off)]
    rng = np.random.default_rng(14)
    lists = [rng.choice(N, size=s, replace=False) for s in (900, 0, 50, 3, 1, 50, 0, 400, 2)]
    slots, prefix = db.debug_list_jobs(lists)
    pairs = np.diff(prefix.astype(np.int64))
    blocks = np.array([sum((2 + int(lens_sorted[slots[2 * p]]) + 3) // 4 for p in range(int(prefix[i]), int(prefix[i + 1])))
                       for i in range(len(lists))])
    for per_wg, resident in ((16, 1024), (4, 768), (16, 4), (1, 100000)):
        deal = db.debug_list_deal(lists, per_wg, resident)
        rows = deal[:, 0].astype(np.int64)
        counts = np.bincount(rows, minlength=len(lists))
        assert np.all((counts > 0) == (pairs > 0)), (per_wg, resident)
        assert np.all(counts <= np.ceil(pairs / per_wg)), (per_wg, resident)
        assert len(deal) <= max(resident, int((pairs > 0).sum())), (per_wg, resident)
        order = [int(r) for i, r in enumerate(rows) if i == 0 or rows[i - 1] != r]       # each row's workgroups are adjacent
        assert len(order) == len(set(order)) and np.all(np.diff(blocks[order]) <= 0), (per_wg, resident)
        for r in order:                                                                 # the index within the row: 0, 1, 2 ..
            assert np.array_equal(deal[rows == r, 1], np.arange(counts[r])), (per_wg, resident, r)
    # in proportion to the work: with room to spare the largest list takes most of the grid, the small ones one each
    deal = db.debug_list_deal(lists, 16, 1024)
    counts = np.bincount(deal[:, 0].astype(np.int64), minlength=len(lists))
    assert counts[0] == np.ceil(pairs[0] / 16) and counts[7] == np.ceil(pairs[7] / 16) and counts[4] == 1 and counts[8] == 1
    deal = db.debug_list_deal(lists, 1, 64)
    counts = np.bincount(deal[:, 0].astype(np.int64), minlength=len(lists))
    spare = 64 - int((pairs > 0).sum())
    want = 1 + np.floor(spare * blocks / blocks.sum()).astype(np.int64)
    assert np.array_equal(counts[pairs > 0], np.minimum(want, pairs)[pairs > 0])
    assert db.debug_list_deal([[], []], 16, 1024).shape == (0, 2)
