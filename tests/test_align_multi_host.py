"""Alignments of a batch's hits, host side (no GPU): swg_align_hits_multi, swg_align_hits_multi_pssm and
swg_align_ops_bound_multi are exported and bound, the ops bound is the longest query of the batch plus the shard's
longest sequence plus 1, and a NULL context is refused with the global error set."""
import ctypes as C

import numpy as np

NEW = ("swg_align_hits_multi", "swg_align_hits_multi_pssm", "swg_align_ops_bound_multi")


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def test_abi_exports_align_hits_multi(swg):
    for name in NEW:
        assert name in swg.ABI_SYMBOLS and hasattr(swg.lib, name), name
    assert callable(getattr(swg.Context, "align_hits_multi", None))
    assert callable(getattr(swg.Context, "align_hits_multi_pssm", None))


def test_ops_bound_multi_whole_database(swg):
    flat, off = swg.synth_db(0x5EED0001, 1024)
    db = swg.Database(flat, off)
    longest = int(np.diff(off.astype(np.int64)).max())
    qoff = np.array([0, 128, 300, 301, 1001], dtype=np.uint64)           # lengths 128, 172, 1, 700
    assert swg.lib.swg_align_ops_bound_multi(db.handle, _vp(qoff), 4) == 700 + longest + 1
    assert swg.lib.swg_align_ops_bound_multi(db.handle, _vp(qoff), 2) == 172 + longest + 1
    db.close()


def test_ops_bound_multi_shard_and_offset(swg):
    """A shard's bound uses the shard's own longest sequence; offsets need not start at 0."""
    flat, off = swg.synth_db(0x5EED0009, 300, max_len=5000)
    lens = np.diff(off.astype(np.int64))
    half = swg.Database(flat, off, shard_rank=1, shard_count=2)
    mine = [int(i) for i in half.order() if i != 0xFFFFFFFF]
    assert 0 < len(mine) < len(lens)
    longest = int(lens[mine].max())
    qoff = np.array([5000, 5060, 5200], dtype=np.uint64)                 # lengths 60, 140
    assert swg.lib.swg_align_ops_bound_multi(half.handle, _vp(qoff), 2) == 140 + longest + 1
    assert swg.lib.swg_align_ops_bound_multi(half.handle, _vp(qoff[1:]), 1) == 140 + longest + 1
    half.close()


def test_ops_bound_multi_null(swg):
    flat, off = swg.synth_db(3, 50)
    db = swg.Database(flat, off)
    qoff = np.array([0, 10], dtype=np.uint64)
    assert swg.lib.swg_align_ops_bound_multi(None, _vp(qoff), 1) == 0
    assert swg.lib.swg_align_ops_bound_multi(db.handle, None, 1) == 0
    db.close()


def test_align_hits_multi_null_context(swg):
    q = np.ones(4, dtype=np.int8)
    off = np.array([0, 4], dtype=np.uint64)
    hits = (swg.Hit * 1)()
    nh = (C.c_size_t * 1)(1)
    out = (swg.Alignment * 1)()
    for name in ("swg_align_hits_multi", "swg_align_hits_multi_pssm"):
        src = q if name == "swg_align_hits_multi" else np.zeros((4, 32), dtype=np.int8)
        rc = getattr(swg.lib, name)(None, None, _vp(src), _vp(off), 1, C.cast(hits, C.c_void_p), 1,
                                    C.cast(nh, C.c_void_p), C.cast(out, C.c_void_p), None, 0)
        assert rc == swg.SWG_ERR_ARG
        assert name.encode() + b": NULL context" in swg.lib.swg_global_error()
