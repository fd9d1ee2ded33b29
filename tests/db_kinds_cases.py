"""Shared by the database-kinds matrix (plain module, no tests of its own): every call family on every kind of swg_db.

One world -- 677 sequences (five whole bins of 128 and one of 37), BLOSUM62, gaps -11/-1, three index queries with their
PSSM twins sub[query] -- and two tables:

  KINDS     how a handle is made (a root, the shards swg_db_pack keeps, a shard cut elsewhere, a view, a masked copy, a
            view of that, an image loaded from a file) and which original indices it holds;
  FAMILIES  (name, run on a handle, expected from truth and members, takes hits).

A new call family or a new kind of database is one row here; tests/test_gpu_db_kinds.py runs every family on every kind
and tests/test_db_kinds_cases_host.py proves on the CPU what that relies on.  Every truth comes from the CPU: the
oracle, gapless_numpy, the host twins.  Expected answers are written in the world's indices and carried into a handle's
own by remap(), so that the shard cut elsewhere (other indices, another total) is the same row as the rest.

Everything a call may write is handed over filled with the byte 0x5A: a score array of total_count entries, the hit rows
of the batch calls, the alignment and count rows.  An answer holds the whole array, so "exactly the members' entries
are written" and "slots past n_hits[i] stay untouched" are part of the comparison."""
import ctypes as C
import functools
import os
import re
from collections import namedtuple

import numpy as np

import above_multi_cases as amc
import gapless_cases as gc
import pssm_build_cases as pc
from test_gpu_stats import counts_of

N = 5 * 128 + 37
BIN = 128
GAPS = (-11, -1)
SEED = 20262
TOP = 16                       # the truth's top list: its members on a handle are the hits of the hit-taking families
K = 12
MIN_HSP = 40
N_TOTAL_ELSEWHERE = 100000
FILL = 0x5A
FILL32 = 0x5A5A5A5A            # (no score of this world comes near it)
LEVELS = ("above_best", "tenth", "one")

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def f16_ceiling():
    """The score at which the f16 cells flag a pair, as the library's header spells it."""
    text = open(os.path.join(_ROOT, "seq-align-gpu_amd", "csrc", "swg_host_internal.h")).read()
    return int(re.search(r"#define\s+SWG_F16_CEILING\s+(\d+)", text).group(1))


def elsewhere(i):
    """The global index of original sequence i in the database the cut-elsewhere shard belongs to."""
    return 7 + 131 * np.asarray(i, dtype=np.int64)


# ---- the world --------------------------------------------------------------------------------------------------------
# (rank in the length order, query): where each relative is planted.  Bins are ranks 0-127, 128-255, ...; the ranks of
# three hold bins {0, 3}, {1, 4} and {2, 5}.
NEAR_COPIES = (5, 40, 129, 130, 131)                                  # of the 600-column query: bins 0 and 1
PLANTS = {0: ((15, "gapped"), (100, "plain"), (150, "gapped"), (240, "plain"), (270, "gapped"), (330, "plain"), (370, "plain"),
              (400, "plain"), (440, "plain")),
          1: ((25, "gapped"), (110, "plain"), (160, "gapped"), (200, "plain"), (250, "plain"), (265, "plain"), (300, "plain"),
              (320, "plain"), (390, "plain"), (135, "repeat")),
          2: ((20, "gapped"), (180, "plain"), (280, "plain"), (350, "plain"), (420, "plain"))}
LOW_COMPLEXITY = (50, 66)                                             # columns of the 130-column query that are one residue


def _fit(rng, core, n):
    """core cut or padded with random residues to exactly n residues."""
    if len(core) >= n:
        a = (len(core) - n) // 2
        return core[a:a + n].copy()
    left = int(rng.integers(0, n - len(core) + 1))
    return np.concatenate([pc.random_seq(rng, left), core, pc.random_seq(rng, n - len(core) - left)]).astype(np.int8)


def _relative(rng, q, style, subst, keep=()):
    lq = len(q)
    if style == "gapped":
        return pc.relative(rng, q, subst, keep, ins=[(lq // 3, 2)], dele=[(2 * lq // 3, 2)])
    if style == "repeat":                                             # the same 100 columns twice: two alignments of one pair
        return np.concatenate([pc.relative(rng, q, subst, keep, hi=100), pc.random_seq(rng, 20), pc.relative(rng, q, subst, keep, hi=100)])
    return pc.relative(rng, q, subst, keep)


@functools.lru_cache(maxsize=None)
def world():
    import swg_loader
    swg, orc = swg_loader.load(), swg_loader.oracle()
    rng = np.random.default_rng(SEED)
    sub = pc.table("BLOSUM62")
    q40, q130, q600 = pc.random_seq(rng, 40), pc.random_seq(rng, 130), pc.random_seq(rng, 600)
    q130[LOW_COMPLEXITY[0]:LOW_COMPLEXITY[1]] = pc.idx("S")
    rich = rng.random(600) < 0.8                                      # residues that score 7 to 11 against themselves
    q600[rich] = rng.choice([pc.idx(c) for c in "WCHYP"], size=int(rich.sum()), p=[0.3, 0.25, 0.2, 0.125, 0.125])
    queries = [q40, q130, q600]
    by_rank = np.sort(np.concatenate([[3000, 2200, 1500], rng.integers(600, 616, size=130),
                                      13 + (287 * rng.random(484) ** 3).astype(np.int64), rng.integers(1, 13, size=60)]))[::-1]
    assert len(by_rank) == N
    lens = np.zeros(N, dtype=np.int64)
    lens[rng.permutation(N)] = by_rank
    order = amc.sorted_order(np.concatenate([[0], np.cumsum(lens)]))
    seqs = [pc.random_seq(rng, int(n)) for n in lens]
    keep_low = tuple(range(*LOW_COMPLEXITY))
    for r in NEAR_COPIES:
        i = int(order[r])
        seqs[i] = _fit(rng, pc.relative(rng, q600, 0.01, ins=[(200, 1)], dele=[(400, 1)]), int(lens[i]))
    for qi, plants in PLANTS.items():
        for n, (r, style) in enumerate(plants):
            i = int(order[r])
            subst = (0.08, 0.12, 0.3)[qi] if style != "plain" else 0.1 + 0.03 * n
            seqs[i] = _fit(rng, _relative(rng, queries[qi], style, subst, keep_low if qi == 1 else ()), int(lens[i]))
    assert [len(s) for s in seqs] == lens.tolist()
    flat, off = pc.pack(seqs)
    mflat, totals = swg.seg_mask_flat(flat, off)                      # the masked twin: the same offsets
    per_seq = np.array([_mask_counts(swg, s) for s in seqs], dtype=np.int64).reshape(N, 2)
    w = dict(sub=sub, queries=queries, pssms=amc.pssms(sub, queries), lens=lens, order=order, off=off, flat=(flat, mflat),
             mask_totals=totals, masked_residues=per_seq[:, 0], mask_segments=per_seq[:, 1])
    w["seqs"] = tuple([f[int(off[i]):int(off[i + 1])] for i in range(N)] for f in (flat, mflat))
    w["truth"] = tuple([orc.score_db(q, f, off, sub, *GAPS) for q in queries] for f in (flat, mflat))
    w["gapless"] = tuple([gc.gapless_numpy(q, f, off, sub=sub) for q in queries] for f in (flat, mflat))
    w["top"] = tuple([orc.topk(t, TOP) for t in truths] for truths in w["truth"])
    w["gapless_top"] = tuple([orc.topk(t, TOP) for t in truths] for truths in w["gapless"])
    w["levels"] = tuple([_levels(t) for t in truths] for truths in w["truth"])
    w["gapless_levels"] = tuple([_levels(t) for t in truths] for truths in w["gapless"])
    lrng = np.random.default_rng(SEED + 1)                            # the candidate lists: global, the same for every kind
    w["lists"] = [np.concatenate([[i for _, i in w["top"][0][qi]], lrng.choice(N, size=60, replace=False),
                                  [i for _, i in w["top"][0][qi][:5]]]).astype(np.int64) for qi in range(3)]
    w["elsewhere_shuffle"] = np.random.default_rng(SEED + 2).permutation(len(members_of_rank(w, 1, 3)))
    return w


def _mask_counts(swg, seq):
    mask, segments = swg.seg_mask(seq, want_segments=True)
    return int(mask.sum()), int(segments)


def _levels(truth):
    """The three thresholds of a query: above the best, the tenth best of the whole database, 1."""
    s = np.sort(truth)
    return (int(s[-1]) + 1, max(1, int(s[-10])), 1)


def members_of_rank(w, rank, count):
    """The original indices swg_db_pack(rank, count) keeps: bins b % count == rank of the global order."""
    order = w["order"]
    keep = [order[b * BIN:(b + 1) * BIN] for b in range(-(-N // BIN)) if b % count == rank]
    return np.sort(np.concatenate(keep)).astype(np.int64) if keep else np.zeros(0, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def trace(masked, qi, i):
    """The oracle's alignment of query qi with sequence i (of the masked twin or not) as align_stats' dict, with the path."""
    import swg_loader
    w, orc = world(), swg_loader.oracle()
    q, d = w["queries"][qi], w["seqs"][masked][i]
    score, (qb, qe, db_, de), ops = orc.pair_trace(q, d, w["sub"], *GAPS)
    a = {"score": score, "index": int(i), "q_begin": qb, "q_end": qe, "d_begin": db_, "d_end": de, "n_ops": len(ops)}
    a.update(zip(("n_ident", "n_match", "n_gap_open", "n_gap"), counts_of(q, d, qb, db_, ops)))
    a["ops"] = ops
    return a


@functools.lru_cache(maxsize=None)
def hsps(masked, qi, i, max_hsps):
    """The host twin's alignments of the pair, with counts and paths."""
    import swg_loader
    w, swg = world(), swg_loader.load()
    out = swg.align_hsps_host(w["sub"], GAPS[0], GAPS[1], w["seqs"][masked][i], max_hsps, MIN_HSP, query=w["queries"][qi], want_counts=True)
    for a in out:
        a["index"] = int(i)
    return out


# ---- kinds ------------------------------------------------------------------------------------------------------------
NOT_DIVISIBLE_BY_3 = np.array([i for i in range(N) if i % 3], dtype=np.int64)    # the list every rank of a run would pass


class Kind:
    """One way to make a swg_db.  base: (rank, count) of the packed shard everything starts from; elsewhere: packed with
    index= / n_total=; loaded: saved, loaded from the file; masked: swg_db_mask of that; view: swg_db_view of that."""

    def __init__(self, name, base, elsewhere=False, loaded=False, masked=False, view=False):
        self.name, self.base, self.elsewhere, self.loaded, self.masked, self.view = name, base, elsewhere, loaded, masked, view
        self.n_total = N_TOTAL_ELSEWHERE if elsewhere else N

    def base_members(self, w):
        return members_of_rank(w, *self.base)

    def members(self, w):
        m = self.base_members(w)
        return m[m % 3 != 0] if self.view else m

    def g(self, i):
        """World index -> this handle's index."""
        return elsewhere(i) if self.elsewhere else np.asarray(i, dtype=np.int64)

    def pack(self, swg, w, tmpdir):
        """The host half: the packed (or loaded) database, not resident."""
        flat, off = w["flat"][0], w["off"]
        if self.elsewhere:
            m = self.base_members(w)[w["elsewhere_shuffle"]]          # local position says nothing about the global index
            lflat, loff = pc.pack([w["seqs"][0][i] for i in m])
            db = swg.Database(lflat, loff, index=self.g(m), n_total=self.n_total)
        else:
            db = swg.Database(flat, off, *self.base)
        if self.loaded:
            path = os.path.join(str(tmpdir), self.name + ".swgdb")
            db.save(path)
            db.close()
            db = swg.Database(path=path)
        return db

    def open(self, swg, ctx, w, tmpdir):
        """-> (the handle, everything to close afterwards, the handle last)."""
        db = self.pack(swg, w, tmpdir).upload(ctx)
        chain = [db]
        if self.masked:
            chain.append(chain[-1].mask(ctx))
        if self.view:
            chain.append(chain[-1].view(ctx, self.g(NOT_DIVISIBLE_BY_3)))
        return chain[-1], chain

    def outside(self, w):
        """An index this handle does not hold (for the whole database there is none below total_count)."""
        rest = np.setdiff1d(np.arange(N), self.base_members(w))
        return int(self.g(rest[0])) if len(rest) else self.n_total + 5

    def unselected(self, w):
        """A view's: a valid index of its parent that it does not select; None for every other kind."""
        m = self.base_members(w)
        return int(self.g(m[m % 3 == 0][0])) if self.view else None


KINDS = {k.name: k for k in (
    Kind("whole", (0, 1)),
    Kind("rank0of3", (0, 3)), Kind("rank1of3", (1, 3)), Kind("rank2of3", (2, 3)),
    Kind("rank2of7", (2, 7)),                                         # one full bin
    Kind("rank5of7", (5, 7)),                                         # only the partial bin: 37 sequences, 91 empty slots
    Kind("rank6of7", (6, 7)),                                         # fewer bins than ranks: nothing
    Kind("cut_elsewhere", (1, 3), elsewhere=True),
    Kind("view_of_rank1of3", (1, 3), view=True),
    Kind("masked_rank1of3", (1, 3), masked=True),
    Kind("view_of_masked_rank1of3", (1, 3), masked=True, view=True),
    Kind("loaded_rank2of3", (2, 3), loaded=True),
)}


# ---- answers ----------------------------------------------------------------------------------------------------------
H = namedtuple("H", "score index")


class ByIndex:
    """An array whose last axis is indexed by database index, as the call left it: FILL32 where nothing was written."""

    def __init__(self, arr):
        self.arr = np.asarray(arr)

    @classmethod
    def of(cls, n_total, members, values, rows=None):
        a = np.full(n_total if rows is None else (rows, n_total), FILL32, dtype=np.int32)
        a[..., np.asarray(members, dtype=np.int64)] = values
        return cls(a)


class Pssm:
    """(pssm, values, info) of one query: compared by test_gpu_pssm_build._assert_same."""

    def __init__(self, pssm, values, info):
        self.t = (pssm, values, info)


def remap(a, kind):
    """An answer in the world's indices -> in the handle's."""
    if isinstance(a, ByIndex):
        written = np.nonzero((a.arr != FILL32).reshape(-1, a.arr.shape[-1]).any(axis=0))[0]
        return ByIndex.of(kind.n_total, kind.g(written), a.arr[..., written], rows=None if a.arr.ndim == 1 else a.arr.shape[0])
    if isinstance(a, H):
        return H(a.score, int(kind.g(a.index)))
    if isinstance(a, dict):
        return {k: (int(kind.g(v)) if k == "index" else remap(v, kind)) for k, v in a.items()}
    if isinstance(a, (list, tuple)):
        return type(a)(remap(x, kind) for x in a)
    return a


def same(got, want, where, assert_pssm):
    """Exact, entry for entry; the only tolerances are assert_pssm's (test_gpu_pssm_build._assert_same)."""
    if isinstance(want, ByIndex):
        assert isinstance(got, ByIndex) and got.arr.shape == want.arr.shape, where
        bad = np.nonzero(got.arr != want.arr)
        assert not len(bad[0]), (where, [b[:8].tolist() for b in bad], got.arr[bad][:8].tolist(), want.arr[bad][:8].tolist())
    elif isinstance(want, Pssm):
        assert_pssm(got.t, want.t, where)
    elif isinstance(want, np.ndarray):
        assert isinstance(got, np.ndarray) and got.dtype == want.dtype and np.array_equal(got, want), (where, got, want)
    elif isinstance(want, dict):
        assert isinstance(got, dict) and sorted(got) == sorted(want), (where, sorted(got), sorted(want))
        for k in want:
            same(got[k], want[k], "%s.%s" % (where, k), assert_pssm)
    elif isinstance(want, (list, tuple)) and not isinstance(want, H):
        assert isinstance(got, (list, tuple)) and len(got) == len(want), (where, got, want)
        for n, (g, x) in enumerate(zip(got, want)):
            same(g, x, "%s[%d]" % (where, n), assert_pssm)
    else:
        assert type(got) is type(want) and got == want, (where, got, want)


# ---- raw calls: every output pre-filled ------------------------------------------------------------------------------------
HIT = np.dtype([("score", "<i4"), ("index", "<u4")])
ALN = np.dtype([(f, "<i4" if f == "score" else "<u4") for f in ("score", "index", "q_begin", "q_end", "d_begin", "d_end", "n_ops", "reserved")])
CNT = np.dtype([(f, "<u4") for f in ("n_ident", "n_match", "n_gap_open", "n_gap")])


def refused_arg(swg):
    """What a refused call must answer: SWG_ERR_ARG, and nothing written."""
    return {"refused": swg.SWG_ERR_ARG, "untouched": True}


def _fresh(n, dtype):
    a = np.empty(max(int(n), 1), dtype=dtype)
    a.view(np.uint8)[...] = FILL
    return a


def _untouched(*arrays):
    return all(bool((a.view(np.uint8) == FILL).all()) for a in arrays if a is not None)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _hits_of(hits, n):
    return [H(int(s), int(i)) for s, i in zip(hits["score"][:n].tolist(), hits["index"][:n].tolist())]


class Env:
    """What a family runs with: the binding, the context, the world."""

    def __init__(self, swg, ctx):
        self.swg, self.ctx, self.w = swg, ctx, world()
        qs, ps = self.w["queries"], self.w["pssms"]
        self.qoff = np.zeros(4, dtype=np.uint64)
        self.qoff[1:] = np.cumsum([len(q) for q in qs])
        self.qflat = np.ascontiguousarray(np.concatenate(qs), dtype=np.int8)
        self.pflat = np.ascontiguousarray(np.concatenate(ps), dtype=np.int8)

    def packed(self, pssm):
        return self.pflat if pssm else self.qflat

    def set_query(self, qi, pssm=False):
        if pssm:
            self.ctx.set_query_pssm(self.w["pssms"][qi])
        else:
            self.ctx.set_query(self.w["queries"][qi])


def _search_raw(e, db, fn, k, want_scores=True):
    scores = _fresh(db.total_count, np.int32)[:db.total_count] if want_scores else None
    hits, nh, st = _fresh(k, HIT), C.c_size_t(0), e.swg.Stats()
    rc = fn(e.ctx.handle, db.handle, _p(scores), _p(hits) if k else None, k, C.byref(nh), C.byref(st))
    assert rc == e.swg.SWG_OK, e.swg.lib.swg_last_error(e.ctx.handle)
    out = {"hits": _hits_of(hits, nh.value), "tail": _untouched(hits[nh.value:])}
    if want_scores:
        out["scores"] = ByIndex(scores)
    return out, st.as_dict()


def _multi_raw(e, db, fn, pssm, k):
    scores = _fresh(3 * db.total_count, np.int32)[:3 * db.total_count].reshape(3, db.total_count)
    hits, nh, st = _fresh(3 * k, HIT), (C.c_size_t * 3)(), e.swg.Stats()
    rc = fn(e.ctx.handle, db.handle, _p(e.packed(pssm)), _p(e.qoff), 3, _p(scores), _p(hits), k, C.cast(nh, C.c_void_p), C.byref(st))
    assert rc == e.swg.SWG_OK, e.swg.lib.swg_last_error(e.ctx.handle)
    return {"scores": ByIndex(scores), "hits": [_hits_of(hits[i * k:], nh[i]) for i in range(3)],
            "tail": _untouched(*[hits[i * k + nh[i]:(i + 1) * k] for i in range(3)])}


def _above_raw(e, db, gapless, T, cap):
    """swg_search_above / swg_search_gapless_above of the context's query; cap 0: the pure count."""
    fn = e.swg.lib.swg_search_gapless_above if gapless else e.swg.lib.swg_search_above
    hits, nh, nt, st = _fresh(cap, HIT), C.c_size_t(0), C.c_uint64(0), e.swg.Stats()
    rc = fn(e.ctx.handle, db.handle, int(T), _p(hits) if cap else None, cap, C.byref(nh), C.byref(nt), C.byref(st))
    assert rc == e.swg.SWG_OK, e.swg.lib.swg_last_error(e.ctx.handle)
    return {"hits": _hits_of(hits, nh.value), "n_total": int(nt.value), "tail": _untouched(hits[nh.value:])}


def _lists_raw(e, db, pssm, lists, k):
    """swg_search_lists[_pssm]: the scores parallel to the lists and the hit rows, both pre-filled."""
    cand = np.ascontiguousarray(np.concatenate(lists), dtype=np.uint32)
    coff = np.zeros(4, dtype=np.uint64)
    coff[1:] = np.cumsum([len(l) for l in lists])
    scores, hits, nh, st = _fresh(len(cand), np.int32), _fresh(3 * k, HIT), (C.c_size_t * 3)(), e.swg.Stats()
    fn = e.swg.lib.swg_search_lists_pssm if pssm else e.swg.lib.swg_search_lists
    rc = fn(e.ctx.handle, db.handle, _p(e.packed(pssm)), _p(e.qoff), 3, _p(cand), _p(coff), _p(scores), _p(hits), k, C.cast(nh, C.c_void_p),
            C.byref(st))
    assert rc == e.swg.SWG_OK, e.swg.lib.swg_last_error(e.ctx.handle)
    return {"scores": [scores[int(coff[i]):int(coff[i + 1])].copy() for i in range(3)], "hits": [_hits_of(hits[i * k:], nh[i]) for i in range(3)],
            "tail": _untouched(*[hits[i * k + nh[i]:(i + 1) * k] for i in range(3)])}


def _above_multi_raw(e, db, fn, pssm, min_scores, cap):
    ms = np.ascontiguousarray(min_scores, dtype=np.int32)
    hits, nh, nt, st = _fresh(3 * cap, HIT), (C.c_size_t * 3)(), np.zeros(3, dtype=np.uint64), e.swg.Stats()
    rc = fn(e.ctx.handle, db.handle, _p(e.packed(pssm)), _p(e.qoff), 3, _p(ms), _p(hits), cap, C.cast(nh, C.c_void_p), _p(nt), C.byref(st))
    assert rc == e.swg.SWG_OK, e.swg.lib.swg_last_error(e.ctx.handle)
    return {"hits": [_hits_of(hits[i * cap:], nh[i]) for i in range(3)], "n_total": [int(v) for v in nt],
            "tail": _untouched(*[hits[i * cap + nh[i]:(i + 1) * cap] for i in range(3)])}


def _align_raw(e, db, name, rows, mode, pssm=False, max_hsps=0, min_score=MIN_HSP):
    """One swg_align_* call.  rows: None, [indices] (the single-query call `name`, on the context's query) or three rows
    (the batch call).  mode: "hits" (with paths), "bounds", "stats", "hsps" (counts and paths).  Every row has one slot
    more than its longest holds, so that there is always a slot the call must leave alone."""
    single = len(rows) == 1
    k = max(len(r) for r in rows) + 1
    per = max_hsps if mode == "hsps" else 1
    hin = np.zeros(len(rows) * k, dtype=HIT)
    nh = (C.c_size_t * len(rows))()
    for i, r in enumerate(rows):
        nh[i] = len(r)
        hin["index"][i * k:i * k + len(r)] = r
    slots = len(rows) * k
    out = _fresh(slots * per, ALN)
    cnt = _fresh(slots * per, CNT) if mode in ("stats", "hsps") else None
    nout = _fresh(slots, np.uint32) if mode == "hsps" else None
    lib, ctx = e.swg.lib, e.ctx.handle
    stride = int(lib.swg_align_ops_bound(ctx, db.handle) if single else lib.swg_align_ops_bound_multi(db.handle, _p(e.qoff), 3))
    ops = _fresh(slots * per * stride, np.uint8) if mode in ("hits", "hsps") else None
    head = (ctx, db.handle) + (() if single else (_p(e.packed(pssm)), _p(e.qoff), 3)) + ((_p(hin), len(rows[0])) if single else (_p(hin), k, C.cast(nh, C.c_void_p)))
    tail = {"hits": (_p(out), _p(ops), stride), "bounds": (_p(out),), "stats": (_p(out), _p(cnt)),
            "hsps": (max_hsps, min_score, _p(out), _p(nout), _p(cnt), _p(ops), stride)}[mode]
    rc = getattr(lib, name)(*head, *tail)
    if rc != e.swg.SWG_OK:
        return {"refused": rc, "untouched": _untouched(out, cnt, nout, ops)}

    def one(s):
        a = {f: int(out[s][f]) for f in ALN.names}
        if cnt is not None:
            a.update((f, int(cnt[s][f])) for f in CNT.names)
        if ops is not None:
            a["ops"] = ops[s * stride:s * stride + a["n_ops"]].tobytes().decode()
            assert ops[s * stride + a["n_ops"]] == 0                    # NUL-terminated
        return a

    res, left = [], []
    for i, r in enumerate(rows):
        for j in range(len(r), k):                                    # slots past n_hits[i]
            s = i * k + j
            left += [out[s * per:(s + 1) * per]] + ([cnt[s * per:(s + 1) * per]] if cnt is not None else []) + \
                    ([nout[s:s + 1]] if nout is not None else []) + ([ops[s * per * stride:(s + 1) * per * stride]] if ops is not None else [])
        if mode != "hsps":
            res.append([one(i * k + j) for j in range(len(r))])
            continue
        row = []
        for j in range(len(r)):
            s = i * k + j
            n = int(nout[s])
            row.append([one(s * per + x) for x in range(n)])
            left += [out[s * per + n:(s + 1) * per]] + [cnt[s * per + n:(s + 1) * per]] + [ops[(s * per + n) * stride:(s + 1) * per * stride]]
        res.append(row)
    return {"rows": res, "tail": _untouched(*left)}


def _pssm_build_raw(e, db, rows, pssm, single):
    """swg_pssm_build (the context's query: rows = [indices]) or swg_pssm_build_multi[_pssm] (three rows)."""
    lib, ctx = e.swg.lib, e.ctx.handle
    k = max(len(r) for r in rows) + 1
    hin = np.zeros(len(rows) * k, dtype=HIT)
    nh = (C.c_size_t * len(rows))()
    for i, r in enumerate(rows):
        nh[i] = len(r)
        hin["index"][i * k:i * k + len(r)] = r
    lq = e.ctx._lq if single else int(e.qoff[3])
    out, values = _fresh(lq * 32, np.int8), _fresh(lq * 32, np.float64)
    raw_info = _fresh(len(rows) * C.sizeof(e.swg.PssmInfo), np.uint8)
    info = (e.swg.PssmInfo * len(rows)).from_buffer(raw_info)
    tail = (None, float(e.swg.PSSM_PSEUDOCOUNT_DEFAULT), _p(out), _p(values), _p(raw_info))
    if single:
        residues = np.ascontiguousarray(e.w["queries"][single[0]], dtype=np.int8)
        rc = lib.swg_pssm_build(ctx, db.handle, _p(hin), len(rows[0]), _p(residues) if pssm else None, *tail)
    elif pssm:
        rc = lib.swg_pssm_build_multi_pssm(ctx, db.handle, _p(e.pflat), _p(e.qflat), _p(e.qoff), 3, _p(hin), k, C.cast(nh, C.c_void_p), *tail)
    else:
        rc = lib.swg_pssm_build_multi(ctx, db.handle, _p(e.qflat), _p(e.qoff), 3, _p(hin), k, C.cast(nh, C.c_void_p), *tail)
    if rc != e.swg.SWG_OK:
        return {"refused": rc, "untouched": _untouched(out, values, raw_info)}
    cut = [(0, lq)] if single else [(int(e.qoff[i]), int(e.qoff[i + 1])) for i in range(3)]
    return {"rows": [Pssm(out.reshape(-1, 32)[a:b].copy(), values.reshape(-1, 32)[a:b].copy(), info[i].as_dict()) for i, (a, b) in enumerate(cut)]}


# ---- what truth says about a kind -------------------------------------------------------------------------------------
def _top(truth, members, k):
    return [H(s, i) for s, i in amc.above(truth, 1 - (1 << 30), members)[:k]]


def _searched(w, kind, truths, k=K, scores=True, qis=(0, 1, 2)):
    m = kind.members(w)
    out = [dict(hits=_top(truths[qi], m, k), tail=True, **({"scores": ByIndex.of(N, m, truths[qi][m])} if scores else {})) for qi in qis]
    return out


def _batch(w, kind, truths, k=K):
    m = kind.members(w)
    return {"scores": ByIndex.of(N, m, np.stack([t[m] for t in truths]), rows=3), "hits": [_top(t, m, k) for t in truths], "tail": True}


def hit_rows(w, kind):
    """Per query the members among the truth's top list, best first (world indices)."""
    m = set(kind.members(w).tolist())
    return [[i for _, i in top if i in m] for top in w["top"][int(kind.masked)]]


def _rows_for(e, kind, bad, qi=None):
    rows = [list(kind.g(np.array(r, dtype=np.int64)).tolist()) for r in hit_rows(e.w, kind)]
    if qi is not None:
        rows = [rows[qi]]
    if bad is not None:
        rows[min(1, len(rows) - 1)].append(bad)
    return rows


def _aligned(w, kind, mode, max_hsps=0):
    keys = {"hits": ALN.names + ("ops",), "bounds": ALN.names, "stats": ALN.names + CNT.names, "hsps": ALN.names + CNT.names + ("ops",)}[mode]

    def one(a):
        return {k: a.get(k, 0) for k in keys}                        # (reserved = 0)

    mk = int(kind.masked)
    if mode == "hsps":
        return [[[one(a) for a in hsps(mk, qi, i, max_hsps)] for i in row] for qi, row in enumerate(hit_rows(w, kind))]
    return [[one(trace(mk, qi, i)) for i in row] for qi, row in enumerate(hit_rows(w, kind))]


def _pssms(w, kind):
    import swg_loader
    swg, orc = swg_loader.load(), swg_loader.oracle()
    mk = int(kind.masked)
    out = []
    for qi, row in enumerate(hit_rows(w, kind)):
        als = pc.align(orc, w["queries"][qi], w["flat"][mk], w["off"], row, w["sub"], GAPS)
        out.append(Pssm(*swg.pssm_from_paths(w["sub"], w["queries"][qi], w["flat"][mk], w["off"], als, want_values=True)))
    return out


# ---- families: run(e, kind, db, bad) -> answer in the handle's indices; expected(w, kind) -> answer in the world's ---------------
def _with_option(e, key, value, default, fn):
    e.ctx.set_option(key, value)
    try:
        return fn()
    finally:
        e.ctx.set_option(key, default)


def _flagged_are_rescored(e, kind, qi, st, what):
    """Where a search ran on the f16 cells alone (cell_form 2), what it ran again is exactly what reaches their ceiling."""
    flagged = int((e.w["truth"][int(kind.masked)][qi][kind.members(e.w)] >= f16_ceiling()).sum())
    assert st["cell_form"] != 2 or st["n_rescored"] == flagged, (kind.name, what, st, flagged)


def run_search(e, kind, db, bad=None):
    out = {}
    for f16 in (1, 0):
        rows = []
        for qi in range(3):
            e.set_query(qi)
            ans, st = _with_option(e, "f16", f16, 1, lambda: _search_raw(e, db, e.swg.lib.swg_search, K))
            _flagged_are_rescored(e, kind, qi, st, "f16=%d, query %d" % (f16, qi))
            if f16 == 1:                                              # the library's own choice of cells
                ans["rescored"] = st["n_rescored"] > 0
            rows.append(ans)
        out["f16=%d" % f16] = rows
    for prune in (0, 2):
        rows = []
        for qi in range(3):
            e.set_query(qi)
            rows.append(_with_option(e, "prune", prune, 1, lambda: _search_raw(e, db, e.swg.lib.swg_search, K, want_scores=False)[0]))
        out["hits only, prune=%d" % prune] = rows
    return out


def expect_search(w, kind):
    t = w["truth"][int(kind.masked)]
    out = {"f16=%d" % f: _searched(w, kind, t) for f in (1, 0)}
    for qi, ans in enumerate(out["f16=1"]):                           # a member at the f16 cells' ceiling is run again
        ans["rescored"] = bool((t[qi][kind.members(w)] >= f16_ceiling()).any())
    out.update({"hits only, prune=%d" % p: _searched(w, kind, t, scores=False) for p in (0, 2)})
    return out


def run_rescoring(e, kind, db, bad=None):
    """The 600-column query on the f16 cells of the lane groups: what reaches their ceiling is flagged and run again."""
    e.set_query(2)
    e.ctx.set_option("engine", 2)
    try:
        ans, st = _with_option(e, "f16", 2, 1, lambda: _search_raw(e, db, e.swg.lib.swg_search, K))
    finally:
        e.ctx.set_option("engine", 0)
    assert st["cell_form"] == (2 if db.count else 0), (kind.name, st)   # forced: the f16 cells alone (nothing to fill: no form)
    _flagged_are_rescored(e, kind, 2, st, "f16=2 on the lane groups")
    ans["rescored"] = st["n_rescored"] > 0
    return ans


def expect_rescoring(w, kind):
    t = w["truth"][int(kind.masked)]
    ans = _searched(w, kind, t, qis=(2,))[0]
    ans["rescored"] = bool((t[2][kind.members(w)] >= f16_ceiling()).any())
    return ans


def run_search_begin_end(e, kind, db, bad=None):
    out = []
    tickets = []
    for qi in (0, 1):                                                 # (an index query may change between two begins)
        e.set_query(qi)
        tickets.append(e.ctx.search_begin(db, k=K, want_scores=True)[0])
    for t in tickets:
        out.append(_search_raw(e, db, lambda c, d, s, h, k, nh, st: e.swg.lib.swg_search_end(c, t, s, h, nh, st), K)[0])
    return out


def expect_search_begin_end(w, kind):
    return _searched(w, kind, w["truth"][int(kind.masked)], qis=(0, 1))


def _run_multi(name, pssm):
    return lambda e, kind, db, bad=None: _multi_raw(e, db, getattr(e.swg.lib, name), pssm, K)


def _run_gapless(e, kind, db, bad=None):
    rows = []
    for qi in range(3):
        e.set_query(qi)
        rows.append(_search_raw(e, db, e.swg.lib.swg_search_gapless, K)[0])
    return rows


def _run_above(gapless):
    def run(e, kind, db, bad=None):
        levels = e.w["gapless_levels" if gapless else "levels"][int(kind.masked)]
        out = []
        for qi in range(3):
            e.set_query(qi)
            for T in levels[qi]:
                ans = _above_raw(e, db, gapless, T, max(db.count, 1) + 1)
                ans["count"] = _above_raw(e, db, gapless, T, 0)["n_total"]
                out.append(ans)
        return out
    return run


def _expect_above(gapless):
    def expect(w, kind):
        mk, m = int(kind.masked), kind.members(w)
        truths, levels = w["gapless" if gapless else "truth"][mk], w["gapless_levels" if gapless else "levels"][mk]
        out = []
        for qi in range(3):
            for T in levels[qi]:
                hits = [H(*h) for h in amc.above(truths[qi], T, m)]
                out.append({"hits": hits, "n_total": len(hits), "tail": True, "count": len(hits)})
        return out
    return expect


def _run_above_multi(name, pssm, gapless):
    def run(e, kind, db, bad=None):
        levels = e.w["gapless_levels" if gapless else "levels"][int(kind.masked)]
        return [_above_multi_raw(e, db, getattr(e.swg.lib, name), pssm, [levels[qi][l] for qi in range(3)], max(db.count, 1) + 1)
                for l in range(len(LEVELS))]
    return run


def _expect_above_multi(gapless):
    def expect(w, kind):
        mk, m = int(kind.masked), kind.members(w)
        truths, levels = w["gapless" if gapless else "truth"][mk], w["gapless_levels" if gapless else "levels"][mk]
        out = []
        for l in range(len(LEVELS)):
            hits = [[H(*h) for h in amc.above(truths[qi], levels[qi][l], m)] for qi in range(3)]
            out.append({"hits": hits, "n_total": [len(h) for h in hits], "tail": True})
        return out
    return expect


def _run_lists(pssm):
    def run(e, kind, db, bad=None):
        return _lists_raw(e, db, pssm, [kind.g(l) for l in e.w["lists"]], K)
    return run


def expect_lists(w, kind):
    t, m = w["truth"][int(kind.masked)], kind.members(w)
    held = [np.isin(l, m) for l in w["lists"]]
    return {"scores": [np.where(h, t[qi][l], FILL32).astype(np.int32) for qi, (l, h) in enumerate(zip(w["lists"], held))],
            "hits": [_top(t[qi], np.unique(l[h]), K) for qi, (l, h) in enumerate(zip(w["lists"], held))], "tail": True}


def run_composition(e, kind, db, bad=None):
    return {"counts": db.composition(e.ctx), "residues": int(db.residues)}


def expect_composition(w, kind):
    m = kind.members(w)
    seqs = [w["seqs"][int(kind.masked)][i] for i in m]
    counts = np.bincount(np.concatenate(seqs).astype(np.int64), minlength=32).astype(np.uint64) if seqs else np.zeros(32, dtype=np.uint64)
    return {"counts": counts, "residues": int(w["lens"][m].sum())}


def run_sequence(e, kind, db, bad=None):
    out = {"members": [db.sequence(int(i)) for i in kind.g(kind.members(e.w))]}
    for key, i in (("outside", kind.outside(e.w)), ("unselected", kind.unselected(e.w))):
        if i is None:
            out[key] = None
            continue
        try:
            db.sequence(i)
            out[key] = e.swg.SWG_OK
        except e.swg.SwgError as err:
            out[key] = err.code
    return out


def expect_sequence(w, kind):
    return {"members": [np.asarray(w["seqs"][int(kind.masked)][i], dtype=np.int8) for i in kind.members(w)], "outside": -1,
            "unselected": -1 if kind.view else None}


def _run_align(name, mode, pssm=False, single=False, max_hsps=0):
    def run(e, kind, db, bad=None):
        if not single:
            return _align_raw(e, db, name, _rows_for(e, kind, bad), mode, pssm, max_hsps)
        out = []
        for qi in range(3):
            e.set_query(qi, pssm)
            a = _align_raw(e, db, name, _rows_for(e, kind, bad if qi == 1 else None, qi), mode, pssm, max_hsps)
            if "refused" in a:
                return a
            out.append(a)
        return {"rows": [a["rows"][0] for a in out], "tail": all(a["tail"] for a in out)}
    return run


def _expect_align(mode, max_hsps=0):
    return lambda w, kind: {"rows": _aligned(w, kind, mode, max_hsps), "tail": True}


def run_hsps_of_one_equal_align_hits(e, kind, db, bad=None):
    """max_hsps 1 at min_score 1 against swg_align_hits, call against call."""
    rows = _rows_for(e, kind, bad)
    if bad is not None:
        return _align_raw(e, db, "swg_align_hsps_multi", rows, "hsps", max_hsps=1)
    one = _align_raw(e, db, "swg_align_hsps_multi", rows, "hsps", max_hsps=1, min_score=1)
    hits = _align_raw(e, db, "swg_align_hits_multi", rows, "hits")
    strip = lambda a: {k: v for k, v in a.items() if k not in CNT.names}
    return {"rows": [[[strip(a) for a in pair] for pair in row] for row in one["rows"]], "tail": one["tail"],
            "align_hits": [[[a] for a in row] for row in hits["rows"]]}


def expect_hsps_of_one(w, kind):
    rows = [[[a] for a in row] for row in _aligned(w, kind, "hits")]
    return {"rows": rows, "tail": True, "align_hits": rows}


def _run_pssm_build(pssm, single):
    def run(e, kind, db, bad=None):
        if not single:
            return _pssm_build_raw(e, db, _rows_for(e, kind, bad), pssm, None)
        out = []
        for qi in range(3):
            e.set_query(qi, pssm)
            a = _pssm_build_raw(e, db, _rows_for(e, kind, bad if qi == 1 else None, qi), pssm, (qi,))
            if "refused" in a:
                return a
            out += a["rows"]
        return {"rows": out}
    return run


def expect_pssm_build(w, kind):
    return {"rows": _pssms(w, kind)}


Family = namedtuple("Family", "name run expected takes_hits")
_T = lambda w, kind: w["truth"][int(kind.masked)]
_G = lambda w, kind: w["gapless"][int(kind.masked)]
FAMILIES = [
    Family("search", run_search, expect_search, False),
    Family("search rescoring", run_rescoring, expect_rescoring, False),
    Family("search_begin / search_end", run_search_begin_end, expect_search_begin_end, False),
    Family("search_multi", _run_multi("swg_search_multi", False), lambda w, k: _batch(w, k, _T(w, k)), False),
    Family("search_multi_pssm", _run_multi("swg_search_multi_pssm", True), lambda w, k: _batch(w, k, _T(w, k)), False),
    Family("search_gapless", _run_gapless, lambda w, k: _searched(w, k, _G(w, k)), False),
    Family("search_gapless_multi", _run_multi("swg_search_gapless_multi", False), lambda w, k: _batch(w, k, _G(w, k)), False),
    Family("search_gapless_multi_pssm", _run_multi("swg_search_gapless_multi_pssm", True), lambda w, k: _batch(w, k, _G(w, k)), False),
    Family("search_above", _run_above(False), _expect_above(False), False),
    Family("search_gapless_above", _run_above(True), _expect_above(True), False),
    Family("search_above_multi", _run_above_multi("swg_search_above_multi", False, False), _expect_above_multi(False), False),
    Family("search_above_multi_pssm", _run_above_multi("swg_search_above_multi_pssm", True, False), _expect_above_multi(False), False),
    Family("search_gapless_above_multi", _run_above_multi("swg_search_gapless_above_multi", False, True), _expect_above_multi(True), False),
    Family("search_gapless_above_multi_pssm", _run_above_multi("swg_search_gapless_above_multi_pssm", True, True), _expect_above_multi(True), False),
    Family("search_lists", _run_lists(False), expect_lists, False),
    Family("search_lists_pssm", _run_lists(True), expect_lists, False),
    Family("composition", run_composition, expect_composition, False),
    Family("sequence", run_sequence, expect_sequence, False),
    Family("align_hits", _run_align("swg_align_hits", "hits", single=True), _expect_align("hits"), True),
    Family("align_hits, PSSM query", _run_align("swg_align_hits", "hits", pssm=True, single=True), _expect_align("hits"), True),
    Family("align_hits_multi", _run_align("swg_align_hits_multi", "hits"), _expect_align("hits"), True),
    Family("align_hits_multi_pssm", _run_align("swg_align_hits_multi_pssm", "hits", pssm=True), _expect_align("hits"), True),
    Family("align_bounds", _run_align("swg_align_bounds", "bounds", single=True), _expect_align("bounds"), True),
    Family("align_bounds, PSSM query", _run_align("swg_align_bounds", "bounds", pssm=True, single=True), _expect_align("bounds"), True),
    Family("align_bounds_multi", _run_align("swg_align_bounds_multi", "bounds"), _expect_align("bounds"), True),
    Family("align_bounds_multi_pssm", _run_align("swg_align_bounds_multi_pssm", "bounds", pssm=True), _expect_align("bounds"), True),
    Family("align_stats", _run_align("swg_align_stats", "stats", single=True), _expect_align("stats"), True),
    Family("align_stats, PSSM query", _run_align("swg_align_stats", "stats", pssm=True, single=True), _expect_align("stats"), True),
    Family("align_stats_multi", _run_align("swg_align_stats_multi", "stats"), _expect_align("stats"), True),
    Family("align_stats_multi_pssm", _run_align("swg_align_stats_multi_pssm", "stats", pssm=True), _expect_align("stats"), True),
    Family("align_hsps, max_hsps 1", run_hsps_of_one_equal_align_hits, expect_hsps_of_one, True),
    Family("align_hsps", _run_align("swg_align_hsps", "hsps", single=True, max_hsps=3), _expect_align("hsps", 3), True),
    Family("align_hsps, PSSM query", _run_align("swg_align_hsps", "hsps", pssm=True, single=True, max_hsps=3), _expect_align("hsps", 3), True),
    Family("align_hsps_multi", _run_align("swg_align_hsps_multi", "hsps", max_hsps=3), _expect_align("hsps", 3), True),
    Family("align_hsps_multi_pssm", _run_align("swg_align_hsps_multi_pssm", "hsps", pssm=True, max_hsps=3), _expect_align("hsps", 3), True),
    Family("pssm_build", _run_pssm_build(False, True), expect_pssm_build, True),
    Family("pssm_build, PSSM query", _run_pssm_build(True, True), expect_pssm_build, True),
    Family("pssm_build_multi", _run_pssm_build(False, False), expect_pssm_build, True),
    Family("pssm_build_multi_pssm", _run_pssm_build(True, False), expect_pssm_build, True),
]
# what test_ranks_merge_to_the_whole merges: every family whose answer is a search result or a sum over the shard, that is
# every row that takes no hits, but `sequence` (a read-back of single sequences: nothing to merge)
MERGED = tuple(f.name for f in FAMILIES if not f.takes_hits and f.name != "sequence")


def expected(family, kind):
    """The family's answer on a handle of this kind, in the handle's indices."""
    return remap(family.expected(world(), kind), kind)
