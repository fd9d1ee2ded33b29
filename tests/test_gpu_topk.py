"""GPU (-m gpu): the device top-K selection (swg_topk_hist_kernel -> swg_topk_threshold_kernel -> swg_topk_compact_kernel,
the host's sort of the candidates and its fall-back to every score) at its histogram and capacity edges, on databases
whose scores are planted (tests/topk_cases.py; tests/test_topk_cases_host.py proves them against the oracle).

The rule: every case asserts hits == oracle.topk(planted scores, k) exactly -- score descending, original index
ascending -- for a search that asks for hits only (want_scores = False), on both sides of every edge; which route ran
is not asked, equality on both sides is the assertion."""
import numpy as np
import pytest

import topk_cases as tc
from test_gpu_parity import _reset_options

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _planted_scoring(ctx):
    _reset_options(ctx)
    ctx.set_option("autotune", 0)
    ctx.set_scoring(tc.table(), *tc.GAPS)
    ctx.set_query(tc.query())
    yield
    _reset_options(ctx)
    ctx.set_option("autotune", 1)               # (the two options _reset_options leaves alone)
    ctx.set_option("side_readout", 1)


@pytest.fixture(scope="module")
def ties():
    return {n_tie: tc.ties_case(n_tie) for n_tie in (8092, 8093)}


def _hits_only(ctx, orc, db, case, k):
    none, hits, _ = ctx.search(db, want_scores=False, k=k)
    assert none is None
    assert len(hits) == min(k, case["n"])
    assert hits == orc.topk(case["scores"], k), k
    return hits


def _with_scores(ctx, db, case, k, hits):
    scores, hits2, _ = ctx.search(db, want_scores=True, k=k)
    assert np.array_equal(scores, case["scores"]) and hits2 == hits, k


@pytest.mark.parametrize("T", tc.THRESHOLDS)
def test_kth_best_at_a_named_bin(swg, ctx, orc, T):
    """The K-th best score at 4094 (the last bin the device selects on), at 4095 and 4096 (the shared last bin: the
    host selects; from 4096 the pair is flagged by the f16 cells and re-run first), either side of a boundary between
    two threads of the threshold kernel (15 | 16, 17; 4079 | 4080) and at 0 (k beyond the non-zero scores): the k-th
    hit cuts a tie of four, scores up to 4199 lie above it, some in the bins of the same thread.  Also k = 1, a k that
    takes exactly the scores beyond one thread's bins, and k = n - 1, n, n + 1, where the number of hits stops at n
    (the last bin's padding slots are nobody's hit)."""
    case = tc.threshold_case(T)
    db = swg.Database(case["flat"], case["offsets"]).upload(ctx)
    for k in case["ks"]:
        hits = _hits_only(ctx, orc, db, case, k)
        if k == case["k"]:
            assert hits[-1][0] == T
            _with_scores(ctx, db, case, k, hits)
    db.close()


@pytest.mark.parametrize("n_tie", [8092, 8093])
def test_ties_against_the_candidate_capacity(swg, ctx, orc, ties, n_tie):
    """100 scores above T, then a tie of 8092 at T: with k in 101 .. 4096 exactly the 8192 candidates the device keeps;
    a tie of 8093: one more, and the host selects.  The tie's members have varied lengths and shuffled indices: the
    k - 100 lowest original indices are reported, on both sides of the capacity.  k = 4095, 4096 | 4097, 8193: the
    device selects up to half the capacity, the host beyond; k = n - 1, n, n + 1: the hits stop at n."""
    case = ties[n_tie]
    db = swg.Database(case["flat"], case["offsets"]).upload(ctx)
    for k in tc.TIES_KS + tc.TIES_KS_HALF_CAP + tc.TIES_KS_COUNT:
        hits = _hits_only(ctx, orc, db, case, k)
        if k in (150, 4097):
            _with_scores(ctx, db, case, k, hits)
    assert [h[0] for h in orc.topk(case["scores"], 150)[100:]] == [tc.TIES_T] * 50
    db.close()


def test_more_slots_than_one_sweep_of_the_histogram(swg, ctx, orc):
    """150 000 sequences, the 50 best scores the 50 shortest ones, at the last sorted slots, and padding slots in the
    last bin: candidates, their keys and the padding test beyond slot 131 072, where the histogram's grid of 512 x 256
    threads has begun to stride.  (The stride itself cannot show in a hit list: a histogram of fewer slots only lowers
    the threshold, the compaction reads every slot, and the host counts the candidates.)"""
    case = tc.sweep_case()
    db = swg.Database(case["flat"], case["offsets"]).upload(ctx)
    for k in tc.SWEEP_KS:
        hits = _hits_only(ctx, orc, db, case, k)
    _with_scores(ctx, db, case, tc.SWEEP_KS[-1], hits)
    db.close()


def test_nothing_but_ties(swg, ctx, orc):
    """9000 empty records and 10 one-residue sequences, every score 0: the tie overflows the candidate list and the
    order is by original index alone."""
    case = tc.all_ties_case()
    db = swg.Database(case["flat"], case["offsets"]).upload(ctx)
    for k in tc.ALL_TIES_KS:
        assert _hits_only(ctx, orc, db, case, k) == [(0, i) for i in range(k)]
    db.close()


def test_state_between_searches_on_one_resident_database(swg, ctx, orc, ties):
    """A search the host has to select for, then one the device selects, then scores only, then the device again, on
    one context and database: no status, count or histogram of a search is seen by the next."""
    case = ties[8093]
    db = swg.Database(case["flat"], case["offsets"]).upload(ctx)
    for _ in range(2):
        _hits_only(ctx, orc, db, case, 150)
        _hits_only(ctx, orc, db, case, 50)
        scores, hits, _ = ctx.search(db, want_scores=True, k=0)
        assert np.array_equal(scores, case["scores"]) and hits == []
        _hits_only(ctx, orc, db, case, 3)
    db.close()


@pytest.mark.parametrize("side_readout", [1, 0])
def test_state_between_searches_in_flight(swg, ctx, orc, ties, side_readout):
    """Four searches in flight on one database -- the host's selection, the device's and score arrays mixed --,
    redeemed out of order, twice, so that every slot's buffers serve a search of another kind the second time; with
    the read-out on its own stream and on the main one."""
    case = ties[8093]
    ctx.set_option("side_readout", side_readout)
    db = swg.Database(case["flat"], case["offsets"]).upload(ctx)
    _hits_only(ctx, orc, db, case, 7)                            # (the read-out stream exists from the second search on)
    for asks in (((150, False), (50, False), (0, True), (4096, False)),
                 ((3, False), (101, False), (20, True), (100, False)),
                 ((0, True), (4096, False), (1, False), (150, False))):
        tickets = [ctx.search_begin(db, k=k, want_scores=ws) for k, ws in asks]
        for t in (2, 0, 3, 1):
            k, ws = asks[t]
            scores, hits, _ = ctx.search_end(tickets[t])
            assert hits == orc.topk(case["scores"], k), (asks, t)
            assert np.array_equal(scores, case["scores"]) if ws else scores is None
    db.close()


@pytest.mark.parametrize("k", [7, 150, 4096])
def test_tie_across_shards(swg, ctx, orc, ties, k):
    """The ties database cut into three shards: each shard's keys merged by swg_topk_merge_keys, and a group of three
    contexts on one device (no collective), equal the whole database's top-K -- the tie spans the shards and breaks by
    GLOBAL original index; k = 4096 exceeds the smallest shard's count."""
    case = ties[8093]
    want = orc.topk(case["scores"], k)
    keys = []
    for r in range(3):
        db = swg.Database(case["flat"], case["offsets"], shard_rank=r, shard_count=3).upload(ctx)
        assert db.total_count == case["n"] and 0 < db.count < 4096
        keys.append(ctx.search_keys(db, k)[0])
        db.close()
    assert swg.topk_merge_keys(np.concatenate(keys), k) == want
    grp = swg.Group([0, 0, 0])
    grp.set_option("autotune", 0)
    grp.set_scoring(tc.table(), *tc.GAPS)
    grp.set_query(tc.query())
    grp.load(case["flat"], case["offsets"])
    none, hits, _ = grp.search(want_scores=False, k=k)
    assert none is None and hits == want
    grp.close()


# ---- query batches: capacity 1024 per query, the device selects for k <= 512 ----------------------------------------
def _batch(ctx, orc, db, case, queries, k, forms, pssm):
    if pssm:
        none, hits, st = ctx.search_multi_pssm(db, [tc.pssm(a, c) for a, c in queries], k=k, want_scores=False)
    else:
        none, hits, st = ctx.search_multi(db, [tc.query(a, c) for a, c in queries], k=k, want_scores=False)
    assert none is None and len(hits) == len(queries)
    if len(queries) > 1:        # the batch went through its own launches (swg_launch_topk_multi), not one query after another
        assert st["fill_launches"] == 1 and st["engine"] == 2 and st["cell_form"] in forms, st
    else:                       # a batch of one is a single search (swg_launch_topk, 8192 candidates): it reports no batch launch
        assert st["fill_launches"] == 0, st
    for r, (a, c) in enumerate(queries):
        assert hits[r] == orc.topk(tc.analytic(case["i"], case["j"], a, c), k), (queries, r, k, pssm)


@pytest.mark.parametrize("opts,forms", [({}, (3, 2)), ({"qq": 0}, (2,)), ({"f16": 0}, (0,))])
def test_batch_rows_take_different_routes(swg, ctx, orc, opts, forms):
    """Four queries against 20 001 short sequences (the batch's histogram grid of 64 x 256 threads strides): for every
    k up to 512 query 0 has exactly the 1024 candidates a row holds, query 1 has 1025 (that row alone goes to the
    host), query 2's k-th best score is 4095 for k <= 110 (the shared last bin: the host), query 3 is ordinary.  Every
    row gets its own list in every order of the rows, so no row's histogram, status, count or candidates reach
    another's; k = 513 is the host's for all; a batch of three; a batch of one, which the library searches as a single
    search (so its row has the single search's capacity); the three cell forms; and the same batch as position-specific
    queries."""
    case = tc.batch_case()
    ctx.set_option("engine", 2)             # (lane groups: short sequences would otherwise go one query after another)
    for key, v in opts.items():
        ctx.set_option(key, v)
    db = swg.Database(case["flat"], case["offsets"]).upload(ctx)
    q = tc.BATCH_QUERIES
    for queries in (q, (q[2], q[1], q[3], q[0]), q[:3], q[1:2]):
        for k in tc.BATCH_KS:
            for pssm in (False, True):
                _batch(ctx, orc, db, case, queries, k, forms, pssm)
    scores, hits, _ = ctx.search_multi(db, [tc.query(a, c) for a, c in q], k=tc.BATCH_K)
    for r, (a, c) in enumerate(q):
        want = tc.analytic(case["i"], case["j"], a, c)
        assert np.array_equal(scores[r], want) and hits[r] == orc.topk(want, tc.BATCH_K)
    db.close()


def test_batch_chunks_share_the_rows_of_the_buffers(swg, ctx, orc):
    """300 queries are searched as chunks of 256 and 44 through the same histogram, status, count and candidate rows:
    the second chunk's rows start from nothing."""
    case = tc.chunk_case()
    ctx.set_option("engine", 2)
    db = swg.Database(case["flat"], case["offsets"]).upload(ctx)
    for pssm in (False, True):
        _batch(ctx, orc, db, case, tc.chunk_queries(), tc.CHUNK_K, (3, 2), pssm)
    db.close()
