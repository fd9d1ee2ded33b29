"""CPU: the databases of tests/topk_cases.py are what they claim to be.  For every case the GPU tests use, the analytic
scores equal the oracle's, and the case has the property it is named for -- a K-th best score at the named histogram
bin, a tie of exactly the candidate capacity or one more, more slots than one sweep of the histogram's grid."""
import numpy as np
import pytest

import topk_cases as tc


def _oracle_agrees(orc, case, a=41, c=99, gaps=tc.GAPS):
    want = orc.score_db(tc.query(a, c), case["flat"], case["offsets"], tc.table(), *gaps)
    assert np.array_equal(want, tc.analytic(case["i"], case["j"], a, c))


@pytest.mark.parametrize("gaps", [(-11, -1), (-2, -1), (0, -1)])
def test_formula_for_every_planted_score(orc, gaps):
    """Every (i, j) up to a sequence longer than the query in both runs, with and without flanks, three gap settings and
    three queries: the score is 100 min(i, a) + min(j, c)."""
    i, j = (v.ravel() for v in np.meshgrid(np.arange(0, 45, 4), np.arange(0, 104, 5), indexing="ij"))
    rng = np.random.default_rng(1)
    case = tc._case(np.tile(i, 2), np.tile(j, 2), np.concatenate([0 * i, rng.integers(0, 9, size=len(i))]),
                    np.concatenate([0 * i, rng.integers(0, 9, size=len(i))]), rng)
    for a, c in ((41, 99), (40, 95), (2, 20)):
        _oracle_agrees(orc, case, a, c, gaps)


@pytest.mark.parametrize("T", tc.THRESHOLDS)
def test_threshold_cases(orc, T):
    case = tc.threshold_case(T)
    _oracle_agrees(orc, case)
    kth, count = tc.kth_and_count(case["scores"], case["k"])
    assert kth == T and count > case["k"]                      # the K-th best is T, and the tie at T is cut
    assert int((case["scores"] > T).sum()) == case["k"] - 2
    assert case["scores"].max() == 4199 and case["n"] % tc.BIN != 0
    bins, bin_T = np.minimum(case["scores"], tc.LAST_BIN), min(T, tc.LAST_BIN)
    if bin_T % 16 != 15:                                       # scores above T in bins of the same thread of 16
        assert int(((case["scores"] > T) & (bins // 16 == bin_T // 16)).sum()) >= 6
    # (low thresholds) one k selects exactly the scores beyond a thread's 16 bins: its `above` equals k
    assert T > 4000 or any(int((case["scores"] >= 16 * t).sum()) in case["ks"] for t in range(1, 256))
    assert tc.THRESHOLDS == (4094, 4095, 4096, 15, 16, 17, 4079, 4080, 0)


@pytest.mark.parametrize("n_tie,candidates", [(8092, tc.CAND_CAP), (8093, tc.CAND_CAP + 1)])
def test_ties_cases(orc, n_tie, candidates):
    case = tc.ties_case(n_tie)
    _oracle_agrees(orc, case)
    assert case["n"] == tc.TIES_N and case["n"] % tc.BIN != 0
    assert int((case["scores"] > tc.TIES_T).sum()) == 100 and int((case["scores"] == tc.TIES_T).sum()) == n_tie
    for k in (101, 150, 4096):
        assert tc.kth_and_count(case["scores"], k) == (tc.TIES_T, candidates)
    assert tc.kth_and_count(case["scores"], 100) == (tc.TIES_T + 1, 100)
    # the tie's members in sorted order are not in index order: a key built from the slot reports other members
    order = tc.sorted_order(case["offsets"])
    tie_by_rank = order[case["scores"][order] == tc.TIES_T]
    assert not np.array_equal(tie_by_rank[:50], np.sort(tie_by_rank)[:50])
    # three shards (bins b % 3): the tie spans all of them, and the smallest holds fewer than 4096 sequences
    shard_of_rank = (np.arange(case["n"]) // tc.BIN) % 3
    assert all((case["scores"][order[shard_of_rank == r]] == tc.TIES_T).sum() > 2000 for r in range(3))
    assert min(int((shard_of_rank == r).sum()) for r in range(3)) < 4096


def test_sweep_case(orc):
    case = tc.sweep_case()
    _oracle_agrees(orc, case)
    n = case["n"]
    assert n == tc.SWEEP_N and n % tc.BIN != 0 and tc.n_slots(n) > tc.HIST_SWEEP
    rank = np.empty(n, dtype=np.int64)
    rank[tc.sorted_order(case["offsets"])] = np.arange(n)
    best = np.argsort(-case["scores"], kind="stable")[:50]
    assert case["scores"][best].min() == 100 and int((case["scores"] >= 100).sum()) == 50
    assert rank[best].min() >= n - 50 >= tc.HIST_SWEEP         # the 50 best hold the 50 last sorted ranks
    assert tc.kth_and_count(case["scores"], 4096)[1] <= tc.CAND_CAP


def test_all_ties_case(orc):
    case = tc.all_ties_case()
    _oracle_agrees(orc, case)
    lens = np.diff(case["offsets"].astype(np.int64))
    assert case["n"] == 9010 > tc.CAND_CAP and not case["scores"].any()
    assert int((lens == 0).sum()) == 9000 and int((lens == 1).sum()) == 10


def test_batch_case(orc):
    case = tc.batch_case()
    for a, c in tc.BATCH_QUERIES:
        _oracle_agrees(orc, case, a, c)
    assert tc.n_slots(case["n"]) > tc.MULTI_SWEEP and case["n"] % tc.BIN != 0
    sc = [tc.analytic(case["i"], case["j"], a, c) for a, c in tc.BATCH_QUERIES]
    for k in (1, tc.BATCH_K, 512):
        assert tc.kth_and_count(sc[0], k) == (220, tc.MULTI_CAP)
        assert tc.kth_and_count(sc[1], k) == (310, tc.MULTI_CAP + 1)
    assert tc.kth_and_count(sc[2], tc.BATCH_K) == (tc.LAST_BIN, tc.BATCH_LONG)
    assert sc[2].max() == tc.LAST_BIN                          # no query of the batch can reach the f16 cells' 4096
    T3, n3 = tc.kth_and_count(sc[3], tc.BATCH_K)
    assert T3 < tc.LAST_BIN and tc.BATCH_K < n3 <= tc.MULTI_CAP
    assert tc.BATCH_KS == (1, 100, 512, 513)


def test_chunk_case(orc):
    case = tc.chunk_case()
    qs = tc.chunk_queries()
    assert len(qs) == tc.CHUNK_QUERIES > 256
    for a, c in qs[:6] + qs[-3:]:
        _oracle_agrees(orc, case, a, c)
    counts = [tc.kth_and_count(tc.analytic(case["i"], case["j"], a, c), tc.CHUNK_K)[1] for a, c in qs]
    # rows r and 256 + r share a row of the buffers: both chunks' candidates together would still fit it
    assert all(counts[r] + counts[256 + r] <= tc.MULTI_CAP for r in range(tc.CHUNK_QUERIES - 256))
    assert min(counts) >= tc.CHUNK_K
