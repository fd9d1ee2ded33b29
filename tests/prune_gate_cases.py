"""The gate in front of the first pruning level (option prune_gate): the databases, the cases and the
mirror rule the host and GPU tests share.

A gated search leaves in the pair bounds: 0xFFFFFFFF for the pairs of the first, unpruned stage (the K-th best route
only); max(U_1x, U_1y) -- the colmax sum of swg_debug_prune_bound -- where that is below the T of the stage that queues the
first level; elsewhere what the ungated search leaves."""
import numpy as np

GO, GE = -2, -1
LQ = 300
COPY = 150            # residues of the query the best sequences of the first stage hold: T lands near 800
NOT_BOUNDED = 0xFFFFFFFF
EDGE_BLOCKS = (4, 5, 6, 9, 10, 11, 31, 32, 33, 40, 41, 160, 161)   # the k = 5 unit, its tail, a chunk of 8 and of 32 units

OFF = {"prune_refine": 1, "prune_refine3": 1, "prune_refine4": 1}
# label -> (database, query kind, options, route: ("topk", k) | ("above", "inside" | "over"))
CASES = {
    "s32": ("main", "index", dict(OFF, prune_kmer=4, prune_segments=32), ("topk", 10)),
    "s16": ("main", "index", dict(OFF, prune_kmer=4, prune_segments=16), ("topk", 10)),
    "s8": ("main", "index", dict(OFF, prune_kmer=4, prune_segments=8), ("topk", 10)),
    "s20_of_32_lanes": ("main", "index", dict(OFF, prune_kmer=4, prune_segments=20), ("topk", 10)),
    "k5_s8": ("main", "index", dict(OFF, prune_kmer=5, prune_segments=8), ("topk", 10)),
    "k5_s8_short_partner": ("long_short", "index", dict(OFF, prune_kmer=5, prune_segments=8), ("topk", 10)),
    "s32_short_partner": ("long_short", "index", dict(OFF, prune_kmer=4, prune_segments=32), ("topk", 10)),
    "bits16": ("main", "index", dict(OFF, prune_kmer=4, prune_segments=32, prune_table_bits=16), ("topk", 10)),
    "pssm": ("main", "pssm", dict(OFF, prune_kmer=4, prune_segments=32), ("topk", 10)),
    "view": ("view", "index", dict(OFF, prune_kmer=4, prune_segments=32), ("topk", 10)),
    "shard": ("shard", "index", dict(OFF, prune_kmer=4, prune_segments=32), ("topk", 10)),
    "k_at_least_n": ("small", "index", dict(OFF, prune_kmer=4, prune_segments=32), ("topk", 400)),
    "head_and_rest": ("main", "index", dict(OFF, prune_kmer=4, prune_segments=32, segment_blocks=0), ("topk", 10)),
    "above_inside": ("main", "index", dict(OFF, prune_kmer=4, prune_segments=32), ("above", "inside")),
    "above_over_every_bound": ("main", "index", dict(OFF, prune_kmer=4, prune_segments=32), ("above", "over")),
    "levels_topk": ("main", "index", dict(prune_kmer=4, prune_segments=32, prune_refine=128, prune_refine3=256, prune_refine4=5256), ("topk", 10)),
    "levels_above": ("main", "index", dict(prune_kmer=4, prune_segments=32, prune_refine=128, prune_refine3=256, prune_refine4=5256),
                     ("above", "inside")),
}


def _packed(rng, seqs):
    seqs = [seqs[i] for i in rng.permutation(len(seqs))]
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return np.concatenate(seqs).astype(np.int8), off


def make_data(swg):
    """main: 60 sequences of 900..1000 residues (the first stage), fourteen of them around COPY residues of the query, so
    that the tenth best score stands near 800; six each of the lengths whose pairs have EDGE_BLOCKS token blocks, with B, Z,
    X and the indices behind Z in some; 2400 of 1..420 residues, so that T falls inside the range: the short ones have
    U_1 < T, the longer ones reach it and are walked.  long_short: the 60, then 1201 of 200..260, 602 of 60..80 and 799 of
    1..4 residues -- an odd count each, so one pair is a sequence of 200 or more beside one of at most 80 and one a
    sequence of 60 or more beside one of at most 4.  small: 200 sequences of 20..300 residues, fewer than the K asked for."""
    rng = np.random.default_rng(0x5EED0F01)
    q = swg.synth_query(0x5EED0F02, LQ)
    longs = [rng.integers(1, 21, size=int(n)).astype(np.int8) for n in rng.integers(900, 1001, size=60)]
    for i in range(14):
        at = int(rng.integers(0, LQ - COPY))
        to = int(rng.integers(0, len(longs[4 * i]) - COPY))
        longs[4 * i][to:to + COPY] = q[at:at + COPY]
    odd = np.array([2, 26, 24, 27, 28, 29, 30], dtype=np.int8)
    edges = []
    for nb in EDGE_BLOCKS:
        n = 4 * nb - 3
        for j in range(6):
            s = rng.integers(1, 21, size=n).astype(np.int8)
            if j in (1, 3, 5):
                at = rng.choice(n, size=max(1, n // 9), replace=False)
                s[at] = rng.choice(odd, size=len(at))
            edges.append(s)
    body = [rng.integers(1, 21, size=int(n)).astype(np.int8) for n in rng.integers(1, 421, size=2400)]
    main = _packed(rng, longs + edges + body)
    mid = [rng.integers(1, 21, size=int(n)).astype(np.int8) for n in rng.integers(200, 261, size=1201)]
    low = [rng.integers(1, 21, size=int(n)).astype(np.int8) for n in rng.integers(60, 81, size=602)]
    tiny = [rng.integers(1, 31, size=int(n)).astype(np.int8) for n in rng.integers(1, 5, size=799)]
    long_short = _packed(rng, longs + mid + low + tiny)
    small = _packed(rng, [rng.integers(1, 21, size=int(n)).astype(np.int8) for n in rng.integers(20, 301, size=200)])
    return {"q": q, "main": main, "long_short": long_short, "small": small, "cache": {}}


def pair_sequences(order, flat, off):
    """The pairs of the token order as sequences for the mirrors: x, then y filled up to x's length with padding rows
    (a pair without a partner: y is padding alone)."""
    o = off.astype(np.int64)
    parts, lens = [], []
    for x, y in zip(order[0::2], order[1::2]):
        sx = flat[o[x]:o[x + 1]]
        sy = flat[o[y]:o[y + 1]] if y != NOT_BOUNDED else flat[:0]
        assert x != NOT_BOUNDED and len(sx) >= len(sy)
        parts += [sx, sy, np.zeros(len(sx) - len(sy), dtype=np.int8)]
        lens += [len(sx), len(sx)]
    poff = np.zeros(len(lens) + 1, dtype=np.uint64)
    poff[1:] = np.cumsum(lens)
    return np.concatenate(parts).astype(np.int8), poff


def expected_bounds(ungated, u1, stages, fixed):
    """The mirror rule.  ungated: the bounds the same search leaves with prune_gate = 1; u1: max(U_1x, U_1y) per pair;
    stages: the gated search's cut stages (begin, end, T, list) -- the first is the one that queues the first level."""
    want = np.asarray(ungated, dtype=np.int64).copy()
    if not stages:
        return want   # (one uncut stage: nothing waits for a threshold, every pair is bounded ungated)
    begin, T = stages[0][0], stages[0][2]
    if fixed:
        assert begin == 0
    else:
        want[:begin] = NOT_BOUNDED
    left = np.flatnonzero(u1[begin:] < T) + begin
    want[left] = u1[left]
    assert np.all(want[left] >= np.asarray(ungated, dtype=np.int64)[left])   # (every level's bound is at most U_1)
    return want
