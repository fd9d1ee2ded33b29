"""GPU (-m gpu): the fourth level of the pruning bound (option prune_refine4) -- blocks of 5 residues over
256 segments, behind the three levels of k = 4 -- and the prefix-shared table kernel of k = 5 that builds its table.

The device's table must be the recurrence's entry for entry; after a search under the four levels every pair's bound
must be what the mirrors give, level by level; each stage's list must be the pairs whose bound reaches its T; the hits
must be the unpruned search's and the oracle's; a query whose k = 5 entries need 16 bits runs without the level."""
import numpy as np
import pytest

from test_gpu_parity import _reset_options
from test_gpu_prune_kmer import _pair_sequences
from test_prune_deep_host import numpy_table5

pytestmark = pytest.mark.gpu

GO, GE = -2, -1
LQ = 300
EDGE_BLOCKS = (4, 5, 6, 9, 10, 11, 31, 32, 33, 160, 161)   # the five-uint4 unit, its tail and the chunk of 32 units
PRUNE_KEYS = ("prune_kmer", "prune_segments", "prune_refine", "prune_cut", "prune_refine3", "prune_refine4", "prune_table_bits")


@pytest.fixture(autouse=True)
def _options(ctx):
    def reset():
        _reset_options(ctx)
        ctx.set_option("prune", 1)
        ctx.set_option("prune_head", 4)
        for key in PRUNE_KEYS:
            ctx.set_option(key, 0)

    reset()
    ctx.set_option("autotune", 0)
    yield
    reset()
    ctx.set_option("autotune", 1)


def _sub(swg, name):
    return np.asarray(swg.load_scoring(name).table(), dtype=np.int8).reshape(32, 32)


def _force_levels(ctx, swg, fourth=True):
    ctx.set_option("prune", 2)
    for key, v in (("prune_kmer", 4), ("prune_segments", 32), ("prune_refine", 128), ("prune_refine3", 256),
                   ("prune_refine4", swg.PRUNE_REFINE4_FORCED if fourth else 1)):
        ctx.set_option(key, v)


# ---------------------------------------------------------------------------------------------------------------------
# the table

def _sample_blocks(rng):
    """-> class blocks [n][5]: random ones over all 22 classes, and ones with leading, inner and trailing padding (class 0)
    and with class 21 at every place"""
    blocks = [rng.integers(0, 22, size=(1500, 5)), rng.integers(1, 21, size=(1500, 5))]
    for place in ([0], [4], [2], [0, 1], [3, 4], [1, 3], [0, 1, 2, 3], [1, 2, 3, 4], [0, 1, 2, 3, 4]):
        b = rng.integers(1, 22, size=(40, 5))
        b[:, place] = 0
        blocks.append(b)
    for j in range(5):
        b = rng.integers(1, 21, size=(40, 5))
        b[:, j] = 21
        blocks.append(b)
    blocks.append(np.array([[0, 0, 0, 0, 0], [21, 21, 21, 21, 21], [21, 0, 21, 0, 21], [1, 1, 1, 1, 1], [20, 20, 20, 20, 0]]))
    return np.unique(np.concatenate(blocks).astype(np.int64), axis=0)


@pytest.mark.parametrize("lq", [37, 300, 777])
def test_the_fourth_table_equals_the_recurrence(swg, ctx, lq):
    """lq = 37 leaves 219 of the 256 segments without columns, 300 and 777 are no multiples of 256 (W = 2 and 4, the last
    segments empty); 777 is more than three of the kernel's chunks of 256 columns."""
    rng = np.random.default_rng(0x5EED0E01 + lq)
    q = swg.synth_query(0x5EED0E02, 777)[:lq].copy()
    sub = _sub(swg, "BLOSUM62")
    cls = _sample_blocks(rng)
    assert len(cls) > 3000
    want, _ = numpy_table5(swg, sub, q, (GO, GE), 256, cls)
    flat, off = swg.synth_db(0x5EED0E03, 600, median=40, max_len=200)
    ctx.set_scoring(sub, GO, GE)
    ctx.set_query(q)
    db = swg.Database(flat, off).upload(ctx)
    _force_levels(ctx, swg)
    before = ctx.debug_prune_tables4()
    ctx.search(db, want_scores=False, k=10)
    info = ctx.debug_prune_tables4()
    assert ctx.prune_last()["pruned"] and not info["refused"]
    assert info["refine4"] == 256 and info["bits"] == 8 and info["refine4_builds"] == before["refine4_builds"] + 1
    ix = ((((cls[:, 0] * 22 + cls[:, 1]) * 22 + cls[:, 2]) * 22 + cls[:, 3]) * 22 + cls[:, 4]).astype(np.uint32)
    got = ctx.debug_prune_refine4_read(ix).astype(np.int64)
    assert np.array_equal(got, want), (lq, np.argwhere(got != want)[:3])
    W = -(-lq // 256)
    assert np.any(got[:, (lq - 1) // W]) and not np.any(got[:, (lq - 1) // W + 1:])
    # the same search again builds nothing
    ctx.search(db, want_scores=False, k=10)
    assert ctx.debug_prune_tables4()["refine4_builds"] == info["refine4_builds"]
    db.close()


@pytest.mark.parametrize("bits", [0, 16])
@pytest.mark.parametrize("lq", [37, 300, 777])
def test_the_table_of_5_in_8_segments_equals_the_mirror(swg, ctx, lq, bits):
    """The same kernel as a first-level table, (5, 8), in both entry widths: one 8-byte store per row as bytes, two as
    uint16_t; the whole table against the mirror's."""
    q = swg.synth_query(0x5EED0E02, 777)[:lq].copy()
    sub = _sub(swg, "BLOSUM62")
    one, off1 = np.array([1], dtype=np.int8), np.array([0, 1], dtype=np.uint64)
    want = swg.debug_prune_kmer_seg(sub, q, GO, GE, 5, 8, one, off1)[0]
    flat, off = swg.synth_db(0x5EED0E03, 600, median=40, max_len=200)
    ctx.set_scoring(sub, GO, GE)
    ctx.set_query(q)
    db = swg.Database(flat, off).upload(ctx)
    ctx.set_option("prune", 2)
    ctx.set_option("prune_table_bits", bits)
    for key, v in (("prune_kmer", 5), ("prune_segments", 8), ("prune_refine", 1), ("prune_refine3", 1)):
        ctx.set_option(key, v)
    ctx.search(db, want_scores=False, k=10)
    assert ctx.prune_last()["pruned"] and ctx.debug_prune_tables()["bits"]["first5"] == (bits or 8)
    got = ctx.debug_prune_kmer_seg_read(db, k=5, segments=8)
    assert np.array_equal(got["table"], want), (lq, bits, np.argwhere(got["table"] != want)[:3])
    # ... and unsegmented: single entries, no packed store
    ctx.set_option("prune_segments", 1)
    ctx.search(db, want_scores=False, k=10)
    got = ctx.debug_prune_kmer_read(db, k=5)
    assert np.array_equal(got["table"], want.max(axis=1)), (lq, bits)
    db.close()


# ---------------------------------------------------------------------------------------------------------------------
# the bounds of the four levels

@pytest.fixture(scope="module")
def data(swg):
    """60 sequences of 900..1000 residues (the first stage); six each of the lengths whose pairs have EDGE_BLOCKS token
    blocks, four of the six behind a copy of 20 residues of the query (or of all they have), with B, Z, X and the indices
    27..30 in some; 2401 of 119..130 residues, twelve of them distant relatives of a stretch of the query; 1599 of 1..4.
    In the length order the 41-residue sequences lie between those, so a second database ("long_short") holds the 2401 and
    the 1599 alone: one of its pairs is a sequence of 119 or more residues beside one of at most 4."""
    rng = np.random.default_rng(0x5EED0E04)
    q = swg.synth_query(0x5EED0E05, LQ)
    seqs = [rng.integers(1, 21, size=int(n)).astype(np.int8) for n in rng.integers(900, 1001, size=60)]
    odd = np.array([2, 26, 24, 27, 28, 29, 30], dtype=np.int8)   # B, Z, X and the indices behind Z
    for nb in EDGE_BLOCKS:
        n = 4 * nb - 3
        for j in range(6):
            s = rng.integers(1, 21, size=n).astype(np.int8)
            if j < 4:
                at = (40 * j + nb) % (LQ - 20)
                s[:min(n, 20)] = q[at:at + min(n, 20)]   # (scores at least 4 x 13 under BLOSUM62)
            if j == 5 or (j in (1, 3) and n > 29):
                at = (0 if j == 5 else 20) + rng.choice(n - (0 if j == 5 else 20), size=max(1, n // 9), replace=False)
                s[at] = rng.choice(odd, size=len(at))
            seqs.append(s)
    body = [rng.integers(1, 21, size=int(n)).astype(np.int8) for n in rng.integers(119, 131, size=2401)]
    for i in range(12):
        n = len(body[7 * i])
        at = int(rng.integers(0, LQ - n))
        s = q[at:at + n].copy()
        hit = rng.random(n) < 0.12 * (1 + i % 4)
        s[hit] = rng.integers(1, 21, size=int(hit.sum()))
        body[7 * i] = s
    short = [rng.integers(1, 31, size=int(n)).astype(np.int8) for n in rng.integers(1, 5, size=1599)]

    def packed(seqs):
        seqs = [seqs[i] for i in rng.permutation(len(seqs))]
        off = np.zeros(len(seqs) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(s) for s in seqs])
        return np.concatenate(seqs).astype(np.int8), off

    flat, off = packed(seqs + body + short)
    long_short = packed(body + short)
    pssm = _sub(swg, "BLOSUM62")[q.astype(np.int64)].copy()
    pssm51, pssm52 = pssm.copy(), pssm.copy()
    pssm51[151, 9] = 51
    pssm52[151, 9] = 52
    return {"q": q, "flat": flat, "off": off, "long_short": long_short, "pssm51": pssm51, "pssm52": pssm52, "mirrors": {}}


def _geometry(ctx, off):
    """Four passes, and launch segments of the first stage's size: the 30 longest pairs"""
    lens = np.sort(np.diff(off.astype(np.int64)))[::-1]
    blocks = (lens[0::2] + 2 + 3) // 4
    for key, v in {"cols_per_wave": 4, "group_lanes": 16, "segment_blocks": int(blocks[:30].sum())}.items():
        ctx.set_option(key, v)


def _set_query(ctx, swg, rows, q, gaps):
    ctx.set_scoring(_sub(swg, "BLOSUM62") if q is None else rows, gaps[0], gaps[1])
    if q is None:
        ctx.set_query_pssm(rows)
    else:
        ctx.set_query(q)


def _pair_mirrors(swg, data, label, rows, q, gaps, pflat, poff):
    """-> the four levels' pair bounds from the host mirrors, computed once per query"""
    if label not in data["mirrors"]:
        out = []
        for S in (32, 128, 256):
            u = (swg.debug_prune_kmer_seg(rows, q, gaps[0], gaps[1], 4, 32, pflat, poff, table=False) if S == 32
                 else swg.debug_prune_kmer_refine(rows, q, gaps[0], gaps[1], S, pflat, poff, table=False))[1]
            out.append(np.maximum(u[0::2], u[1::2]).astype(np.int64))
        u = swg.debug_prune_kmer_refine4(rows, q, gaps[0], gaps[1], 256, pflat, poff)
        out.append(np.maximum(u[0::2], u[1::2]).astype(np.int64))
        data["mirrors"][label] = out
    return data["mirrors"][label]


def _expected_bounds(stages, n_pairs, mirrors, fixed):
    """What a search leaves: in a cut stage a pair at or above T is walked again, level by level, and keeps the least bound;
    elsewhere the first level's.  -> (bounds, walked by the fourth level [n_pairs], cut by the fourth level alone)"""
    want = mirrors[0].copy()
    walked4 = np.zeros(n_pairs, dtype=bool)
    cut4 = 0
    for si, (begin, end, T, _) in enumerate(stages):
        p = np.arange(begin, min(end, n_pairs))
        b = mirrors[0][p].copy()
        # (a caller's threshold: the first of several stages is walked again only where the first level cut an eighth of it)
        if fixed and si == 0 and len(stages) > 1 and (int(np.sum(b < T)) + max(0, end - n_pairs)) * 8 < end - begin:
            continue
        for level in (1, 2, 3):
            walk = b >= T
            if level == 3:
                walked4[p[walk]] = True
                cut4 += int(np.sum(walk & (mirrors[3][p] < T)))
            b[walk] = np.minimum(b[walk], mirrors[level][p][walk])
        want[p] = b
    return want, walked4, cut4


def _check_bounds(ctx, db, n, mirrors, fixed):
    got = ctx.debug_prune_refine_read(db)
    assert got["refine"] == 128 and ctx.debug_prune_tables()["refine3"] == 256 and ctx.debug_prune_tables4()["refine4"] == 256
    b = got["bounds"].astype(np.int64)
    want, walked4, cut4 = _expected_bounds(got["stages"], n, mirrors, fixed)
    assert np.array_equal(b[:n], want), np.flatnonzero(b[:n] != want)[:5]
    assert not np.any(b[n:])
    for begin, end, T, lst in got["stages"]:
        assert np.array_equal(lst.astype(np.int64), begin + np.flatnonzero(b[begin:end] >= T)), begin
    return got, walked4, cut4


@pytest.mark.parametrize("which", ["edges", "long_short"])
def test_bounds_are_the_least_of_the_four_mirrors(swg, ctx, data, which):
    flat, off = (data["flat"], data["off"]) if which == "edges" else data["long_short"]
    q = data["q"]
    sub = _sub(swg, "BLOSUM62")
    _set_query(ctx, swg, sub, q, (GO, GE))
    db = swg.Database(flat, off).upload(ctx)
    pflat, poff = _pair_sequences(db, flat, off)
    mirrors = _pair_mirrors(swg, data, which, sub, q, (GO, GE), pflat, poff)
    n = len(mirrors[0])
    lens = np.diff(poff.astype(np.int64))[0::2]
    nb = (2 + lens + 3) // 4
    ylens = np.array([np.count_nonzero(pflat[int(poff[2 * i + 1]):int(poff[2 * i + 2])]) for i in range(n)])
    long_short = (lens > 118) & (ylens <= 4)
    if which == "edges":
        assert set(EDGE_BLOCKS) <= set(int(v) for v in nb) and all(np.any(pflat == r) for r in (2, 24, 26, 27, 28, 29, 30))
    else:
        assert np.any(long_short)
    _geometry(ctx, off)
    _force_levels(ctx, swg)
    # the K-th best so far: T rises from stage to stage
    ctx.search(db, want_scores=False, k=10)
    info = ctx.prune_last()
    assert info["pruned"] and info["threshold"] > 0
    got, walked4, cut4 = _check_bounds(ctx, db, n, mirrors, False)
    assert len(got["stages"]) >= 4
    assert cut4 > 0   # pairs every k = 4 level left at or above their stage's T, below it by the blocks of 5 alone
    # a caller's threshold below every copy's score: every stage is cut, and pairs of every edge length are walked to
    # the fourth level -- the short y beside a long x among them
    hits, total, _ = ctx.search_above(db, 40)
    assert ctx.prune_last()["pruned"] and total > 100
    got, walked4, cut4 = _check_bounds(ctx, db, n, mirrors, True)
    assert all(T == 40 for _, _, T, _ in got["stages"])
    if which == "edges":
        assert set(EDGE_BLOCKS) <= set(int(v) for v in nb[walked4]), sorted(set(int(v) for v in nb[walked4]))
    else:
        assert np.any(walked4 & long_short)
    # without the fourth level: the least of three
    ctx.set_option("prune_refine4", 1)
    ctx.search(db, want_scores=False, k=10)
    got = ctx.debug_prune_refine_read(db)
    assert ctx.debug_prune_tables4()["refine4"] == 0
    want, _, _ = _expected_bounds(got["stages"], n, mirrors[:3] + [np.full(n, 1 << 40)], False)
    assert np.array_equal(got["bounds"].astype(np.int64)[:n], want)
    db.close()


# ---------------------------------------------------------------------------------------------------------------------
# the hits

def _queries(swg, data):
    """-> [(label, rows, index query or None, gaps, whether the fourth level runs)]"""
    return [("blosum62", _sub(swg, "BLOSUM62"), data["q"], (GO, GE), True), ("pam250", _sub(swg, "PAM250"), data["q"], (-11, -2), True),
            ("pssm51", data["pssm51"], None, (-11, -1), True), ("pssm52", data["pssm52"], None, (-11, -1), False)]


@pytest.mark.parametrize("which", [0, 1, 2, 3], ids=["blosum62", "pam250", "pssm51", "pssm52"])
def test_hits_equal_the_unpruned_search(swg, orc, ctx, data, which):
    """A PSSM whose largest entry is 51 has byte tables at k = 5 (5 x 51 = 255); one with 52 has not (260), while its k = 4
    tables are still bytes: the search runs under three levels, without an error, and returns the same hits."""
    flat, off = data["flat"], data["off"]
    label, rows, q, gaps, has_fourth = _queries(swg, data)[which]
    _set_query(ctx, swg, rows, q, gaps)
    db = swg.Database(flat, off).upload(ctx)
    _geometry(ctx, off)
    plain = {}
    for k in (1, 10):
        ctx.set_option("prune", 0)
        _, plain[k], _ = ctx.search(db, want_scores=False, k=k)
        assert not ctx.prune_last()["pruned"] and len(plain[k]) == k
    if q is not None:
        scores = orc.score_db(q, flat, off, rows, gaps[0], gaps[1])
        assert plain[10] == orc.topk(scores, 10)
    T10 = plain[10][-1][0]
    above_plain = ctx.search_above(db, T10)[:2]
    assert T10 > 0 and above_plain[1] >= 10
    assert swg.debug_prune_table_bits(rows, q, 5) == (8 if has_fourth else 16) and swg.debug_prune_table_bits(rows, q, 4) == 8
    skipped = {}
    for fourth in (False, True):
        _force_levels(ctx, swg, fourth)
        for k in (1, 10):
            _, hits, _ = ctx.search(db, want_scores=False, k=k)
            t4 = ctx.debug_prune_tables4()
            assert ctx.prune_last()["pruned"] and hits == plain[k], (label, fourth, k, ctx.prune_last())
            assert t4["refine4"] == (256 if fourth and has_fourth else 0) and not t4["refused"], (label, fourth, t4)
            assert ctx.debug_prune_tables()["refine3"] == 256
        skipped[fourth] = ctx.prune_last()["pairs_skipped"]
        assert ctx.search_above(db, T10)[:2] == above_plain, (label, fourth)
    assert skipped[True] >= skipped[False] and (has_fourth or skipped[True] == skipped[False])
    db.close()


# ---------------------------------------------------------------------------------------------------------------------
# the table's life

def test_one_table_for_views_shards_and_searches_in_flight(swg, ctx, data):
    flat, off, q = data["flat"], data["off"], data["q"]
    sub = _sub(swg, "BLOSUM62")
    _set_query(ctx, swg, sub, q, (GO, GE))
    _geometry(ctx, off)
    db = swg.Database(flat, off).upload(ctx)
    ctx.set_option("prune", 0)
    _, plain, _ = ctx.search(db, want_scores=False, k=10)
    _force_levels(ctx, swg)
    _, hits, _ = ctx.search(db, want_scores=False, k=10)
    builds = ctx.debug_prune_tables4()["refine4_builds"]
    assert hits == plain and ctx.debug_prune_tables4()["refine4"] == 256
    # a view of the same database: the context's table, no new build
    members = np.arange(0, len(off) - 1, 2, dtype=np.uint32)
    view = db.view(ctx, members)
    ctx.set_option("prune", 0)
    _, vplain, _ = ctx.search(view, want_scores=False, k=10)
    ctx.set_option("prune", 2)
    _, vhits, _ = ctx.search(view, want_scores=False, k=10)
    assert vhits == vplain and ctx.prune_last()["pruned"]
    assert ctx.debug_prune_tables4() == {"refine4": 256, "refine4_builds": builds, "bits": 8, "refused": False}
    view.close()
    # a shard: another database on the same context
    shard = swg.Database(flat, off, shard_rank=1, shard_count=2).upload(ctx)
    ctx.set_option("prune", 0)
    _, splain, _ = ctx.search(shard, want_scores=False, k=10)
    ctx.set_option("prune", 2)
    _, shits, _ = ctx.search(shard, want_scores=False, k=10)
    assert shits == splain and ctx.debug_prune_tables4()["refine4_builds"] == builds
    # two searches in flight share the one table
    s1 = ctx.search_begin(db, want_scores=False, k=10)
    s2 = ctx.search_begin(shard, want_scores=False, k=10)
    assert ctx.search_end(s1)[1] == plain and ctx.search_end(s2)[1] == splain
    assert ctx.debug_prune_tables4()["refine4_builds"] == builds
    # a new query: a new epoch, the table is built again, once
    ctx.set_query(q[::-1].copy())
    assert ctx.debug_prune_tables4()["bits"] == 0
    ctx.set_option("prune", 0)
    _, rplain, _ = ctx.search(db, want_scores=False, k=10)
    ctx.set_option("prune", 2)
    for _ in range(2):
        _, rhits, _ = ctx.search(db, want_scores=False, k=10)
        assert rhits == rplain and ctx.debug_prune_tables4() == {"refine4": 256, "refine4_builds": builds + 1, "bits": 8, "refused": False}
    with pytest.raises(Exception, match="prune_refine4"):
        ctx.set_option("prune_refine4", 256)
    shard.close()
    db.close()
