"""GPU (-m gpu): the byte-wide k-mer tables (option prune_table_bits) and the third level of the pruning bound (option
prune_refine3, 256 segments).

The device's tables, whatever their width, must be the host mirror's entry for entry; after a search under the three
levels every pair's bound must be what the mirrors give -- the first level's, the lesser of it and the second's where it
reached the stage's T, the least of the three where that still did; the result must not depend on the tables' width; and
the hits must be the unpruned search's."""
import numpy as np
import pytest

from test_gpu_parity import _reset_options
from test_gpu_prune import _segment_blocks
from test_gpu_prune_kmer import _pair_sequences

pytestmark = pytest.mark.gpu

GO, GE = -2, -1
LQ = 300


@pytest.fixture(autouse=True)
def _options(ctx):
    def reset():
        _reset_options(ctx)
        ctx.set_option("prune", 1)
        ctx.set_option("prune_head", 4)
        for key in ("prune_kmer", "prune_segments", "prune_refine", "prune_cut", "prune_refine3", "prune_table_bits"):
            ctx.set_option(key, 0)

    reset()
    ctx.set_option("autotune", 0)
    yield
    reset()
    ctx.set_option("autotune", 1)


def _sub(swg, name):
    return np.asarray(swg.load_scoring(name).table(), dtype=np.int8).reshape(32, 32)


@pytest.fixture(scope="module")
def data(swg):
    """2401 sequences of 118..130 residues (120..132 token rows: the walk's chunk of 32 blocks ends at 128), 1599 of 1..4
    -- so one pair holds a long and a short one --, twelve of the long ones relatives of a stretch of the query, distant
    enough (12 to 48 % of their residues redrawn) for the 10th best score to lie among the unrelated pairs' bounds."""
    rng = np.random.default_rng(0x5EED0D01)
    q = swg.synth_query(0x5EED0D02, LQ)
    seqs = [rng.integers(1, 21, size=int(n)).astype(np.int8) for n in rng.integers(118, 131, size=2401)]
    seqs += [rng.integers(1, 26, size=int(n)).astype(np.int8) for n in rng.integers(1, 5, size=1599)]
    for i in range(12):
        n = len(seqs[7 * i])
        at = int(rng.integers(0, LQ - n))
        s = q[at:at + n].copy()
        hit = rng.random(n) < 0.12 * (1 + i % 4)
        s[hit] = rng.integers(1, 21, size=int(hit.sum()))
        seqs[7 * i] = s
    perm = rng.permutation(len(seqs))
    seqs = [seqs[i] for i in perm]
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    flat = np.concatenate(seqs).astype(np.int8)
    pssm = _sub(swg, "BLOSUM62")[q.astype(np.int64)].copy()
    pssm[151, 9] = 127
    return {"q": q, "flat": flat, "off": off, "pssm127": pssm, "mirrors": {}}


def _geometry(ctx, off):
    for key, v in {"cols_per_wave": 4, "group_lanes": 16, "segment_blocks": _segment_blocks(off, parts=6)}.items():
        ctx.set_option(key, v)


def _queries(swg, data):
    """-> [(label, rows, index query or None, gaps, the tables' automatic width)]"""
    return [("blosum62", _sub(swg, "BLOSUM62"), data["q"], (GO, GE), 8), ("pam250", _sub(swg, "PAM250"), data["q"], (-11, -2), 8),
            ("pssm127", data["pssm127"], None, (-11, -1), 16)]


def _set_query(ctx, swg, rows, q, gaps):
    ctx.set_scoring(_sub(swg, "BLOSUM62") if q is None else rows, gaps[0], gaps[1])
    if q is None:
        ctx.set_query_pssm(rows)
    else:
        ctx.set_query(q)


def _pair_mirrors(swg, data, label, rows, q, gaps, pflat, poff):
    """-> the three levels' pair bounds from the host mirrors (32, 128, 256 segments), computed once per query"""
    if label not in data["mirrors"]:
        out = []
        for S in (32, 128, 256):
            u = (swg.debug_prune_kmer_seg(rows, q, gaps[0], gaps[1], 4, 32, pflat, poff, table=False) if S == 32
                 else swg.debug_prune_kmer_refine(rows, q, gaps[0], gaps[1], S, pflat, poff, table=False))[1]
            out.append(np.maximum(u[0::2], u[1::2]).astype(np.int64))
        data["mirrors"][label] = out
    return data["mirrors"][label]


# ---------------------------------------------------------------------------------------------------------------------
# the tables

@pytest.fixture(scope="module")
def table_mirrors(swg):
    cache = {}

    def get(lq):
        if lq not in cache:
            sub = _sub(swg, "BLOSUM62")
            q = swg.synth_query(0x5EED0D03, 300)[:lq].copy()
            one, off1 = np.array([1], dtype=np.int8), np.array([0, 1], dtype=np.uint64)
            cache[lq] = (q, {(4, 32): swg.debug_prune_kmer_seg(sub, q, GO, GE, 4, 32, one, off1)[0],
                             (4, 128): swg.debug_prune_kmer_refine(sub, q, GO, GE, 128, one, off1)[0],
                             (4, 256): swg.debug_prune_kmer_refine(sub, q, GO, GE, 256, one, off1)[0],
                             (5, 8): swg.debug_prune_kmer_seg(sub, q, GO, GE, 5, 8, one, off1)[0]})
        return cache[lq]

    return get


@pytest.mark.parametrize("bits", [0, 16])
@pytest.mark.parametrize("lq", [1, 255, 256, 257, 300])
def test_device_tables_equal_the_mirror(swg, ctx, table_mirrors, lq, bits):
    """(k, S) = (4, 32), (4, 128), (4, 256) from one search under the three levels, (5, 8) from a second; lq = 256 is the
    table kernel's chunk, lq = 1 leaves 255 segments empty, lq = 300 at 256 segments fills 150 of two columns."""
    q, want = table_mirrors(lq)
    flat, off = swg.synth_db(0x5EED0D04, 600, median=40, max_len=200)
    ctx.set_scoring(_sub(swg, "BLOSUM62"), GO, GE)
    ctx.set_query(q)
    db = swg.Database(flat, off).upload(ctx)
    ctx.set_option("prune", 2)
    ctx.set_option("prune_table_bits", bits)
    width = bits or 8
    for key, v in (("prune_kmer", 4), ("prune_segments", 32), ("prune_refine", 128), ("prune_refine3", 256)):
        ctx.set_option(key, v)
    before = ctx.debug_prune_tables()
    ctx.search(db, want_scores=False, k=10)
    assert ctx.prune_last()["pruned"]
    info = ctx.debug_prune_tables()
    assert info["refine3"] == 256 and info["refine3_builds"] == before["refine3_builds"] + 1 and info["auto_bits"] == 8
    assert (info["bits"]["first4"], info["bits"]["second"], info["bits"]["third"]) == (width, width, width), info
    got = ctx.debug_prune_kmer_seg_read(db, k=4, segments=32)
    assert got["table"].dtype == np.uint16 and np.array_equal(got["table"], want[(4, 32)]), (lq, bits)
    for S in (128, 256):
        t = ctx.debug_prune_refine_read(db, segments=S)["table"]
        assert t.dtype == np.uint16 and np.array_equal(t, want[(4, S)]), (lq, bits, S, np.argwhere(t != want[(4, S)])[:3])
    if lq == 300:
        assert np.any(want[(4, 256)][:, 149]) and not np.any(want[(4, 256)][:, 150:])
    # the same search again builds nothing
    ctx.search(db, want_scores=False, k=10)
    assert ctx.debug_prune_tables()["refine3_builds"] == info["refine3_builds"]
    for key, v in (("prune_kmer", 5), ("prune_segments", 8), ("prune_refine", 1), ("prune_refine3", 1)):
        ctx.set_option(key, v)
    ctx.search(db, want_scores=False, k=10)
    assert ctx.prune_last()["pruned"]
    info = ctx.debug_prune_tables()
    assert info["refine3"] == 0 and info["bits"]["first5"] == width, info
    got = ctx.debug_prune_kmer_seg_read(db, k=5, segments=8)
    assert np.array_equal(got["table"], want[(5, 8)]), (lq, bits)
    db.close()


def test_a_width_is_a_table_of_its_own(swg, ctx, table_mirrors):
    """The same query under the other prune_table_bits: every table is built anew, once."""
    q, _ = table_mirrors(257)
    flat, off = swg.synth_db(0x5EED0D04, 600, median=40, max_len=200)
    ctx.set_scoring(_sub(swg, "BLOSUM62"), GO, GE)
    ctx.set_query(q)
    db = swg.Database(flat, off).upload(ctx)
    ctx.set_option("prune", 2)
    for key, v in (("prune_kmer", 4), ("prune_segments", 32), ("prune_refine", 128), ("prune_refine3", 256)):
        ctx.set_option(key, v)
    counts = []
    for bits in (0, 0, 16, 16, 0):
        ctx.set_option("prune_table_bits", bits)
        _, hits, _ = ctx.search(db, want_scores=False, k=10)
        r, t = ctx.debug_prune_refine_read(db, arrays=False), ctx.debug_prune_tables()
        counts.append((r["builds"], r["refine_builds"], t["refine3_builds"], t["bits"]["third"], hits))
    base = counts[0]
    for i, step in enumerate((0, 0, 1, 1, 2)):
        assert counts[i][:3] == (base[0] + step, base[1] + step, base[2] + step), (i, counts[i][:4])
        assert counts[i][3] == (16 if i in (2, 3) else 8) and counts[i][4] == base[4]
    with pytest.raises(Exception, match="prune_table_bits"):
        ctx.set_option("prune_table_bits", 8)
    with pytest.raises(Exception, match="prune_refine3"):
        ctx.set_option("prune_refine3", 128)
    db.close()


# ---------------------------------------------------------------------------------------------------------------------
# the bounds of the three levels

def _expected_bounds(stages, n_pairs, first, second, third, with_third):
    """What a search leaves: in a cut stage a pair at or above T is walked again, level by level; elsewhere the first level's."""
    want = first.copy()
    for begin, end, T, _ in stages:
        p = np.arange(begin, min(end, n_pairs))
        b = first[p].copy()
        walk = b >= T
        b[walk] = np.minimum(b[walk], second[p][walk])
        if with_third:
            walk = b >= T
            b[walk] = np.minimum(b[walk], third[p][walk])
        want[p] = b
    return want


def test_bounds_are_the_least_of_the_three_mirrors(swg, ctx, data):
    flat, off = data["flat"], data["off"]
    label, rows, q, gaps, _ = _queries(swg, data)[0]
    _set_query(ctx, swg, rows, q, gaps)
    db = swg.Database(flat, off).upload(ctx)
    pflat, poff = _pair_sequences(db, flat, off)
    first, second, third = _pair_mirrors(swg, data, label, rows, q, gaps, pflat, poff)
    n = len(first)
    lens = np.diff(poff.astype(np.int64))[0::2]
    ylens = np.array([np.count_nonzero(pflat[int(poff[2 * i + 1]):int(poff[2 * i + 2])]) for i in range(n)])
    assert np.any((lens >= 118) & (ylens <= 4)) and {30, 31, 32, 33} <= set(int(v) for v in (2 + lens + 3) // 4)
    _geometry(ctx, off)
    ctx.set_option("prune", 2)
    for key, v in (("prune_kmer", 4), ("prune_segments", 32), ("prune_refine", 128), ("prune_refine3", 256)):
        ctx.set_option(key, v)
    seen = {}
    for bits in (0, 16):
        ctx.set_option("prune_table_bits", bits)
        _, hits, _ = ctx.search(db, want_scores=False, k=10)
        info = ctx.prune_last()
        got = ctx.debug_prune_refine_read(db)
        assert info["pruned"] and info["threshold"] > 0 and got["refine"] == 128 and ctx.debug_prune_tables()["refine3"] == 256
        assert len(got["stages"]) >= 4
        b = got["bounds"].astype(np.int64)
        want = _expected_bounds(got["stages"], n, first, second, third, True)
        assert np.array_equal(b[:n], want), (bits, np.flatnonzero(b[:n] != want)[:5])
        assert not np.any(b[n:])
        # the third level did cut: pairs the second left at or above their stage's T, now below it
        cut3 = sum(int(np.sum((np.minimum(first, second)[bg:min(e, n)] >= T) & (b[bg:min(e, n)] < T))) for bg, e, T, _ in got["stages"])
        assert cut3 > 0
        for begin, end, T, lst in got["stages"]:
            assert np.array_equal(lst.astype(np.int64), begin + np.flatnonzero(b[begin:end] >= T)), (bits, begin)
        seen[bits] = (hits, info, b.copy(), [(s[0], s[1], s[2]) for s in got["stages"]])
    assert seen[0][0] == seen[16][0] and seen[0][1] == seen[16][1] and np.array_equal(seen[0][2], seen[16][2]) and seen[0][3] == seen[16][3]
    # without the third level: the lesser of two
    ctx.set_option("prune_refine3", 1)
    ctx.set_option("prune_table_bits", 0)
    ctx.search(db, want_scores=False, k=10)
    got = ctx.debug_prune_refine_read(db)
    assert ctx.debug_prune_tables()["refine3"] == 0
    assert np.array_equal(got["bounds"].astype(np.int64)[:n], _expected_bounds(got["stages"], n, first, second, third, False))
    db.close()


# ---------------------------------------------------------------------------------------------------------------------
# the hits

@pytest.mark.parametrize("which", [0, 1, 2], ids=["blosum62", "pam250", "pssm127"])
def test_hits_equal_the_unpruned_search(swg, ctx, data, which):
    flat, off = data["flat"], data["off"]
    label, rows, q, gaps, auto_bits = _queries(swg, data)[which]
    _set_query(ctx, swg, rows, q, gaps)
    db = swg.Database(flat, off).upload(ctx)
    pflat, poff = _pair_sequences(db, flat, off)
    first, second, third = _pair_mirrors(swg, data, label, rows, q, gaps, pflat, poff)
    n = len(first)
    _geometry(ctx, off)
    plain = {}
    for k in (1, 10):
        ctx.set_option("prune", 0)
        _, plain[k], _ = ctx.search(db, want_scores=False, k=k)
        assert not ctx.prune_last()["pruned"] and len(plain[k]) == k
    T10 = plain[10][-1][0]
    above_plain = ctx.search_above(db, T10)[:2]
    assert T10 > 0 and above_plain[1] >= 10
    ctx.set_option("prune", 2)
    for key, v in (("prune_kmer", 4), ("prune_segments", 32), ("prune_refine", 128)):
        ctx.set_option(key, v)
    for bits in (0, 16):
        for r3 in (1, 256):
            ctx.set_option("prune_table_bits", bits)
            ctx.set_option("prune_refine3", r3)
            for k in (1, 10):
                _, hits, _ = ctx.search(db, want_scores=False, k=k)
                assert ctx.prune_last()["pruned"] and hits == plain[k], (label, bits, r3, k, ctx.prune_last())
                t = ctx.debug_prune_tables()
                want_bits = 16 if bits == 16 else auto_bits
                assert t["refine3"] == (256 if r3 == 256 else 0) and t["auto_bits"] == auto_bits
                assert t["bits"]["first4"] == want_bits and t["bits"]["second"] == want_bits, (label, bits, t)
                if r3 == 256:
                    assert t["bits"]["third"] == want_bits
            # every hit at or above the 10th's score, and what the mirrors say is skipped
            above = ctx.search_above(db, T10)[:2]
            info = ctx.prune_last()
            got = ctx.debug_prune_refine_read(db)
            assert info["pruned"] and above == above_plain, (label, bits, r3)
            pairs = got["pairs"]
            f = np.zeros(pairs, dtype=np.int64)
            f[:n] = first
            skipped = 0
            assert got["stages"] and got["stages"][0][0] == 0 and got["stages"][-1][1] == pairs
            for si, (begin, end, T, _) in enumerate(got["stages"]):
                assert T == T10
                b = f[begin:end].copy()
                e = min(end, n)
                # (the first of several stages is walked again only where the first level cut an eighth of it)
                gated_off = si == 0 and len(got["stages"]) > 1 and int(np.sum(b < T)) * 8 < end - begin
                if not gated_off and e > begin:
                    w = b[:e - begin] >= T
                    b[:e - begin][w] = np.minimum(b[:e - begin][w], second[begin:e][w])
                    if r3 == 256:
                        w = b[:e - begin] >= T
                        b[:e - begin][w] = np.minimum(b[:e - begin][w], third[begin:e][w])
                assert np.array_equal(got["bounds"].astype(np.int64)[begin:end], b), (label, bits, r3, si)
                skipped += int(np.sum(b < T))
            assert info["pairs_skipped"] == skipped and skipped > 0, (label, bits, r3, info, skipped)
    db.close()
