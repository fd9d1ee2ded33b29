"""Shared by the tests of swg_align_hsps* (several non-overlapping alignments per hit): named cases generated
from seeds, no fixtures.  A case is one pair and one call's limits:

    name, sub (int8[32, 32]), gap_open, gap_extend, query (table indices), seq (table indices), max_hsps, min_score,
    small (the Python model of hsps_model.py is quick enough to judge it)

Every case exists because something specific can go wrong; the comment at its generator says what."""
import numpy as np

AA = np.arange(1, 21, dtype=np.int8)        # the twenty residues' table indices (any of 1..31 would do)


def simple_table(match=3, mismatch=-2):
    t = np.full((32, 32), mismatch, dtype=np.int8)
    t[np.arange(32), np.arange(32)] = match
    return t


def _case(name, sub, gaps, query, seq, max_hsps, min_score, small=True):
    return {"name": name, "sub": np.ascontiguousarray(sub, dtype=np.int8), "gap_open": int(gaps[0]), "gap_extend": int(gaps[1]),
            "query": np.ascontiguousarray(query, dtype=np.int8), "seq": np.ascontiguousarray(seq, dtype=np.int8),
            "max_hsps": int(max_hsps), "min_score": int(min_score), "small": small}


def tiny_cases():
    """One cell: one alignment, then nothing is left.  A pair that scores 0: no alignment at all."""
    t = simple_table()
    return [_case("one_by_one", t, (-4, -1), [5], [5], 4, 1),
            _case("scores_zero", t, (-4, -1), [1, 2, 3], [4, 5, 6, 7], 4, 1)]


REPEAT_UNIT = np.array([1, 2, 3, 4, 5, 6, 7], dtype=np.int8)
# the repeat case by hand: three units against themselves give the main diagonal, then the two diagonals one unit off
# (the smaller database end first), then the two diagonals two units off: (score, q_begin, q_end, d_begin, d_end, steps)
REPEAT_EXPECTED = [(63, 0, 21, 0, 21, 21), (42, 7, 21, 0, 14, 14), (42, 0, 14, 7, 21, 14), (21, 14, 21, 0, 7, 7), (21, 0, 7, 14, 21, 7)]


def repeat_cases():
    """Checkable by hand; the same pair stopped by the cap and stopped by the score."""
    t, s = simple_table(3, -2), np.tile(REPEAT_UNIT, 3)
    return [_case("repeat", t, (-4, -1), s, s, 6, 10), _case("repeat_cap2", t, (-4, -1), s, s, 2, 10),
            _case("repeat_min43", t, (-4, -1), s, s, 6, 43)]


def domain_cases(b62):
    """Two planted domains: in swapped order (two alignments, disjoint in both sequences), and in order with a
    60-residue insert between them, which one gapped alignment bridges or two alignments leave out, by the gap scores."""
    rng = np.random.default_rng(0xD0A1)
    a, b = rng.choice(AA, 30), rng.choice(AA, 30)
    flank = lambda n: rng.choice(AA, n)                       # noqa: E731
    query = np.concatenate([a, flank(5), b])
    swapped = np.concatenate([flank(4), b, flank(7), a, flank(3)])
    insert = np.concatenate([a, flank(5), flank(60), b])
    return [_case("domains_swapped", b62, (-11, -1), query, swapped, 4, 40),
            _case("domains_insert_bridged", b62, (-11, -1), query, insert, 4, 40),
            _case("domains_insert_split", b62, (-20, -5), query, insert, 4, 40)]


RANDOM_GAPS = [(-2, -1), (-4, -1), (0, -1), (-1, 0), (0, 1), (1, -3)]


def random_cases(pairs_per_setting=5):
    """A 4-letter alphabet: many ties, many rounds, later paths that cross earlier ones through a gap; gap scores of
    either sign; every stop reason."""
    rng = np.random.default_rng(0x4A11)
    t = simple_table(3, -2)
    out = []
    for gaps in RANDOM_GAPS:
        for n in range(pairs_per_setting):
            q = rng.integers(1, 5, rng.integers(1, 41))
            d = rng.integers(1, 5, rng.integers(1, 41))
            for ms in (1, 9):
                out.append(_case("random_g%d_%d_n%d_min%d" % (gaps[0], gaps[1], n, ms), t, gaps, q, d, 8, ms))
    return out


def _planted(rng, query, spans, total):
    """A sequence of `total` residues holding the query's columns spans[k] = (begin, end), in the order given, spread
    over random residues."""
    free = total - sum(e - b for b, e in spans)
    assert free >= 0
    cuts = np.sort(rng.integers(0, free + 1, len(spans)))
    parts, at = [], 0
    for (b, e), c in zip(spans, cuts):
        parts += [rng.choice(AA, c - at), query[b:e]]
        at = c
    parts.append(rng.choice(AA, free - at))
    return np.concatenate(parts)


def width_cases(b62):
    """The 256-lane stride (255, 256, 257, 600 columns), either side of the LDS limit (1700, 1701), and a diagonal
    shorter than the workgroup (20 columns against 300 residues): sequences of 48 to 96 residues, so a pair's predecessor
    bytes stay small; three planted pieces of the query -- its first columns, its last, and some in between, out of
    order -- so that at least three rounds run and the last column's lane has work."""
    rng = np.random.default_rng(0x71DE)
    out = []
    for lq in (255, 256, 257, 600, 1700, 1701):
        q = rng.choice(AA, lq)
        mid = lq // 2
        spans = [(lq - 24, lq), (0, 20), (mid - 8, mid + 10)]
        out.append(_case("width_%d" % lq, b62, (-11, -1), q, _planted(rng, q, spans, int(rng.integers(70, 97))), 5, 30, small=False))
    q = rng.choice(AA, 20)
    out.append(_case("width_20x300", b62, (-11, -1), q, _planted(rng, q, [(0, 20), (0, 20), (2, 20)], 300), 5, 30, small=False))
    return out


def matrix_cases(b62, pam250):
    """The two matrices with the gap scores the alignment tests use, on related sequences with repeats."""
    rng = np.random.default_rng(0xB62)
    out = []
    for name, sub, gaps, ms in (("blosum62", b62, (-11, -1), 25), ("pam250", pam250, (-2, -1), 30)):
        q = rng.choice(AA, 36)
        d = np.concatenate([q[18:36], rng.choice(AA, 6), q[0:20], rng.choice(AA, 4), q[10:30]])
        flip = rng.random(d.size) < 0.12
        d = np.where(flip, rng.choice(AA, d.size), d)
        out.append(_case("matrix_" + name, sub, gaps, q, d, 6, ms))
    return out


def free_pssm_case():
    """A PSSM that is no matrix's rows: (pssm int8[lq, 32], gaps, seq, max_hsps, min_score)."""
    rng = np.random.default_rng(0x9551)
    pssm = rng.integers(-6, 9, (31, 32)).astype(np.int8)
    seq = rng.choice(AA, 57)
    return {"name": "free_pssm", "pssm": pssm, "gap_open": -7, "gap_extend": -1, "seq": seq.astype(np.int8), "max_hsps": 8, "min_score": 12}


def small_cases(b62, pam250):
    return tiny_cases() + repeat_cases() + domain_cases(b62) + random_cases() + matrix_cases(b62, pam250)


def all_cases(b62, pam250):
    return small_cases(b62, pam250) + width_cases(b62)


def pssm_of(case):
    """The PSSM whose rows are the matrix rows of the case's query: it must give the case's alignments."""
    return np.ascontiguousarray(case["sub"][case["query"].astype(np.int64)], dtype=np.int8)
