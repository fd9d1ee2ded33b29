"""Calls of the reference-shaped replay (swg_fill_batches16) at its edges, and their truths (plain module, no tests of
its own).

swg_fill_batches16 takes [max_len][16] batches exactly as alignment_fill_matrices receives them.  Truth everywhere is the
int32 oracle on a lane's column AS GIVEN: all max_len rows count (the reference computes padded rows as real rows), and
the call delivers min(truth, 32767).  A case is a dict: name, query, sub, gaps, batches [(int8 [max_len, 16],
vector_size)], truth [int32 [vector_size] per batch], all read-only and built once.  tests/test_batches16_cases_host.py
proves on the CPU that the cases are what they claim; tests/test_gpu_batches16.py runs them.

Scoring: "hot" = scoring_edges.diag127(zero0=True) with gaps (-60, -20), as in instantiation_cases: an exact copy of n
query columns scores 127 n and nothing else of a lane can add to it, so 33 rows reach the f16 cells' 4096, 259 the int16
cells' 32767 and 517 the wide form's 65535.  No query holds residue 31, the pad index of oracle.make_batch16: a pad row
matches nothing.

  shape_matrix   one call of many small batches at lq = 40: max_len 1..9, 15, 16, 17 (one token block holds both reset
                 rows and the last-row flag; the flag's row len + 1 moves into block 1 at len = 3) x vector_size 0, 1, 2,
                 3, 15, 16 (max_len 1 has no two different lengths for a third pair: 0..3 only), odd and zero counts in
                 the middle of the call.  The live lanes are exact copies of query stretches, lane 0 of max_len rows, the
                 others shorter and the two of a pair of different lengths: every residue row adds 127 to exactly one
                 lane's score, so a dropped, shifted or swapped row and a swapped lane change a number.  The lanes at or
                 beyond vector_size hold bytes outside 1..31.
  shuffled       the same batches in a seeded random order (ties in max_len: the library sorts them longest first).
  ceilings       lq = 600: lanes whose truths are 4064 and 4191 (either side of the f16 flag), 32766, 32767, 32768, 32893
                 and 66040 (beyond the wide form: the int32 re-score), four of each, among random lanes in the hundreds.
                 The table is the hot one with sub[30][30] = 1 and sub[29][29] = 2; the query holds residue 30 in its first
                 column only and 29 in its last only, so a copy of 258 plain columns with that column in front or behind
                 scores 32766 + 1 or + 2 (one query has to give all seven values in one call).
  multipass      lq = 2100, more than the 2048 columns that 64 lanes x 32 hold: relatives of stretches that lie across
                 every pass boundary a geometry may choose, a third of them with an indel that pays.
  staging        lq = 32: ten batches of about 60 000 rows with two lanes (9.6 MB to stage: three runs of the upload),
                 copies planted in their first rows, in the middle and in their last rows, then thirty small batches.
  mixed          BLOSUM62 (-11, -1), lq = 300: random lanes, every vector_size 0..16.
"""
import functools

import numpy as np

import scoring_edges as se

HOT_GAPS = (-60, -20)
B62_GAPS = (-11, -1)
PAD = 31                                    # oracle.make_batch16's pad index
SENTINEL = -21846                           # what the tests pre-fill max_scores with (0xAAAA): no score of any case
DEAD_BYTES = (0, 32, -1, -128, 127, 64)     # what the lanes at or beyond vector_size hold
MAX_LENS = tuple(range(1, 10)) + (15, 16, 17)
VECTOR_SIZES = (0, 1, 2, 3, 15, 16)
CEILINGS = (4064, 4191, 32766, 32767, 32768, 32893, 66040)
PER_CEILING = 4
STAGE_RUN = 4 << 20                         # the library uploads in runs of about 4 MB
MULTIPASS_LQ = 2100
MULTIPASS_BOUNDARIES = (512, 1024, 1088, 1536, 2048)


def hot_table():
    return se.diag127(zero0=True)


def ceiling_table():
    sub = hot_table()
    sub[30, 30] = 1
    sub[29, 29] = 2
    return sub


def b62_table():
    import swg_loader
    return swg_loader.load().load_scoring("BLOSUM62").table()


def _residues(rng, n, hi=30):
    return rng.integers(1, hi + 1, size=int(n)).astype(np.int8)


def _batch(lanes, max_len, vector_size):
    """lanes: vector_size residue arrays of at most max_len -> [max_len][16] int8, pad rows PAD, dead lanes DEAD_BYTES."""
    assert len(lanes) == vector_size <= 16 and max_len >= 1
    a = np.full((max_len, 16), PAD, dtype=np.int8)
    for l, s in enumerate(lanes):
        assert len(s) <= max_len and (len(s) == 0 or (s.min() >= 1 and s.max() <= 31))
        a[:len(s), l] = s
    rows = np.arange(max_len)
    for l in range(vector_size, 16):
        a[:, l] = np.array(DEAD_BYTES, dtype=np.int8)[(rows + l) % len(DEAD_BYTES)]
    return a


def _case(name, query, sub, gaps, batches):
    """Computes the truths: the int32 oracle on every live lane's whole column."""
    import swg_loader
    orc = swg_loader.oracle()
    cols = [np.ascontiguousarray(a[:, l]) for a, vs in batches for l in range(vs)]
    off = np.zeros(len(cols) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(c) for c in cols])
    flat = np.concatenate(cols) if cols else np.zeros(0, dtype=np.int8)
    scores = orc.score_db(query, flat, off, sub, gaps[0], gaps[1])
    truth, at = [], 0
    for a, vs in batches:
        t = scores[at:at + vs].copy()
        t.setflags(write=False)
        a.setflags(write=False)
        truth.append(t)
        at += vs
    query = np.ascontiguousarray(query, dtype=np.int8)
    query.setflags(write=False)
    sub.setflags(write=False)
    return dict(name=name, query=query, sub=sub, gaps=gaps, batches=batches, truth=truth)


def expected(case):
    """What the call must deliver, per batch: int16 [vector_size] = min(truth, 32767)."""
    return [np.minimum(t, 32767).astype(np.int16) for t in case["truth"]]


def staged_bytes(case):
    return sum(a.shape[0] * 16 for a, _ in case["batches"])


def lane_lengths(max_len, vector_size, b):
    """Lengths of the live lanes of the shape matrix's batch number b: lane 0 has max_len, every other lane less, and the two
    lanes of a pair never the same (the offset 1 + i % (max_len - 1) is no multiple of max_len)."""
    out = []
    for l in range(vector_size):
        i = l // 2
        if l == 0:
            n = max_len
        elif l == 1:
            n = (5 * b + 2) % max_len
        elif l % 2 == 0:
            n = (3 * i + b) % max_len
        else:
            n = ((3 * i + b) % max_len + 1 + i % (max_len - 1)) % max_len
        out.append(n)
    return out


def _copy_batches(q, shapes):
    """One batch per (max_len, vector_size): live lanes are exact copies of stretches of q, of lane_lengths."""
    lq, batches = len(q), []
    for b, (max_len, vs) in enumerate(shapes):
        lanes = []
        for l, n in enumerate(lane_lengths(max_len, vs, b)):
            s = (7 * l + 3 * b) % (lq - n + 1)
            lanes.append(q[s:s + n].copy())
        batches.append((_batch(lanes, max_len, vs), vs))
    return batches


def shapes():
    """(max_len, vector_size) of the shape matrix, longest first as the reference's caller passes them; within one max_len
    the counts are rotated, so zero and odd counts stand in the middle of the call and next to every other count."""
    out = []
    for k, max_len in enumerate(sorted(MAX_LENS, reverse=True)):
        vss = [v for v in VECTOR_SIZES if max_len > 1 or v <= 3]
        vss = vss[k % len(vss):] + vss[:k % len(vss)]
        out += [(max_len, v) for v in vss]
    return out


def shape_matrix(seed=0):
    """seed: which query (40 columns of residues 1..30)."""
    return _shape_matrix(int(seed))


@functools.lru_cache(maxsize=None)
def _shape_matrix(seed):
    q = _residues(np.random.default_rng(0xB160 + seed), 40)
    return _case("shape_matrix_%d" % seed, q, hot_table(), HOT_GAPS, _copy_batches(q, shapes()))


def permutation(n, seed=0):
    return [int(i) for i in np.random.default_rng(0xB161 + seed).permutation(n)]


def shuffled(seed=0):
    """shape_matrix(seed)'s batches in a seeded random order; batch k is the matrix's batch permutation(...)[k]."""
    return _shuffled(int(seed))


@functools.lru_cache(maxsize=None)
def _shuffled(seed):
    c = shape_matrix(seed)
    perm = permutation(len(c["batches"]), seed)
    d = dict(c)
    d.update(name="shuffled_%d" % seed, batches=[c["batches"][i] for i in perm], truth=[c["truth"][i] for i in perm])
    return d


@functools.lru_cache(maxsize=None)
def ceilings():
    rng = np.random.default_rng(0xB162)
    lq = 600
    q = _residues(rng, lq, hi=28)
    q[0], q[lq - 1] = 30, 29
    # (value, first column, columns): plain columns are 1 .. 598, so 520 of them start at 1 .. 79
    plain = lambda n, k: (1 + (23 * k + 5 * n) % (lq - 1 - n), n)
    plant = []
    for k in range(PER_CEILING):
        plant += [(4064,) + plain(32, k), (4191,) + plain(33, k), (32766,) + plain(258, k), (32767, 0, 259),
                  (32768, lq - 259, 259), (32893,) + plain(259, k), (66040,) + plain(520, k)]
    shapes_ = [(530, 16), (600, 15), (521, 16), (523, 13)]
    # where the planted lanes go: seeded, each value twice in an even lane (the pair's x) and twice in an odd one
    slots = [(b, l) for b, (_, vs) in enumerate(shapes_) for l in range(vs)]
    free = [[s for s in slots if s[1] % 2 == par] for par in (0, 1)]
    for f in free:
        rng.shuffle(f)
    lanes_all = [None] * len(slots)
    for i, (_, a, n) in enumerate(plant):
        lanes_all[slots.index(free[(i // 7 + i % 7) % 2].pop())] = q[a:a + n].copy()
    batches, at = [], 0
    for max_len, vs in shapes_:
        lanes = []
        for l in range(vs):
            s = lanes_all[at + l]
            lanes.append(_residues(rng, rng.integers(1, max_len + 1), hi=28) if s is None else s)
        batches.append((_batch(lanes, max_len, vs), vs))
        at += vs
    return _case("ceilings", q, ceiling_table(), HOT_GAPS, batches)


@functools.lru_cache(maxsize=None)
def multipass():
    """-> the case, with "gapped": [(batch, lane)] of the lanes built with an indel."""
    rng = np.random.default_rng(0xB163)
    lq = MULTIPASS_LQ
    q = _residues(rng, lq)
    shapes_ = [(60, 16), (60, 15), (57, 16), (48, 7), (33, 16), (31, 2), (20, 1), (17, 16), (9, 3), (5, 16), (3, 16), (60, 16)]
    batches, gapped = [], []
    for b, (max_len, vs) in enumerate(shapes_):
        lanes = []
        for l in range(vs):
            n = max_len if l == 0 else int(rng.integers(1, max_len + 1))
            kind = (b + l) % 3
            if kind == 0 or n < 12:            # a plain relative: the stretch lies across a pass boundary, or at the query's end
                edge = (MULTIPASS_BOUNDARIES + (lq,))[(b + l) % (len(MULTIPASS_BOUNDARIES) + 1)]
                a = min(max(0, edge - int(rng.integers(1, n + 1))), lq - n)
                s = q[a:a + n].copy()
                if n >= 20 and l % 4 == 2:
                    s[n // 2] = 1 + s[n // 2] % 30      # one substitution
            elif kind == 1:                    # an insertion of one residue in the middle: n - 1 query columns, n rows
                edge = MULTIPASS_BOUNDARIES[(b + l) % len(MULTIPASS_BOUNDARIES)]
                a = min(max(0, edge - n // 2), lq - n)
                h = (n - 1) // 2
                s = np.concatenate([q[a:a + h], _residues(rng, 1), q[a + h:a + n - 1]])
                gapped.append((b, l))
            else:                              # a deletion of one query column in the middle
                a = int(rng.integers(0, lq - n - 1))
                h = n // 2
                s = np.concatenate([q[a:a + h], q[a + h + 1:a + n + 1]])
                gapped.append((b, l))
            assert len(s) == n
            lanes.append(s.astype(np.int8))
        batches.append((_batch(lanes, max_len, vs), vs))
    c = _case("multipass", q, hot_table(), HOT_GAPS, batches)
    c["gapped"] = gapped
    return c


STAGING_LONG = (60000, 60000, 59999, 59999, 59998, 60000, 59997, 59999, 60000, 59996)   # handed over unsorted, with ties


@functools.lru_cache(maxsize=None)
def staging():
    """-> the case, with "planted": [(batch, lane, first row, rows)] of the copies in the long lanes."""
    rng = np.random.default_rng(0xB164)
    q = _residues(rng, 32)
    batches, planted = [], []
    for b, max_len in enumerate(STAGING_LONG):
        a = _batch([_residues(rng, max_len), _residues(rng, max_len)], max_len, 2)
        for l in range(2):
            n = (20 + b % 5) if l == 0 else (12 + b % 4)
            row = (0, (max_len - n) // 2, max_len - n)[(b + l) % 3]     # the first rows, the middle, the last rows
            a[row:row + n, l] = q[3 * l:3 * l + n]
            planted.append((b, l, row, n))
        batches.append((a, 2))
    batches += _copy_batches(q, shapes()[::-1][:30])
    c = _case("staging", q, hot_table(), HOT_GAPS, batches)
    c["planted"] = planted
    return c


@functools.lru_cache(maxsize=None)
def mixed():
    rng = np.random.default_rng(0xB165)
    amino = np.array([ord(ch) - 64 for ch in "ACDEFGHIKLMNPQRSTVWY"], dtype=np.int8)
    q = amino[rng.integers(0, 20, size=300)]
    batches = []
    for b, vs in enumerate([16, 0, 7, 1, 13, 2, 16, 3, 15, 4, 5, 6, 8, 9, 10, 11, 12, 14, 16, 1]):
        max_len = int(rng.integers(1, 121))
        lanes = []
        for l in range(vs):
            n = max_len if l == 0 else int(rng.integers(0, max_len + 1))
            s = amino[rng.integers(0, 20, size=n)]
            if n >= 30 and l % 3 == 1:         # a relative of a query stretch
                a = int(rng.integers(0, 300 - n))
                keep = rng.random(n) < 0.7
                s = np.where(keep, q[a:a + n], s).astype(np.int8)
            lanes.append(s)
        batches.append((_batch(lanes, max_len, vs), vs))
    return _case("mixed", q, b62_table(), B62_GAPS, batches)
