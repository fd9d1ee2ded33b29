"""Shared builder of edge scorings and databases (plain module, no tests of its own).

The kernels are specialised by the scoring parameters: the gap magnitudes g = -(gap_open + gap_extend) and
e = -gap_extend choose the cells (packed f16 iff g, e <= 2048; 16-bit iff both scores <= 0 and g <= 32767; else
int32), and the table entries are int8.  This module builds the tables at the ends of int8 and databases on which
a LARGE gap magnitude is observable: a gap only shows if some alignment scores more with it than without, which
needs both flanks to score more than g.

split_db: the query is A + B, two random flanks of F residues; with the table `diag127` (127 on the diagonal,
-128 .. -100 elsewhere) a copy scores 254 F, either flank alone 127 F, and a relative with one indel between the
flanks about 254 F - g.  F = g // 127 + 4 (at least 8): an insertion of k residues pays when 127 F > g + (k-1) e,
a deletion of k query residues only when 127 (F - k) > g + (k-1) e -- with F = g // 127 + 1 no deletion could ever
pay (127 (F - 1) <= g), so no best path would hold a 'D'; three residues more let deletions of one and two pay for
every e <= 127, and single ones for any e.  One construction then straddles every ceiling:
  g = 2048:  F = 20,  copy 5080,   gapped 3032   (either side of the f16 cells' 4096)
  g = 16000: F = 129, copy 32766,  gapped 16766  (everything just below int16's 32767)
  g = 32767: F = 262, copy 66548,  gapped 33781  (beyond the wide form's 65535, and inside it; on the plain int16
                                                  cells no gap pays below 32767: a saturation test only)
  g = 65536: F = 520, copy 132080, gapped 66544  (int32 only)
"""
import numpy as np

# ---- gap points: (gap_open, gap_extend) and the route each must take ---------------------------------------------
# path_bits: swg_stats.path_bits of a search left to the library; f16: whether option f16 = 2 gets the f16 cells
# (cell_form 2) -- above 2048 it must not, even when asked.
GAP_POINTS = [
    # g = 2047, 2048: the last magnitudes of the f16 cells
    dict(go=-2046, ge=-1, bits=16, f16=True),
    dict(go=-2047, ge=-1, bits=16, f16=True),
    dict(go=0, ge=-2048, bits=16, f16=True),
    dict(go=-1024, ge=-1024, bits=16, f16=True),
    # g = 2049: int16 cells even with f16 = 2
    dict(go=-2048, ge=-1, bits=16, f16=False),
    dict(go=0, ge=-2049, bits=16, f16=False),
    dict(go=-15999, ge=-1, bits=16, f16=False),
    dict(go=0, ge=-16000, bits=16, f16=False),
    # g = 32767: the last magnitude of the 16-bit cells
    dict(go=-32766, ge=-1, bits=16, f16=False),
    dict(go=0, ge=-32767, bits=16, f16=False),
    dict(go=-32767, ge=0, bits=16, f16=False),
    # g = 32768, 65536: int32
    dict(go=-32767, ge=-1, bits=32, f16=False),
    dict(go=-32768, ge=0, bits=32, f16=False),
    dict(go=-32768, ge=-32768, bits=32, f16=False),
]
for _p in GAP_POINTS:
    _p["g"] = -(_p["go"] + _p["ge"])
    _p["e"] = -_p["ge"]


def point_id(p):
    return "go%d_ge%d" % (p["go"], p["ge"])


def gap_point(go, ge):
    return next(p for p in GAP_POINTS if (p["go"], p["ge"]) == (go, ge))


# ---- tables ------------------------------------------------------------------------------------------------------
def diag127(rng=None, zero0=False):
    """127 on the diagonal, every other entry drawn from -128 .. -100, one -128 and one 126 placed explicitly.
    zero0: row and column 0 zero (index 0 is no residue; the golden fixtures want it so)."""
    rng = rng or np.random.default_rng(127)
    sub = rng.integers(-128, -99, size=(32, 32)).astype(np.int8)
    sub[np.arange(32), np.arange(32)] = 127
    sub[3, 7] = -128
    sub[7, 3] = 126          # (asymmetric on purpose: a kernel that transposes the table shows)
    if zero0:
        sub[0, :] = 0
        sub[:, 0] = 0
    return sub


def full_range(rng=None):
    """Every entry uniform in -128 .. 127, rows and columns 0 included; both ends present."""
    rng = rng or np.random.default_rng(128)
    sub = rng.integers(-128, 128, size=(32, 32)).astype(np.int8)
    sub[5, 9], sub[9, 5] = -128, 127
    return sub


def all_127():
    return np.full((32, 32), 127, dtype=np.int8)


def all_m128():
    return np.full((32, 32), -128, dtype=np.int8)


def blosum62_dirty0(b62, rng=None):
    """BLOSUM62 with random bytes in row and column 0: scores must equal plain BLOSUM62's."""
    rng = rng or np.random.default_rng(62)
    sub = np.array(b62, dtype=np.int8).reshape(32, 32).copy()
    sub[0, :] = rng.integers(-128, 128, size=32)
    sub[:, 0] = rng.integers(-128, 128, size=32)
    return sub


TABLES = ("diag127", "full_range", "all_127", "all_m128", "blosum62_dirty0")


def table(name, b62=None):
    if name == "blosum62_dirty0":
        return blosum62_dirty0(b62)
    return {"diag127": diag127, "full_range": full_range, "all_127": all_127, "all_m128": all_m128}[name]()


# ---- databases ---------------------------------------------------------------------------------------------------
def flank_len(g):
    return max(8, g // 127 + 4)


def _res(rng, n, hi):
    return rng.integers(1, hi + 1, size=int(n)).astype(np.int8)


def split_query(g, rng, hi=31):
    """-> (query A + B, F)."""
    F = flank_len(g)
    return np.concatenate([_res(rng, F, hi), _res(rng, F, hi)]), F


KINDS = ("copy", "insert", "delete", "junk", "decoy", "skip3")


def split_db(g, n, rng, hi=31, query=None, long_decoys=0):
    """-> (query, flat, offsets, kinds): n sequences (made odd) of the six kinds, cycled, with seeded variations;
    lengths 1 and 2 always present (the last two decoys).  kinds[i] indexes KINDS.  long_decoys: that many of the
    decoys are longer than every relative instead (3F + 4 .. 5F + 4 residues, at least 70: a class of long pairs for
    option long_split to cut off)."""
    if query is None:
        query, F = split_query(g, rng, hi)
    else:
        F = len(query) // 2
    A, B = query[:F], query[F:]
    n = int(n) | 1
    seqs, kinds = [], []
    for i in range(n):
        k = i % 6
        if k == 0:
            s = query.copy()
        elif k == 1:      # A + insert(1..3) + B: an 'I' in the best path where it pays
            s = np.concatenate([A, _res(rng, rng.choice([1, 1, 2, 3]), hi), B])
        elif k == 2:      # A minus its last 1..2 residues + B: a 'D'
            s = np.concatenate([A[:F - int(rng.choice([1, 1, 2]))], B])
        elif k == 3:      # junk prefix + A + junk + B cut short
            s = np.concatenate([_res(rng, rng.integers(1, F + 1), hi), A, _res(rng, rng.integers(1, 4), hi),
                                B[:F - int(rng.integers(1, F // 2 + 1))]])
        elif k == 4:      # a random decoy of 1 .. 2F residues
            s = _res(rng, rng.integers(1, 2 * F + 1), hi)
        else:
            s = np.concatenate([A, B[3:]])
        seqs.append(s.astype(np.int8))
        kinds.append(k)
    # lengths 1 and 2: the last two decoys; the long ones: the first
    dec = [i for i in range(n) if kinds[i] == 4]
    assert len(dec) >= 2 + long_decoys
    seqs[dec[-1]] = _res(rng, 1, hi)
    seqs[dec[-2]] = _res(rng, 2, hi)
    for i in dec[:long_decoys]:
        seqs[i] = _res(rng, rng.integers(max(70, 3 * F + 4), max(70, 5 * F + 4) + 1), hi)
    flat = np.concatenate(seqs)
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return query, flat, off, np.array(kinds, dtype=np.int32)


# sequences of the database the searches run on, at every gap point: several workgroups, queue shards, both pair classes
SEARCH_DB_SIZE = 3000


def seqs_of(flat, off):
    return [flat[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]


def gapped_relatives(orc, query, flat, off, kinds, sub, go, ge, first=48):
    """The self-check, from the oracle alone: of the relatives of kinds "insert" and "delete" among the first
    `first` sequences, how many have an oracle path that contains I or D AND an oracle score above 127 F (what a
    flank scores on its own) -> (count, with_I, with_D)."""
    F = len(query) // 2
    n = n_i = n_d = 0
    for i in range(min(first, len(kinds))):
        if kinds[i] not in (1, 2):
            continue
        sc, _, ops = orc.pair_trace(query, flat[int(off[i]):int(off[i + 1])], sub, go, ge)
        if sc > 127 * F and ("I" in ops or "D" in ops):
            n += 1
            n_i += "I" in ops
            n_d += "D" in ops
    return n, n_i, n_d


def payable(p, ceiling):
    """Whether a gap can pay below `ceiling` at this point: the gapped relative scores 254 F - g."""
    return 254 * flank_len(p["g"]) - p["g"] < ceiling


def random_db(rng, n, lo, hi_len, hi=31):
    """n random sequences of lo .. hi_len residues; with lo = 1 lengths 1 and 2 are always present."""
    lens = rng.integers(lo, hi_len + 1, size=n)
    if lo == 1 and n > 2:
        lens[n // 2], lens[n // 3] = 1, 2
    flat = _res(rng, int(lens.sum()), hi)
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens)
    return flat, off
