"""Shared by the tests of the row half of the bounds and stats kernels' packed positions (swg_bounds.hip):
named cases generated from seeds, no fixtures.  The kernels keep every position as row << 12 | column in one 32-bit
register, so a row at or above 2^19 sets the register's sign bit; every case here puts rows there.  A case is

    name, sub (int8[32, 32]), gap_open, gap_extend, queries (table indices), seqs (table indices),
    hits (per query, the sequences it is aligned with, in order), and what it claims (`rows` and the keys beside it)

Queries hold residues 1..20 and the table is a match/mismatch one, so a sequence of JUNK (a residue no query holds) with
pieces of a query planted at chosen rows scores exactly where the pieces lie.  test_long_rows_cases_host.py proves every
claim with the oracle; test_gpu_long_rows.py runs the cases on the device."""
import functools

import numpy as np

from hsps_cases import simple_table

HALF = 1 << 19      # the first row whose packed position has bit 31 set
LIMIT = 1 << 20     # the value of SWG_BOUNDS_LEN (swg_host_internal.h): the first sequence length the kernels do not take
GEOMETRIES = [(16, 4), (16, 8), (32, 8), (64, 8), (64, 16)]   # (G, K) of the kernels' instantiations, narrowest first
SMALLEST_LQ = {(16, 4): 60, (16, 8): 65, (32, 8): 129, (64, 8): 257, (64, 16): 513}   # the shortest query that selects each
JUNK = 21           # in no query: -2 against every column
GAPS = (-4, -1)


def geometry_of(lq):
    """The first instantiation whose G * K columns hold the query; None past the widest."""
    return next(((G, K) for G, K in GEOMETRIES if lq <= G * K), None)


def query_of(lq):
    return np.random.default_rng(0x10A6 + lq).integers(1, 21, lq).astype(np.int8)


def junk(n):
    return np.full(n, JUNK, dtype=np.int8)


def planted(total, pieces):
    """A sequence of `total` JUNK residues with pieces = [(first row, residues)] written over it (rows from 0)."""
    s = junk(total)
    for row, piece in pieces:
        assert 0 <= row and row + len(piece) <= total
        s[row:row + len(piece)] = piece
    return s


def _case(name, sub, gaps, queries, seqs, hits=None, **claims):
    queries = [np.ascontiguousarray(q, dtype=np.int8) for q in queries]
    seqs = [np.ascontiguousarray(s, dtype=np.int8) for s in seqs]
    hits = hits if hits is not None else [list(range(len(seqs))) for _ in queries]
    return dict(claims, name=name, sub=np.ascontiguousarray(sub, dtype=np.int8), gap_open=int(gaps[0]), gap_extend=int(gaps[1]),
                queries=queries, seqs=seqs, hits=hits, geometries=[geometry_of(len(q)) for q in queries])


def high_copy(q):
    """The query with one residue deleted and one substituted: the copy's alignment has a gap and a mismatch, and each of
    its three stretches scores more than the step between them costs."""
    lq = len(q)
    copy = q.copy()
    copy[2 * lq // 3] = q[2 * lq // 3] % 20 + 1             # another of the residues 1..20
    return np.delete(copy, lq // 3)


def high_case(G, K):
    """The best cell and its origin both lie above row 2^19 (bpos and borg have bit 31 set); a lower-scoring decoy, the
    query's first half near row 100, is the best cell for the first 2^19 rows."""
    lq = SMALLEST_LQ[(G, K)]
    q = query_of(lq)
    decoy, copy = (100, q[:lq // 2]), (HALF + 200, high_copy(q))
    return _case("high_%dx%d" % (G, K), simple_table(3, -2), GAPS, [q], [planted(HALF + 300 + lq, [decoy, copy])],
                 rows="high", decoy=decoy, copy=copy)


def straddle_case():
    """A copy of the query across row 2^19: the origin has bit 31 clear and the best cell has it set."""
    q = query_of(SMALLEST_LQ[(16, 8)])
    copy = (HALF - 30, q)
    return _case("straddle", simple_table(3, -2), GAPS, [q], [planted(HALF + 300, [copy])], rows="straddle", copy=copy)


TIE_STRETCH = 12


def tie_case(G, K):
    """Two different stretches of the query, equally long, one below row 2^19 and one above; they end in columns of
    different lanes, so the cross-lane reduction decides, and its rule -- the smallest database position -- must pick the
    low one.  The low one has the higher column: a rule that looked at the column first would pick the other."""
    lq = SMALLEST_LQ[(G, K)]
    q = query_of(lq)
    a, b = 2 * lq // 3, lq // 6
    low, high = (1000, q[a:a + TIE_STRETCH]), (HALF + 1000, q[b:b + TIE_STRETCH])
    return _case("tie_across_sign_%dx%d" % (G, K), simple_table(3, -2), GAPS, [q], [planted(HALF + 2000, [low, high])],
                 rows="tie", low=low, high=high, low_columns=(a, a + TIE_STRETCH), high_columns=(b, b + TIE_STRETCH))


EVERY_ROW_LEN = HALF + 77
# (name, sub, gaps, score, n_ops): measured with the oracle; test_long_rows_cases_host.py restates them as asserts
EVERY_ROW_SCORINGS = [("every_row_path_gaps_2_1", np.full((32, 32), -100, dtype=np.int8), (2, 1), 524298, 524371),
                      ("every_row_path_gaps_0_1", simple_table(3, -2), (0, 1), 524381, 524365)]


def every_row_cases():
    """A positive gap_extend: one path runs in from the border through every row, so the step counter, the score and
    d_end all pass 2^19."""
    q = np.ones(8, dtype=np.int8)
    return [_case(name, sub, gaps, [q], [np.ones(EVERY_ROW_LEN, dtype=np.int8)], rows="every", score=score, n_ops=n_ops)
            for name, sub, gaps, score, n_ops in EVERY_ROW_SCORINGS]


def limit_case():
    """One sequence of SWG_BOUNDS_LEN - 1 residues (the kernel's longest) and one of SWG_BOUNDS_LEN (the fallback's
    first); in each the query is the last 8 rows, so the best cell is the last row and the last column, and a lower
    decoy lies near row 10."""
    q = query_of(8)
    seqs = [planted(n, [(10, q[:4]), (n - 8, q)]) for n in (LIMIT - 1, LIMIT)]
    return _case("limit", simple_table(3, -2), GAPS, [q], seqs, rows="limit", decoy=(10, q[:4]))


def after_a_long_pair_case():
    """high_16x4's pair, directly behind it (a launch takes its pairs longest first, equal lengths in the order given) a
    one-residue pair that scores above 0, then a pair that scores 0: no high bit of one job may reach the next.  Meant
    for one lane group (option bounds_groups = 1)."""
    h = high_case(16, 4)
    q = h["queries"][0]
    return _case("after_a_long_pair", h["sub"], GAPS, [q], [h["seqs"][0], q[17:18].copy(), junk(1)], rows="after")


@functools.lru_cache(maxsize=None)
def all_cases():
    return tuple([high_case(G, K) for G, K in GEOMETRIES] + [straddle_case()] +
                 [tie_case(G, K) for G, K in ((16, 4), (32, 8), (64, 16))] + every_row_cases() +
                 [limit_case(), after_a_long_pair_case()])


NAMES = (["high_%dx%d" % g for g in GEOMETRIES] + ["straddle"] + ["tie_across_sign_%dx%d" % g for g in ((16, 4), (32, 8), (64, 16))] +
         [s[0] for s in EVERY_ROW_SCORINGS] + ["limit", "after_a_long_pair"])


def case(name):
    return next(c for c in all_cases() if c["name"] == name)


def packed(c):
    """The case's sequences as one database: (flat int8, offsets uint64)."""
    flat = np.ascontiguousarray(np.concatenate(c["seqs"]), dtype=np.int8)
    off = np.zeros(len(c["seqs"]) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in c["seqs"]])
    return flat, off


def pssm_of(c, i=0):
    """The PSSM whose rows are the table's rows of query i: it must give the index query's answers."""
    return np.ascontiguousarray(c["sub"][c["queries"][i].astype(np.int64)], dtype=np.int8)


def counts_of(q, d, q_begin, d_begin, ops):
    """(n_ident, n_match, n_gap_open, n_gap) of a spelled path (test_gpu_stats.counts_of, restated where a test without
    a GPU can import it)."""
    qi, di, ident, opens, prev = q_begin, d_begin, 0, 0, ""
    for o in ops:
        if o == "M":
            ident += int(q[qi] == d[di])
            qi, di = qi + 1, di + 1
        elif o == "I":
            di += 1
        else:
            qi += 1
        opens += o != "M" and o != prev
        prev = o
    n_match = ops.count("M")
    return ident, n_match, opens, len(ops) - n_match


# ---- the best-cell reduction of the kernels, restated: what a signed compare would do to the tie cases ------------------
def best_cell(candidates, signed):
    """candidates: (score, row, column), rows and columns from 1, one per lane -> the winner of the kernels' rule `higher
    score, else smaller packed position`, with the packed words compared as uint32 (signed=False, the kernels) or as
    int32 (signed=True, the fault the tie cases are aimed at)."""
    def word(row, col):
        w = (row << 12 | col) & 0xFFFFFFFF
        return w - (1 << 32) if signed and w >> 31 else w
    best = candidates[0]
    for c in candidates[1:]:
        if c[0] > best[0] or (c[0] == best[0] and word(c[1], c[2]) < word(best[1], best[2])):
            best = c
    return best
