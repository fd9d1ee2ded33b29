"""Shared inputs of the swg_search_above_multi tests (plain module, no tests of its own).

Database A of tests/test_gpu_prune.py -- 4 000 short sequences, 1 % of them near-copies of the 200-column query qA,
BLOSUM62, gaps -2/-1 -- and a batch of FIVE queries: an odd count, so that the last query of a two-per-lane chunk is
paired with itself.  Each query has five threshold levels taken from its own oracle scores (LEVELS).
tests/test_above_multi_cases_host.py proves on the CPU what the GPU tests rely on."""
import numpy as np

N = 4000
GO, GE = -2, -1
LEVELS = ("above_best", "best", "tenth", "median", "one")


def table(swg):
    return np.asarray(swg.load_scoring("BLOSUM62").table(), dtype=np.int8).reshape(32, 32)


def database(swg):
    """-> (flat, off, qA): database A and the query its near-copies were made from."""
    qA = swg.synth_query(0x5EED0A01, 200)
    flat, off = swg.synth_db(0x5EED0A02, N, median=60, max_len=600, query=qA, fraction=0.01, subst=0.05)[:2]
    return flat, off, qA


def queries(swg, qA):
    return [qA, qA[60:141].copy(), qA[:1].copy(), swg.synth_query(0x5EED0C11, 77), swg.synth_query(0x5EED0C12, 150)]


def pssms(sub, qs):
    """The same queries as position-specific ones: row p of query i is the table's row of its residue."""
    return [np.ascontiguousarray(np.asarray(sub)[np.asarray(q, dtype=np.int64)], dtype=np.int8) for q in qs]


def thresholds(truth, members=None):
    """One score per level of LEVELS: above the best (no hit), the best, the 10th best (its ties come along), the median, 1."""
    s = np.sort(np.asarray(truth) if members is None else np.asarray(truth)[np.asarray(members, dtype=np.int64)])
    return [int(s[-1]) + 1, max(1, int(s[-1])), max(1, int(s[-10])), max(1, int(s[len(s) // 2])), 1]


def above(truth, T, members=None):
    """The oracle's answer: the members that score at least T, higher score first, ties by lower index."""
    members = np.arange(len(truth)) if members is None else np.asarray(members, dtype=np.int64)
    sel = members[np.asarray(truth)[members] >= T]
    order = np.lexsort((sel, -np.asarray(truth, dtype=np.int64)[sel]))
    return [(int(truth[i]), int(i)) for i in sel[order]]


def level_table(truths, members=None):
    """T[i][l]: the threshold of query i at level l."""
    return [thresholds(t, members) for t in truths]


def mixed(T):
    """One call in which query i takes level i (five queries, five levels)."""
    return [T[i][i % len(LEVELS)] for i in range(len(T))]


def pair_order_bounds(swg, sub, q, flat, off, order):
    """The colmax bound of every pair of the fill (slots 2p and 2p + 1 of the database's order): max(U_x, U_y)."""
    _, u = swg.debug_prune_bound(sub, q, flat, off)
    u = u.astype(np.int64)
    order = np.asarray(order, dtype=np.int64)
    return np.maximum(u[order[0::2]], u[order[1::2]])


def sorted_order(off):
    """The database's order without a device: by length, longest first, ties by index (what db.order() gives)."""
    lens = np.diff(np.asarray(off).astype(np.int64))
    return np.lexsort((np.arange(len(lens)), -lens))
