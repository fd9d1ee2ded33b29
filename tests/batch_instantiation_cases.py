"""The matrix of the BATCH instantiations of the lane-group fill and its inputs (plain module, no tests of its own).

tests/instantiation_cases.py forces every instantiation a single search can force.  The kernels behind swg_search_multi
and swg_search_lists are compiled once per entry of SWG_DIAG_VARIANTS too -- swg_diag_qq_kernel<K, MAXW> with CellsQQ<K>
(two queries per lane), swg_diag_dyn_kernel with n_queries > 1, and its LISTS instantiations on both cell forms -- and a
batch reaches them only through plan_batch / plan_lists, which option batch_geometry = 1 lets take cols_per_wave and
group_lanes.  CASES forces every (family, K, lanes) below on instantiation_cases' database (151 sequences of at most 300
rows: under BLOSUM62 no score bound reaches the f16 cells' 4096, so the cells are the options' choice), all in one pass:

  qq           two queries per lane: every K at 16 and at 32 lanes, and at 64 lanes every K whose pair profile fits LDS
               (the planner hook decides which: tests/test_batch_instantiation_cases_host.py)
  qq_fallback  the K at 64 lanes whose pair profile does not fit: the batch must run the perm pairing (cell_form 2)
  batch_f16    option qq = 0: two sequences per lane on the f16 cells, every K at the width rot(K)
  batch_i16    option f16 = 0: the same on the packed int16 cells
  lists_f16 / lists_i16   swg_search_lists on either cell form, every K at rot(K)

Every case's batch has five queries (queries(case)); lq_max = G * K minus the last lane's cut (single_lq), so the group's
last lane is partly filled:

  0  QUERY[:lq_max]
  1  QUERY[SHIFT:SHIFT + n], n = second_length(K, G): shorter, no multiple of K (it ends inside a lane), the second
     longest of the batch -- the qq path sorts by length and pairs neighbours, so it is the other half of the first pair
  2  one residue (the odd batch's last pair: paired with itself)
  3, 4  unrelated random residues of two different lengths below n (the second pair, of unequal lengths)

Query 1 is short on purpose: a window of QUERY scores what the prefix scores wherever the best alignment lies inside it, and
the database's planted copies (SWEEP) lie in the first 44 columns for both.  With n about a fifth of lq_max the two halves
of the first pair disagree on most sequences (the host test asserts the share from the oracle alone), so a kernel that
swapped or merged the halves is caught, while the copies still pin every lane-local column of both halves.

Lists (lists(case)): query 0 takes the whole database, query 1 the pinning sequences and a random subset (odd length),
query 2 a single sequence, query 3 the empty list, query 4 the pinning sequences and another subset.
"""
import functools

import numpy as np

import instantiation_cases as ic

KS = ic.KS
WIDTHS = ic.WIDTHS
SCORING = "b62"
GAPS = ic.GAPS[SCORING]
SHIFT = 1                  # query 1 starts at this column of QUERY: its lane-local columns are the prefix's, shifted
N_QUERIES = 5
FAMILIES = ("qq", "qq_fallback", "batch_f16", "batch_i16", "lists_f16", "lists_i16")
# what each family sets beside engine = 2, batch_geometry = 1, cols_per_wave and group_lanes
OPTIONS = {"qq": {"f16": 2, "qq": 1}, "qq_fallback": {"f16": 2, "qq": 1}, "batch_f16": {"f16": 2, "qq": 0},
           "batch_i16": {"f16": 0, "qq": 1}, "lists_f16": {"f16": 2}, "lists_i16": {"f16": 0}}
QQ_LDS_MAX_K_AT_64 = 18    # (documentation: the hook decides, the host test compares)


def second_length(K, G):
    """Columns of query 1: about a fifth of lq_max, at least the SWEEP ends that pin K consecutive columns of it
    (ends SWEEP[0] .. SWEEP[0] + K - 1 of QUERY, i.e. up to column SWEEP[0] + K - 1 - SHIFT of the window) and one
    more, below lq_max, no multiple of K."""
    lq = ic.single_lq(K, G)
    n = max(lq // 5, ic.SWEEP[0] + K - SHIFT + 1)
    if n % K == 0:
        n += 1
    assert n < lq and n % K != 0, (K, G, n, lq)
    return n


def qq_fits(K, G):
    """Whether the query pairs' profile (128 bytes per column, K padded to even) and the lane-group records of the
    smallest workgroup fit LDS: what the matrix was written for; the planner hook has the last word (host test)."""
    return G < 64 or K <= QQ_LDS_MAX_K_AT_64


def _case(family, K, G):
    form = 0 if family.endswith("i16") else 2
    qq = family == "qq"
    c = dict(family=family, K=K, G=G, lq=ic.single_lq(K, G), n2=second_length(K, G), form=form, qq=qq,
             lists=family.startswith("lists"), options=dict(OPTIONS[family]), scoring=SCORING, gaps=GAPS,
             launcher="qq" if qq else "lists" if family.startswith("lists") else "dyn", cell_form=3 if qq else form)
    c["id"] = "%s-K%d-G%d-lq%d" % (family, K, G, c["lq"])
    return c


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for K in KS:
        for G in WIDTHS:
            out.append(_case("qq" if qq_fits(K, G) else "qq_fallback", K, G))
        for fam in ("batch_f16", "batch_i16", "lists_f16", "lists_i16"):
            out.append(_case(fam, K, ic.rot(K)))
    ids = [c["id"] for c in out]
    assert len(set(ids)) == len(ids)
    return tuple(out)


def required(ks):
    """Every (family, K, lanes) the matrix must hold for the K of the source's macro."""
    need = set()
    for K in ks:
        need |= {("qq" if qq_fits(K, G) else "qq_fallback", K, G) for G in WIDTHS}
        need |= {(fam, K, ic.rot(K)) for fam in ("batch_f16", "batch_i16", "lists_f16", "lists_i16")}
    return need


def held():
    return {(c["family"], c["K"], c["G"]) for c in cases()}


def groups():
    """(family, lanes) -> the cases of one GPU test item, in matrix order."""
    g = {}
    for c in cases():
        g.setdefault((c["family"], c["G"]), []).append(c)
    return g


# ---- inputs -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _queries(K, G):
    q = ic.query()
    lq, n = ic.single_lq(K, G), second_length(K, G)
    rng = np.random.default_rng(0xBA7C + 64 * K + G)
    a, b = max(2, n - 3), max(1, n // 2)               # two different lengths below n
    if a == b:
        b -= 1
    assert 1 <= b < a < n < lq
    qs = [q[:lq], q[SHIFT:SHIFT + n], q[7:8], rng.integers(1, 32, size=a).astype(np.int8), rng.integers(1, 32, size=b).astype(np.int8)]
    qs = tuple(np.ascontiguousarray(x) for x in qs)
    for x in qs:
        x.setflags(write=False)
    assert len(qs) == N_QUERIES and N_QUERIES % 2 == 1
    return qs


def queries(case):
    return _queries(case["K"], case["G"])


def pairs_of(case):
    """The qq path's pairs as query indices: sorted by length, longest first (stable), neighbours paired, the odd batch's
    last query with itself."""
    qs = queries(case)
    order = sorted(range(len(qs)), key=lambda i: -len(qs[i]))
    order.append(order[-1])
    return [(order[i], order[i + 1]) for i in range(0, len(qs), 2)]


@functools.lru_cache(maxsize=None)
def sweep_indices():
    """Original indices of the sequences that pin the lane-local columns: the 12-column copies whose ends sweep SWEEP."""
    flat, off = ic.database()
    q = ic.query()
    want = {q[e - 11:e + 1].tobytes() for e in range(*ic.SWEEP)}
    ix = [i for i in range(ic.DB_COUNT) if flat[int(off[i]):int(off[i + 1])].tobytes() in want]
    assert len(ix) == ic.SWEEP[1] - ic.SWEEP[0]
    return tuple(ix)


@functools.lru_cache(maxsize=None)
def _lists(K, G):
    rng = np.random.default_rng(0x1157 + 64 * K + G)
    pins = np.asarray(sweep_indices(), dtype=np.int64)
    rest = np.setdiff1d(np.arange(ic.DB_COUNT), pins)

    def some(n):
        return rng.permutation(np.concatenate([pins, rng.choice(rest, size=n, replace=False)]))
    odd = some(21 + 2 * (K % 5))                           # 32 pins + an odd count: an odd list, its last pair has one member
    single = rest[rng.integers(0, len(rest), size=1)]
    out = (np.arange(ic.DB_COUNT), odd, single, np.zeros(0, dtype=np.int64), some(10 + 2 * (K % 7)))
    assert len(out[1]) % 2 == 1 and len(out[2]) == 1 and len(out[3]) == 0 and len(out) == N_QUERIES
    for x in out:
        x.setflags(write=False)
    return out


def lists(case):
    """One candidate list per query (original indices), or None for the families that search the whole database."""
    return _lists(case["K"], case["G"]) if case["lists"] else None


@functools.lru_cache(maxsize=None)
def _truth(K, G):
    import swg_loader
    orc, swg = swg_loader.oracle(), swg_loader.load()
    flat, off = ic.database()
    sub = ic.table(swg, SCORING)
    qs = _queries(K, G)
    rows = [ic._truth(len(qs[0]), SCORING, GAPS[0], GAPS[1], False)]
    rows += [orc.score_db(x, flat, off, sub, *GAPS) for x in qs[1:]]
    t = np.stack(rows).astype(np.int32)
    t.setflags(write=False)
    return t


def truth(case):
    """int32 [N_QUERIES, DB_COUNT]: the oracle's scores of every query of the case's batch against the whole database
    (computed once per geometry, shared by the families, read-only)."""
    return _truth(case["K"], case["G"])


def query_column_best(case, i):
    """instantiation_cases.column_best for query i (0 or 1) of the case's batch."""
    if i == 0:
        return ic.column_best(SCORING, *GAPS)[:, :case["lq"]]
    return ic.column_best(SCORING, *GAPS, ic.query_key(queries(case)[i]))


def pinned_columns(case, i, among=None):
    """The lane-local columns k of query i a wrong cell of which changes a reported score: those that hold every best
    cell of some sequence (of the list `among`, original indices; default: the whole database)."""
    best = query_column_best(case, i)
    cls = np.arange(best.shape[1]) % case["K"]             # one pass: column c is lane c // K's column c % K
    t = best.max(axis=1)
    ok = t > 0
    if among is not None:
        sel = np.zeros(ic.DB_COUNT, dtype=bool)
        sel[np.asarray(among, dtype=np.int64)] = True
        ok &= sel
    at = best == t[:, None]
    lo, hi = np.where(at, cls, 1 << 20).min(axis=1), np.where(at, cls, -1).max(axis=1)
    return set(lo[ok & (lo == hi)].tolist())


def expected_launches(case, W=None):
    """The launch log of a case, as (family, K, lanes, form, edges, fma, list, grid rows): one launch, of the batch's own
    launcher -- a record of another family, or a second one, means the batch fell back to single searches."""
    if case["launcher"] == "qq":
        return [("qq", case["K"], case["G"], 2, 0, 0, 0, (N_QUERIES + 1) // 2)]
    if case["launcher"] == "lists":
        return [("lists", case["K"], case["G"], case["form"], 0, 0, 1, 1)]
    return [("dyn", case["K"], case["G"], case["form"], 0, 0, 0, N_QUERIES)]
