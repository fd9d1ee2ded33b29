"""The matrix of lane-group fill instantiations and its inputs (plain module, no tests of its own).

The lane-group kernels are compiled once per entry of SWG_DIAG_VARIANTS (columns per lane K = 2 .. 32) and per family:
int16 cells (single pass, one pass of several, the wide form), packed-f16 cells (single pass and one pass of several,
each with the v_perm_b32 and the v_pk_fma_f16 pairing), the gapless cells, the int32 cells (reduced and exact, each with
and without edges).  Every one of them has code of its own per K -- the partly used last profile chunk, the odd-K arm of
the running best, the fma pairing's 2-column chunks, the fence schedule, the register budget -- and the planner may pick
any K for a user's query length.  CASES forces every (family, K) a single search can force, on one small database, and
says what must run: tests/test_instantiation_cases_host.py proves on the CPU that the planner answers every case as
intended and that the inputs have the properties the cases rely on; tests/test_gpu_instantiations.py runs them.

Inputs: QUERY (every case searches a prefix of it) and one database of DB_COUNT sequences -- lengths 1 .. 9 (every
remainder of the residue dwords and the 4-row blocks), an empty record, an odd count (the last pair has one member),
relatives of query stretches planted at many offsets and lengths, short exact copies whose ends sweep consecutive query
columns (SWEEP for every case's first pass, RUNS for a last pass on a K of its own: with them every lane-local column of
every case holds all the best cells of some sequence, pinned_classes), the rest random up to MAX_LEN residues.  Two scorings:
"b62" = BLOSUM62 with (-11, -1), and "hot" = scoring_edges.diag127 with (-60, -20): 33 matching residues reach the f16
cells' 4096, 258 the int16 cells' 32767, so queries of 40 columns flag and queries of 265 need the wide form.  (A gap's
first position costs 80, less than one match: gaps pay in the planted relatives, while unrelated sequences stay in the
hundreds -- with gaps of a few units they would chain their chance matches and nearly all of them flag.)

Query length of a case: G * K * (passes - 1) + r, with r no multiple of K (the group's last lane is partly filled) and,
for several passes, small enough that the last pass takes a K of its own (swg_plan_last_pass) where one exists.
"""
import functools
import os
import re

import numpy as np

import scoring_edges as se

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = os.path.join(ROOT, "seq-align-gpu_amd", "csrc", "swg_kernels.hip")

QLEN = 2200
DB_COUNT = 151
MAX_LEN = 300
F16_CEILING, I16_CEILING, WIDE_CEILING = 4096, 32767, 65535
X32_MAX_K = 28                      # SWG_X32_MAX_K: the most columns per lane the exact int32 cells hold
LDS = 160 * 1024
GAPS = {"b62": (-11, -1), "hot": (-60, -20)}
WIDTHS = (16, 32, 64)
SWEEP = (12, 44)                    # ends of the 12-column copies: 32 consecutive columns, the first ones below every case's lq
# (first end, count) of the copies that pin a last pass's own columns, and the copies' lengths per run: every last pass of
# the matrix holds a run of at least as many consecutive ends as it has columns per lane, and no longer copy is whole
RUNS = ((100, 3), (200, 4), (296, 16), (450, 24), (516, 24), (900, 16), (1030, 4), (1100, 24))
RUN_MIN_LENGTH, RUN_MAX_LENGTH = 10, 32     # (32 matches stay below the f16 cells' 4096)
AMINO = tuple(ord(ch) - 64 for ch in "ACDEFGHIKLMNPQRSTVWY")
SEPARATOR = 8                       # residues after each copy that match nothing near its end: no alignment runs on past it


def variant_ks():
    """[(K, max_waves)] of the SWG_DIAG_VARIANTS macro (the one the library is built with), read from the source."""
    src = open(KERNELS).read()
    m = re.search(r"#else\s*\n#define SWG_DIAG_VARIANTS\(X\)((?:.*\\\n)*.*)\n", src)
    assert m, "SWG_DIAG_VARIANTS not found in swg_kernels.hip"
    ks = [(int(a), int(b)) for a, b in re.findall(r"X\((\d+),\s*(\d+)\)", m.group(1))]
    assert ks and len(set(k for k, _ in ks)) == len(ks)
    return ks


KS = tuple(range(2, 33))            # what this module was written for; the host test compares it with variant_ks()


# ---- inputs -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def query():
    q = np.random.default_rng(0x1257).integers(1, 32, size=QLEN).astype(np.int8)
    # where the planted copies end, every column holds one of the twenty amino acids: BLOSUM62 scores the other codes
    # with themselves at zero or below, and a copy that ends on one has no best cell in that column
    for a, b in (SWEEP,) + tuple((a - RUN_MAX_LENGTH - 4, a + n + 4) for a, n in RUNS):
        for c in range(a, b):
            if q[c] not in AMINO:
                q[c] = AMINO[c % len(AMINO)]
    q.setflags(write=False)
    return q


@functools.lru_cache(maxsize=None)
def database():
    """-> (flat int8, offsets uint64[DB_COUNT + 1])."""
    import swg_loader
    rng = np.random.default_rng(0x1258)
    q = query()
    junk = lambda n: rng.integers(1, 32, size=int(n)).astype(np.int8)
    seqs = []
    # lengths 1 .. 9 twice: stretches of the query's first 24 columns (every case's prefix holds them), and random ones
    for n in range(1, 10):
        a = (5 * n) % (24 - n)
        seqs.append(q[a:a + n].copy())
        seqs.append(junk(n))
    seqs.append(np.zeros(0, dtype=np.int8))                       # an empty record
    # exact copies: 36 columns (4572 under "hot": flagged by the f16 cells in every case of 40 columns or more), 34 and 32
    # (4318, 4064: either side of the flag), 270 (34290: beyond int16, inside the wide form)
    seqs += [q[:36].copy(), np.concatenate([junk(3), q[2:36]]), q[3:35].copy(), np.concatenate([junk(7), q[:270], junk(5)])]
    # what pins every lane-local column (pinned_classes): exact copies of 12 columns whose ends sweep SWEEP -- consecutive
    # columns inside every case's first pass, so every residue of (column mod K) has a sequence whose only best cell lies there
    for e in range(*SWEEP):
        seqs.append(q[e - 11:e + 1].copy())
    # ... and the same for a last pass on a K of its own, whose columns start wherever the passes before it end: sequence t
    # holds, for each run (start, count) with t < count, a copy that ends at column start + t, longer from run to run
    # and the later run first (so no two of them chain).  In a prefix the longest copy that is whole wins, so the RUN_COUNT
    # sequences' best cells are consecutive columns of the last run that the prefix holds -- which lies in the last pass
    b62 = np.asarray(table(swg_loader.load(), "b62"), dtype=np.int64)
    for t in range(max(n for _, n in RUNS)):
        mine, n, least = [], RUN_MIN_LENGTH - 2, 0
        for a, cnt in RUNS:
            if t < cnt:
                # each copy at least two columns longer than the one before (254 under the hot table) and at least 10 better
                # under BLOSUM62, whose scores depend on the residues
                e, n = a + t, n + 2
                while b62[q[e - n + 1:e + 1], q[e - n + 1:e + 1]].sum() < least:
                    n += 1
                assert n <= RUN_MAX_LENGTH, (t, a, n)
                least = b62[q[e - n + 1:e + 1], q[e - n + 1:e + 1]].sum() + 10
                mine.insert(0, (e, n))
        parts = []
        for i, (e, n) in enumerate(mine):
            # the separator: an amino acid that scores below zero against the column just after this copy and the one just before
            # the next one, and occurs nowhere near either (not C, which the hot table scores at 126 against G)
            after = q[e + 1:e + 13].astype(np.int64)
            before = q[mine[i + 1][0] - mine[i + 1][1] - 3:mine[i + 1][0] - mine[i + 1][1] + 1].astype(np.int64) if i + 1 < len(mine) else after[:0]
            near = np.concatenate([after, before])
            ok = [x for x in AMINO if x != 3 and x not in after and max(b62[after[:1], x].max(), b62[before[-1:], x].max(initial=-9)) < 0]
            x = min(ok, key=lambda x: (b62[near, x].max(), x))
            parts += [q[e - n + 1:e + 1], np.full(SEPARATOR, x, dtype=np.int8)]
        seqs.append(np.concatenate(parts))
    # relatives of query stretches at many offsets and lengths: substitutions, now and then an insertion or a deletion
    starts = np.concatenate([rng.integers(0, 200, size=12), rng.integers(0, QLEN - 150, size=44)])
    for i, a in enumerate(starts):
        n = int(rng.integers(20, 150))
        s = q[a:a + n].copy()
        hit = rng.random(n) < (0.0, 0.05, 0.12)[i % 3]
        s[hit] = junk(int(hit.sum()))
        if i % 4 == 1:
            cut = int(rng.integers(5, n - 5))
            s = np.concatenate([s[:cut], junk(rng.integers(1, 3)), s[cut:]])
        elif i % 4 == 3:
            cut = int(rng.integers(5, n - 5))
            s = np.concatenate([s[:cut], s[cut + 1:]])
        s = np.concatenate([junk(rng.integers(0, 40)), s, junk(rng.integers(0, 40))])
        seqs.append(s[:MAX_LEN].astype(np.int8))
    while len(seqs) < DB_COUNT:
        seqs.append(junk(rng.integers(10, MAX_LEN + 1)))
    assert len(seqs) == DB_COUNT and DB_COUNT % 2 == 1
    order = rng.permutation(DB_COUNT)
    seqs = [seqs[i] for i in order]
    flat = np.concatenate(seqs).astype(np.int8)
    off = np.zeros(DB_COUNT + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    flat.setflags(write=False)
    off.setflags(write=False)
    return flat, off


def table(swg, scoring):
    return swg.load_scoring("BLOSUM62").table() if scoring == "b62" else se.diag127(zero0=True)


@functools.lru_cache(maxsize=None)
def _truth(lq, scoring, go, ge, gapless):
    import gapless_cases as gc
    import swg_loader
    orc, swg = swg_loader.oracle(), swg_loader.load()
    flat, off = database()
    q = np.ascontiguousarray(query()[:lq])
    sub = table(swg, scoring)
    t = gc.oracle_gapless(orc, q, flat, off, sub) if gapless else orc.score_db(q, flat, off, sub, go, ge)
    t.setflags(write=False)
    return t


def truth(case):
    """The int32 oracle's scores of a case (computed once per prefix length, scoring and gaps; read-only)."""
    return _truth(case["lq"], case["scoring"], case["gaps"][0], case["gaps"][1], case["family"] == "gapless")


def query_key(q):
    """A query as column_best takes it: its bytes (hashable, so the result is computed once per query)."""
    return np.ascontiguousarray(q, dtype=np.int8).tobytes()


@functools.lru_cache(maxsize=None)
def column_best(scoring, go, ge, q=None):
    """int32 [DB_COUNT, columns]: the best match-state cell of every query column, per sequence, in plain numpy -- the
    oracle's three-state recurrence (oracle/sw_oracle.c), all sequences at once, one residue row at a time.  q: the query
    as query_key gives it, None for QUERY.  A cell depends on the columns to its left only, so the score against the
    prefix of lq columns is column_best[:, :lq].max(1): the host tests hold that against the oracle for every case, bit
    for bit."""
    import swg_loader
    flat, off = database()
    lens = np.diff(off).astype(np.int64)
    by_len = np.argsort(-lens, kind="stable")
    sub = np.asarray(table(swg_loader.load(), scoring), dtype=np.int32)
    qa = query() if q is None else np.frombuffer(q, dtype=np.int8)
    ncol = len(qa)
    prof = sub[qa.astype(np.int64)]                            # [columns, 32]
    res = np.zeros((DB_COUNT, int(lens.max())), dtype=np.int64)
    for n in range(DB_COUNT):
        res[n, :lens[n]] = flat[int(off[n]):int(off[n + 1])]
    res = res[by_len]
    go1, idx = go + ge, np.arange(ncol + 1, dtype=np.int32)
    H, A, B = (np.zeros((DB_COUNT, ncol + 1), dtype=np.int32) for _ in range(3))
    best = np.zeros((DB_COUNT, ncol), dtype=np.int32)
    for j in range(res.shape[1]):
        n = int((lens > j).sum())                              # the sequences that have a row j: the n longest
        Hp, Ap, Bp = H[:n], A[:n], B[:n]
        h = np.zeros_like(Hp)
        h[:, 1:] = np.maximum(0, np.maximum(np.maximum(Hp, Ap), Bp)[:, :-1] + prof[:, res[:n, j]].T)
        a = np.maximum(0, np.maximum(np.maximum(Hp, Bp) + go1, Ap + ge))
        a[:, 0] = 0
        # B[i] = max(0, max(H, A)[i - 1] + go1, B[i - 1] + ge), B[0] = 0: a running maximum along the row
        y = np.zeros_like(Hp)
        y[:, 1:] = np.maximum(0, np.maximum(h, a)[:, :-1] + go1)
        b = np.maximum.accumulate(y - idx * ge, axis=1) + idx * ge
        H[:n], A[:n], B[:n] = h, a, b
        np.maximum(best[:n], h[:, 1:], out=best[:n])
    out = np.empty_like(best)
    out[by_len] = best
    out.setflags(write=False)
    return out


def case_column_best(case):
    from gapless_cases import PRICED_OUT
    go, ge = PRICED_OUT if case["family"] == "gapless" else case["gaps"]
    return column_best(case["scoring"], go, ge)[:, :case["lq"]]


def column_classes(case):
    """int [lq]: which lane-local column of which instantiation fills each query column -- k = 0 .. K - 1 in the passes
    on K columns per lane, K + k in a last pass on last_k columns of its own (another instantiation)."""
    K, G, lk = case["K"], case["G"], case["last_k"]
    col = np.arange(case["lq"])
    cls = (col % (G * K)) % K
    if lk:
        base = G * K * (case["passes"] - 1)
        cls = np.where(col >= base, K + (col - base) % lk, cls)
    return cls


def pinned_classes(case):
    """The lane-local columns a wrong cell of which would change a score the main fill reports: those that hold every
    best cell of some sequence below the cells' ceiling (a sequence at or above it is scored again by other kernels)."""
    best, cls = case_column_best(case), column_classes(case)
    t = best.max(axis=1)
    ceiling = cell_ceiling(case)
    ok = (t > 0) & ((t < ceiling) if ceiling else True)
    at = best == t[:, None]
    lo, hi = np.where(at, cls, 1 << 20).min(axis=1), np.where(at, cls, -1).max(axis=1)
    return set(lo[ok & (lo == hi)].tolist())


# ---- the matrix ---------------------------------------------------------------------------------------------------
def rot(K):
    """The group width a K meets first: every K meets one, every width ten K or more."""
    return WIDTHS[K % 3]


def last_lane_cut(K):
    """Columns the last lane of the group is short of: 1 .. K - 1, so the prefix length is no multiple of K."""
    return max(1, K // 2)


def single_lq(K, G):
    return G * K - last_lane_cut(K)


def own_last_k(K):
    """The columns per lane the last of several passes is given: about half the others', or K itself where nothing
    smaller exists."""
    return max(2, (K + 1) // 2) if K > 2 else 2


def multi_lq(K, G, passes, last_k):
    return G * K * (passes - 1) + G * last_k - max(1, last_k // 2)


def _case(family, K, G, passes, lq, scoring, gaps=None, W=0, **kw):
    c = dict(family=family, K=K, G=G, W=W, passes=passes, lq=lq, scoring=scoring, gaps=gaps or GAPS[scoring],
             options={}, form=0, fma=0, last_k=0, bits=16, launcher="dyn", exact=0, replaced=False, last_pass=1)
    c.update(kw)
    assert 0 < lq <= QLEN and G * K * (passes - 1) < lq <= G * K * passes, c
    c["id"] = "%s-K%d-G%d-W%d-p%d-lq%d%s" % (family, K, G, W, passes, lq, "" if c["last_pass"] else "-nolast")
    return c


def _multi(family, K, G, scoring, min_lq=0, **kw):
    """Two passes (three where they are short), the last one on own_last_k(K) columns per lane."""
    while 2 * G * K > QLEN and G > 16:
        G //= 2
    passes = 3 if 3 * G * K <= 700 else 2
    while G * K * passes - last_lane_cut(K) < min_lq:
        passes += 1
    lk = own_last_k(K)
    lq = multi_lq(K, G, passes, lk)
    if lq < min_lq:
        lk, lq = K, G * K * passes - last_lane_cut(K)
    return _case(family, K, G, passes, lq, scoring, last_k=lk if lk < K else 0, **kw)


# f16_pair = 2 with a forced workgroup size (or, at 64 lanes, any): geometries whose fma candidate the planner drops --
# the lane-group records do not fit beside the doubled profile, or it would cost resident wavefronts -- and which must
# run the v_perm_b32 kernels: (lanes, forced W, the K)
FALLBACK = ((64, 0, (19, 20)), (16, 4, tuple(range(17, 33))), (32, 4, tuple(range(9, 33))), (64, 4, tuple(range(5, 21))))
# last passes under the fma pairing: main geometry 16 x 32 and 32 x 32, the last pass on 23 and 24 columns per lane (the
# instantiations with edges the planner keeps out of its own candidates), on an odd K (padded to even), on 2
FMA_LAST_KS = (23, 24, 13, 2)
Q32_KS = (11, 15, 19, 27, 29)
X32_GAPS = ((0, 1), (-4, 3))


def _x32_group(K, passes):
    """The widest group not above rot(K) whose int32 profile (K padded to even, 128 bytes per column) and records fit LDS."""
    G = rot(K)
    while G > 16 and (G * ((K + 1) // 2 * 2) * 128 + 4 * (64 // G) * 512 > LDS or G * K * passes > QLEN):
        G //= 2
    return G


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    f16 = dict(options={"f16": 2}, form=2)
    for K in KS:
        G = rot(K)
        # int16 cells, f16 = 0
        out.append(_case("i16_single", K, G, 1, single_lq(K, G), "b62", options={"f16": 0}))
        out.append(_multi("i16_multi", K, G, "b62", options={"f16": 0}))
        # the wide form: a score bound of 32767 or more, i.e. 258 hot columns (and the 270-column copy inside the prefix)
        if single_lq(K, G) >= 275:
            out.append(_case("i16_wide", K, G, 1, single_lq(K, G), "hot", options={"f16": 0}, form=1))
        else:
            out.append(_multi("i16_wide", K, 64 if G * K < 100 else G, "hot", min_lq=275, options={"f16": 0}, form=1))
        # f16 cells, v_perm_b32 pairing
        out.append(_case("f16_perm_single", K, G, 1, single_lq(K, G), "hot", options={"f16": 2, "f16_pair": 1}, form=2))
        out.append(_multi("f16_perm_multi", K, G, "hot", options={"f16": 2, "f16_pair": 1}, form=2))
        # f16 cells, fma pairing, max_waves left free
        for Gf in WIDTHS:
            if Gf < 64 or K <= 18:
                out.append(_case("f16_fma_single", K, Gf, 1, single_lq(K, Gf), "hot", options={"f16": 2, "f16_pair": 2}, form=2, fma=1))
        if K not in (23, 24):
            Gm = G if (G < 64 or K <= 18) else 32
            out.append(_multi("f16_fma_multi", K, Gm, "hot", options={"f16": 2, "f16_pair": 2}, form=2, fma=1))
        # the gapless cells
        out.append(_case("gapless", K, G, 1, single_lq(K, G), "hot", options={}, form=3))
        # the exact int32 cells: a positive gap score
        gaps = X32_GAPS[K % 2]
        if K <= X32_MAX_K:
            for passes in (1, 2):
                Gx = _x32_group(K, passes)
                lq = single_lq(K, Gx) if passes == 1 else multi_lq(K, Gx, 2, K)
                out.append(_case("x32_single" if passes == 1 else "x32_edges", K, Gx, passes, lq, "b62", gaps=gaps, bits=32,
                                 launcher="q32", exact=1))
        else:   # beyond what the exact cells hold: the library runs a geometry of its own, the log says which
            out.append(_case("x32_single", K, 16, 1, single_lq(K, 16), "b62", gaps=gaps, bits=32, launcher="q32", exact=1, replaced=True))
    for Gf, W, ks in FALLBACK:
        for K in ks:
            out.append(_case("f16_fallback", K, Gf, 1, single_lq(K, Gf), "hot", W=W, options={"f16": 2, "f16_pair": 2}, form=2, fma=0))
    for Gm in (16, 32):
        for lk in FMA_LAST_KS:
            out.append(_case("f16_fma_last", 32, Gm, 2, multi_lq(32, Gm, 2, lk), "hot", options={"f16": 2, "f16_pair": 2}, form=2,
                             fma=1, last_k=lk))
        out.append(_case("f16_fma_last", 32, Gm, 2, multi_lq(32, Gm, 2, 23), "hot", options={"f16": 2, "f16_pair": 2, "last_pass": 0},
                         form=2, fma=1, last_k=0, last_pass=0))
    # the reduced int32 cells (force_bits = 32) at the K no other deterministic test forces
    for K in Q32_KS:
        out.append(_case("q32_single", K, 16, 1, single_lq(K, 16), "b62", options={"force_bits": 32}, bits=32, launcher="q32"))
        out.append(_case("q32_edges", K, 16, 2, multi_lq(K, 16, 2, K), "b62", options={"force_bits": 32}, bits=32, launcher="q32"))
    ids = [c["id"] for c in out]
    assert len(set(ids)) == len(ids)
    return tuple(out)


# every (family, K) the matrix must hold: what the completeness test compares CASES with, for the K of the source's macro
def required(ks):
    need = set()
    for K in ks:
        for fam in ("i16_single", "i16_multi", "i16_wide", "f16_perm_single", "f16_perm_multi", "gapless", "x32_single"):
            need.add((fam, K))
        need |= {("f16_fma_single", K, 16), ("f16_fma_single", K, 32)}
        if K <= 18:
            need.add(("f16_fma_single", K, 64))
        if K not in (23, 24):
            need.add(("f16_fma_multi", K))
        if K <= X32_MAX_K:
            need.add(("x32_edges", K))
    return need


def held():
    have = set()
    for c in cases():
        have.add((c["family"], c["K"]))
        if c["family"] == "f16_fma_single":
            have.add((c["family"], c["K"], c["G"]))
    return have


def groups():
    """(family, lanes) -> the cases of one GPU test item, in matrix order."""
    g = {}
    for c in cases():
        g.setdefault((c["family"], c["G"]), []).append(c)
    return g


def cell_ceiling(case):
    """What the cells of a case's main fill flag at (None: int32, nothing is flagged)."""
    return {0: I16_CEILING, 1: WIDE_CEILING, 2: F16_CEILING, 3: F16_CEILING}[case["form"]] if case["bits"] == 16 else None


def expected_main_launches(case):
    """The main fill's launches as the log must name them, in order: (family, K, lanes, form, edges, fma or exact)."""
    edges = 1 if (case["passes"] > 1 or case["form"] == 1) else 0
    flag = case["fma"] if case["launcher"] == "dyn" else case["exact"]
    recs = [(case["launcher"], case["K"], case["G"], case["form"], edges, flag)] * case["passes"]
    if case["last_k"]:
        recs[-1] = (case["launcher"], case["last_k"], case["G"], case["form"], edges, flag)
    return recs


def pairs_by_rank(order):
    """The sorted order's pairs (ranks 2p, 2p + 1) as original indices; the odd database's last pair has one member."""
    order = [int(i) for i in order]
    return [tuple(order[i:i + 2]) for i in range(0, len(order), 2)]
