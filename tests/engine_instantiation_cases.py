"""The matrix of the fixed-stream and the systolic fill instantiations and its inputs (plain module, no tests of its own).

tests/instantiation_cases.py and tests/batch_instantiation_cases.py force every kernel of the work queue.  libswg.so ships
two more families of fill kernels:

  swg_diag_kernel<K, MAXW, MULTIPASS, WIDE>   the lane groups on FIXED STREAMS of pairs (option work_queue = 0): three kernels
      per entry of SWG_DIAG_VARIANTS -- one pass, several passes looped inside the kernel (the last lane's (M, B) spilled
      and read back), the wide form -- each with per-K code of its own and the reset rows between the pairs of a stream.
  swg_fill_kernel<Cells, K, MAXW>             the SYSTOLIC engine (option engine = 1): int16 and packed-f16 cells at every
      strip width the library builds, int32 cells at two of them; what can go wrong is per K and per W (wavefronts of a
      workgroup): the edge ring in LDS, the item ring, the spill between passes (nb = W for bins shorter than W blocks),
      the int32 cells' list mode.

CASES forces every one of them on one small database and says what must run; tests/test_engine_instantiation_cases_host.py
proves on the CPU that the planner answers every case as intended and that the inputs have the properties the cases rely on;
tests/test_gpu_engine_instantiations.py runs them.

Inputs: QUERY (amino acids only; every case searches a prefix of it) and DB_COUNT = 267 sequences of at most MAX_LEN = 372
residues (372 x 11 < 4096: under BLOSUM62 no score bound reaches the f16 cells' ceiling):
  - SHORT: eleven sequences of at most 4 residues, the empty record among them.  The database packs into three bins of 128
    by length, so they ARE the last bin: one block of rows, shorter than W blocks in every multi-pass systolic case.
  - copies of QUERY[0 .. e] for e = 0 .. 10 and exact 12-column copies whose ends sweep the columns 11 .. 58: every column
    0 .. 58 holds all the best cells of some sequence, so every local column of every case does (pinned_classes) -- in
    the prefixes of 9 columns as in those of 2000, for strips of up to 48 columns;
  - GAP_SWEEP: 48 sequences of three exact stretches QUERY[e-35 .. e-25], [e-23 .. e-12], [e-11 .. e], the column e - 24
    left out and one foreign residue put in after column e - 12, for the ends e = 36 .. 83: the best alignment of each
    takes a horizontal gap at column e - 24 and a vertical one at column e - 12, so in every case of 84 columns or more
    every local column's gap registers decide a score too (gap_pinned_classes), not only its match cells;
  - TILES: exact 150-column copies every 100 columns of QUERY: every pass boundary and every wave boundary of every case
    lies strictly inside one of them, so the score of that sequence needs the edge that crosses there (boundaries);
  - random sequences of lengths 5 .. 9, relatives of query stretches with substitutions, insertions and deletions, an
    exact 270-column copy (34290 under "hot": beyond the int16 cells, inside the wide form), random sequences; an odd count.
Scorings: instantiation_cases' "b62" = BLOSUM62 with (-11, -1) and "hot" = scoring_edges.diag127 with (-60, -20).
"""
import functools

import numpy as np

import instantiation_cases as ic

QLEN = 2200
DB_COUNT = 267
MAX_LEN = 372
N_SHORT = 11                        # sequences of at most 4 residues: DB_COUNT - 256, the whole last bin
SWEEP = (11, 59)                    # ends of the 12-column copies: 48 consecutive columns
GAP_SWEEP = (36, 84)                # ends of the gapped copies: 48 consecutive columns
TILE, TILE_STEP = 150, 100
COPY_270 = 270
WIDE_MIN_LQ = 275                   # the wide form: 258 hot columns reach 32767, and the 270-column copy lies inside
STREAM_W = 4                        # option max_waves of the fixed-stream cases: with workgroups = 1, 4 * (64 / G) streams
STREAM_OPTIONS = {"engine": 2, "work_queue": 0, "autotune": 0, "long_split": -1, "workgroups": 1, "max_waves": STREAM_W, "f16": 0}
SYSTOLIC_OPTIONS = {"engine": 1, "autotune": 0}
I32_KS = (32, 16)                   # what the int32 cases were written for; the host test compares it with the library's list
table = ic.table
W_AMINO = ord("W") - 64             # the query's first residue: no other W before column 60, so a lone W scores best there only


# ---- inputs -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def query():
    rng = np.random.default_rng(0xE257)
    q = np.asarray(ic.AMINO, dtype=np.int8)[rng.integers(0, len(ic.AMINO), size=QLEN)]
    others = [a for a in ic.AMINO if a != W_AMINO]
    for c in range(0, 60):
        if q[c] == W_AMINO:
            q[c] = others[c % len(others)]
    q[0] = W_AMINO
    q.setflags(write=False)
    return q


def gap_sweep_parts(e):
    """The three query stretches of the gapped copy that ends at column e, as (first, last + 1)."""
    return (e - 35, e - 24), (e - 23, e - 11), (e - 11, e + 1)


@functools.lru_cache(maxsize=None)
def _database():
    """-> (flat int8, offsets uint64[DB_COUNT + 1], {end e: index of the gapped copy that ends there})."""
    import swg_loader
    b62 = np.asarray(table(swg_loader.load(), "b62"), dtype=np.int64)
    rng = np.random.default_rng(0xE258)
    q = query()
    junk = lambda n: rng.integers(1, 32, size=int(n)).astype(np.int8)
    seqs = [np.zeros(0, dtype=np.int8)]                            # an empty record
    # lengths 1 .. 9 twice: the query's first columns (the copies that end at columns 0 .. 8), and random ones
    for n in range(1, 10):
        seqs.append(q[:n].copy())
        seqs.append(junk(n))
    seqs += [q[7:10].copy(), q[20:24].copy()]                      # two more of at most 4 residues: N_SHORT in all
    assert sum(len(s) <= 4 for s in seqs) == N_SHORT
    seqs += [q[:10].copy(), q[:11].copy()]                         # ... that end at columns 9 and 10
    for e in range(*SWEEP):
        seqs.append(q[e - 11:e + 1].copy())
    first_gapped = len(seqs)
    for e in range(*GAP_SWEEP):
        (a1, b1), (a2, b2), (a3, b3) = gap_sweep_parts(e)
        # the foreign residue: one that scores below zero against both columns beside it
        x = next(x for x in ic.AMINO if b62[x, q[b2 - 1]] < 0 and b62[x, q[a3]] < 0)
        seqs.append(np.concatenate([q[a1:b1], q[a2:b2], np.full(1, x, dtype=np.int8), q[a3:b3]]))
    for a in range(0, QLEN - TILE + 1, TILE_STEP):
        seqs.append(q[a:a + TILE].copy())
    seqs.append(np.concatenate([junk(7), q[:COPY_270], junk(5)]))
    # relatives of query stretches at many offsets and lengths: substitutions, now and then an insertion or a deletion
    starts = np.concatenate([rng.integers(0, 200, size=12), rng.integers(0, QLEN - 200, size=24)])
    for i, a in enumerate(starts):
        n = int(rng.integers(30, 200))
        s = q[a:a + n].copy()
        hit = rng.random(n) < (0.0, 0.05, 0.12)[i % 3]
        s[hit] = junk(int(hit.sum()))
        if i % 2 == 1:
            cut = int(rng.integers(8, n - 8))
            s = np.concatenate([s[:cut], junk(rng.integers(1, 3)), s[cut:]]) if i % 4 == 1 else np.concatenate([s[:cut], s[cut + 2:]])
        s = np.concatenate([junk(rng.integers(0, 40)), s, junk(rng.integers(0, 40))])
        seqs.append(s[:MAX_LEN].astype(np.int8))
    assert len(seqs) < DB_COUNT, len(seqs)
    while len(seqs) < DB_COUNT:
        seqs.append(junk(rng.integers(10, MAX_LEN + 1)))
    seqs[-1] = junk(MAX_LEN)                                       # (the longest the f16 bound allows is there)
    assert len(seqs) == DB_COUNT and DB_COUNT % 2 == 1 and 256 < DB_COUNT <= 384
    order = rng.permutation(DB_COUNT)
    seqs = [seqs[i] for i in order]
    where = {int(o): i for i, o in enumerate(order)}
    gapped = {e: where[first_gapped + e - GAP_SWEEP[0]] for e in range(*GAP_SWEEP)}
    flat = np.concatenate(seqs).astype(np.int8)
    off = np.zeros(DB_COUNT + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    flat.setflags(write=False)
    off.setflags(write=False)
    return flat, off, gapped


def database():
    """-> (flat int8, offsets uint64[DB_COUNT + 1])."""
    return _database()[:2]


@functools.lru_cache(maxsize=None)
def window_truth(a, b, scoring, go, ge):
    """The int32 oracle's scores against QUERY[a:b] (computed once per window, scoring and gaps; read-only)."""
    import swg_loader
    orc, swg = swg_loader.oracle(), swg_loader.load()
    flat, off = database()
    t = orc.score_db(np.ascontiguousarray(query()[a:b]), flat, off, table(swg, scoring), go, ge)
    t.setflags(write=False)
    return t


def truth(case):
    return window_truth(0, case["lq"], case["scoring"], *case["gaps"])


@functools.lru_cache(maxsize=None)
def column_best(scoring, go, ge, ncol):
    """int32 [DB_COUNT, ncol]: the best match-state cell of every column of QUERY[:ncol], per sequence, in plain numpy: the
    recurrence of instantiation_cases.column_best (which is tied to that module's database) on this module's inputs.  A
    cell depends on the columns to its left only, so the score against a prefix of lq <= ncol columns is
    column_best[:, :lq].max(1): the host test holds that against the oracle for every case, bit for bit."""
    import swg_loader
    flat, off = database()
    lens = np.diff(off).astype(np.int64)
    by_len = np.argsort(-lens, kind="stable")
    sub = np.asarray(table(swg_loader.load(), scoring), dtype=np.int32)
    prof = sub[query()[:ncol].astype(np.int64)]                # [columns, 32]
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
    ncol = max(c["lq"] for c in cases() if (c["scoring"], c["gaps"]) == (case["scoring"], case["gaps"]))
    return column_best(case["scoring"], case["gaps"][0], case["gaps"][1], ncol)[:, :case["lq"]]


def column_classes(case):
    """int [lq]: the local column that fills each query column: col % K of a systolic strip, (col % (G * K)) % K of a lane."""
    col = np.arange(case["lq"])
    return col % case["K"] if case["engine"] == 1 else (col % (case["G"] * case["K"])) % case["K"]


def cell_ceiling(case):
    """What the cells of a case's main fill flag at (None: nothing is flagged -- int32 cells, and the systolic f16 cells,
    which run only where no score can reach their ceiling)."""
    if case["bits"] == 32 or case["form"] == 2:
        return None
    return ic.WIDE_CEILING if case["form"] == 1 else ic.I16_CEILING


def counted(case):
    """bool [DB_COUNT]: the sequences whose score the main fill reports (below the cells' ceiling, above zero)."""
    t, ceiling = truth(case), cell_ceiling(case)
    return (t > 0) & ((t < ceiling) if ceiling else True)


def pinned_classes(case):
    """The local columns a wrong cell of which would change a score the main fill reports: those that hold every best
    cell of some sequence below the cells' ceiling."""
    best, cls = case_column_best(case), column_classes(case)
    t = best.max(axis=1)
    at = best == t[:, None]
    lo, hi = np.where(at, cls, 1 << 20).min(axis=1), np.where(at, cls, -1).max(axis=1)
    return set(lo[counted(case) & (lo == hi)].tolist())


def gap_pinned_classes(case, swg):
    """The local columns whose gap registers decide a score the main fill reports: the columns e - 24 (left out) and e - 12
    (a residue put in behind it) of every gapped copy that lies inside the prefix, scores below the cells' ceiling, and
    scores exactly what its three stretches score less the two gaps -- more than any two of them with one gap, as each
    stretch scores more than a gap costs."""
    sub = np.asarray(table(swg, case["scoring"]), dtype=np.int64)
    q, cls, t, ok = query().astype(np.int64), column_classes(case), truth(case), counted(case)
    gap = -(case["gaps"][0] + case["gaps"][1])
    out = set()
    for e, i in _database()[2].items():
        if e >= case["lq"] or not ok[i]:
            continue
        parts = [int(sub[q[a:b], q[a:b]].sum()) for a, b in gap_sweep_parts(e)]
        if min(parts) > gap and int(t[i]) == sum(parts) - 2 * gap:
            out |= {int(cls[e - 24]), int(cls[e - 12])}
    return out


def boundaries(case):
    """The query columns at which an edge is handed over: where a pass ends (through the spill) and, in a systolic
    workgroup of several wavefronts, where a strip ends (through the ring in LDS)."""
    step = case["K"] if case["engine"] == 1 else case["G"] * case["K"]      # (a pass of W strips ends where a strip ends)
    return list(range(step, case["lq"], step))


# ---- the matrix ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def systolic_variants(bits):
    """[(K, max_waves)] of the systolic instantiations, from the library (swg_num_variants / swg_variant_info)."""
    import swg_loader
    swg_loader.build_module().build(verbose=False)     # (as conftest's fixtures: the matrix is read when tests are collected)
    return tuple(swg_loader.load().debug_systolic_variants(bits))


def strip_cut(K):
    """Columns the last strip is short of: odd, 1 .. K - 1, so that lq = K * W - cut is no multiple of 4 (K * W is one of 8)."""
    return K // 2 - 1


def _case(family, engine, K, G, W, passes, lq, scoring, options, form=0, bits=16, rescore=None):
    c = dict(family=family, engine=engine, K=K, G=G, W=W, passes=passes, lq=lq, scoring=scoring, gaps=ic.GAPS[scoring],
             options=dict(options), form=form, bits=bits, rescore=rescore)
    assert 0 < lq <= QLEN, c
    c["id"] = "%s-K%d-G%d-W%d-p%d-lq%d" % (family, K, G, W, passes, lq)
    return c


def _stream(family, K, G, passes, lq, scoring, form=0):
    assert G * K * (passes - 1) < lq <= G * K * passes and lq % K != 0, (family, K, G, passes, lq)
    opts = dict(STREAM_OPTIONS, cols_per_wave=K, group_lanes=G)
    return _case(family, 2, K, G, STREAM_W, passes, lq, scoring, opts, form=form)


def stream_multi_lq(K, G, passes):
    """Several passes: the last one's last quarter of lanes empty, the lane before them partly filled."""
    return G * K * passes - K * (G // 4) - ic.last_lane_cut(K)


def _systolic(family, K, W, passes, scoring, options, form=0, bits=16, rescore=None, max_waves=0):
    lq = K * W * passes - strip_cut(K)
    assert lq % 4 != 0 and K * (W * passes - 1) < lq
    opts = dict(SYSTOLIC_OPTIONS, cols_per_wave=K, **options)
    if max_waves:
        opts["max_waves"] = max_waves
    return _case(family, 1, K, 0, W, passes, lq, scoring, opts, form=form, bits=bits, rescore=rescore)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for K in ic.KS:
        G = ic.rot(K)
        out.append(_stream("streams_single", K, G, 1, ic.single_lq(K, G), "b62"))
        Gm = G
        while 2 * Gm * K > QLEN and Gm > 16:
            Gm //= 2
        passes = 3 if 3 * Gm * K <= 700 else 2
        out.append(_stream("streams_multi", K, Gm, passes, stream_multi_lq(K, Gm, passes), "b62"))
        # the wide form: a score bound of 32767 or more; one pass where G * K holds the 275 columns, else several
        if ic.single_lq(K, G) >= WIDE_MIN_LQ:
            out.append(_stream("streams_wide", K, G, 1, ic.single_lq(K, G), "hot", form=1))
        else:
            Gw, passes = 64 if G * K < 100 else G, 2
            while stream_multi_lq(K, Gw, passes) < WIDE_MIN_LQ:
                passes += 1
            out.append(_stream("streams_wide", K, Gw, passes, stream_multi_lq(K, Gw, passes), "hot", form=1))
    for K, maxw in systolic_variants(16):
        for W in (1, 2, maxw):
            out.append(_systolic("systolic_i16", K, W, 1, "b62", {"f16": 0}))
            out.append(_systolic("systolic_f16", K, W, 1, "b62", {"f16": 1}, form=2))
        # several passes through max_waves (f16 left on: the f16 cells are single-pass by plan, so these run int16 cells)
        for mw in (2, 3):
            out.append(_systolic("systolic_multi", K, mw, mw, "b62", {"f16": 1}, max_waves=mw))
    # the 270-column copy saturates the int16 cells: re-scored by the systolic int32 kernel (its default strip) in list
    # mode, in one pass and in several
    Kf, Kr = systolic_variants(16)[0][0], systolic_variants(32)[0][0]      # the default strips of the fill and of the re-score
    for mw in (0, 3):
        lq = 277
        passes = 1 if not mw else -(-lq // (mw * Kf))
        p32 = 1 if not mw else -(-lq // (mw * Kr))
        out.append(_case("systolic_hot", 1, Kf, 0, -(-lq // (passes * Kf)), passes, lq, "hot",
                         dict(SYSTOLIC_OPTIONS, cols_per_wave=Kf, **({"max_waves": mw} if mw else {})), rescore=(Kr, -(-lq // (p32 * Kr)), p32)))
    for K, maxw in systolic_variants(32):
        out.append(_systolic("systolic_i32", K, 6, 1, "b62", {"force_bits": 32}, bits=32))
        out.append(_systolic("systolic_i32", K, 3, 2, "b62", {"force_bits": 32}, bits=32, max_waves=3))
    ids = [c["id"] for c in out]
    assert len(set(ids)) == len(ids)
    return tuple(out)


def groups():
    """(family, lanes of a fixed-stream group or columns of a systolic strip) -> the cases of one GPU test item."""
    g = {}
    for c in cases():
        g.setdefault((c["family"], c["G"] if c["engine"] == 2 else c["K"]), []).append(c)
    return g


def expected_launches(case):
    """The main fill's launches as the log must name them: (family, K, lanes, W, form, edges, flag).  The fixed streams loop
    their passes inside ONE launch (edges: the multi-pass or the wide kernel); so does the systolic fill (flag: int32 cells)."""
    if case["engine"] == 2:
        return [("streams", case["K"], case["G"], case["W"], case["form"], 1 if (case["passes"] > 1 or case["form"] == 1) else 0, 0)]
    return [("systolic", case["K"], 0, case["W"], case["form"], 1 if case["passes"] > 1 else 0, 1 if case["bits"] == 32 else 0)]


def expected_list_launches(case):
    """The launches off a device-side list that must follow: the systolic int32 re-score of what saturated int16 cells."""
    if not case["rescore"]:
        return []
    K, W, passes = case["rescore"]
    return [("systolic", K, 0, W, 0, 1 if passes > 1 else 0, 1)]
