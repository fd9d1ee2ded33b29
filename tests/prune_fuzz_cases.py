"""The cases of the pruned-search fuzz (plain module, no tests of its own): one generator for the pinned slice of
test_gpu_prune_fuzz.py / test_prune_fuzz_cases_host.py and for the soak of fuzz_prune_gpu.py.

case(seed, i) draws, from np.random.default_rng([seed, i]) alone, one point of the space the hits-only pruning and
swg_search_above were never fuzzed over: a scoring table (the three shipped ones and the int8 edges of
scoring_edges.py), a gap point (zero gaps, a zero open or extend, the magnitudes either side of the f16 cells' 2048, one
positive point that must stay unpruned), an index or PSSM query of 1 .. 600 columns, a database of 600 .. 4000 sequences
of one of six families, a launch geometry with 1, 2 or many segments, the forced pruning levels, the k of the top-K asks
and the seeds of a view.  What a search must return is the oracle's business; the case only says, in `expect_pruned`,
whether swg_prune_plan prunes it (pruned_topk / pruned_above have the rule).

SLICE names the pinned cases.  Its seed was the first one tried: every value of every dimension occurs within SLICE[1]
cases (test_prune_fuzz_cases_host.py), and the GPU test's condition that three quarters of the pruned cases skip a pair
held for it (36 of 45), so nothing was redrawn."""
import hashlib

import numpy as np

import scoring_edges as se

SLICE = (0x5EED5000, 48)

TABLES = ("BLOSUM62", "PAM250", "BLOSUM45", "diag127", "full_range", "blosum62_dirty0", "all_127", "all_m128")
GAPS = ((-2, -1), (0, 0), (-11, -1), (0, -1), (-3, 0), (0, -2048), (-2046, -1), (-1, 0), (0, -127), (-126, -1),
        (-2047, -1), (-2048, -1), (0, -16000), (1, -3))
QUERY_KINDS = ("index", "pssm")
LQS = (1, 3, 5, 31, 64, 65, 200, 257, 600)
FAMILIES = ("lognormal", "equal", "long_short", "chunk_edges", "copies", "odd_residues")
SEGMENTS = ("one", "two", "many")
F16 = (0, 2)
LEVELS = {
    "prune_kmer": (0, 1, 4, 5),
    "prune_segments": (0, 1, 8, 16, 32),
    "prune_refine": (0, 1, 64, 128),
    "prune_refine3": (0, 1, 256),
    "prune_refine4": (0, 1, 5256),
    "prune_gate": (0, 1, 2),
    "prune_cut": (0, 1),
    "prune_table_bits": (0, 16),
}
K_ASKS = ("1", "2", "10", "100", "n-1", "n", "n+5")
EDGE_BLOCKS = (4, 5, 6, 9, 10, 11, 31, 32, 33, 40, 41, 160, 161)   # the k = 5 unit, its tail, chunks of 8 and of 32 units
MAX_CELLS = 3 * 10 ** 8          # lq x residues of a case
PASS_COLUMNS = 64                # cols_per_wave 4 x group_lanes 16
TOPK_CAPACITY = 4096             # the largest k the device top-K selects (SWG_TOPK_CAND_CAP / 2)
I16_CEILING = 32767
NOT_BOUNDED = 0xFFFFFFFF

GEOMETRY = {"engine": 2, "cols_per_wave": 4, "group_lanes": 16, "long_split": -1, "work_queue": 1, "autotune": 0}

_tables = {}


def table(name):
    """The 32 x 32 int8 table of that name (the shipped ones through the library's reader)"""
    if name not in _tables:
        import swg_loader
        swg = swg_loader.load()
        b62 = np.asarray(swg.load_scoring("BLOSUM62").table(), dtype=np.int8).reshape(32, 32)
        if name in ("BLOSUM62", "PAM250", "BLOSUM45"):
            t = np.asarray(swg.load_scoring(name).table(), dtype=np.int8).reshape(32, 32).copy()
        else:
            t = np.asarray(se.table(name, b62), dtype=np.int8).reshape(32, 32).copy()
        t.setflags(write=False)
        _tables[name] = t
    return _tables[name]


def query_bound(sub, q):
    """The most a query can score: every column at its best residue (what the library's score bound sums)"""
    return int(np.maximum(sub[q.astype(np.int64), 1:].astype(np.int64).max(axis=1), 0).sum())


def pair_blocks(lens):
    """Token blocks of the pairs of the length order: two reset rows and the longer sequence, in 4-row blocks"""
    by_len = np.sort(np.asarray(lens, dtype=np.int64))[::-1]
    return (by_len[0::2] + 2 + 3) // 4


def n_segments(lens, lq, segment_blocks):
    """Launch segments of a pass over these sequences (token_segments in swg_api.cpp): one unless the fill has several
    passes and the token image spans more than segment_blocks, else runs of consecutive pairs taken greedily."""
    blocks = pair_blocks(lens)
    total = int(blocks.sum())
    if lq <= PASS_COLUMNS or segment_blocks == 0 or total <= segment_blocks:
        return 1
    pre = np.concatenate([[0], np.cumsum(blocks)])
    b, n = 0, 0
    while b < len(blocks):
        e = int(np.searchsorted(pre, pre[b] + segment_blocks, side="right")) - 1
        assert e > b
        b, n = min(e, len(blocks)), n + 1
    return n


def structural(case):
    """The conditions of swg_prune_plan that the case holds by construction or not at all: the geometry is the 16-bit
    lane groups' work queue with one class and one cell form; what is left is the sign of the gap scores."""
    return case["gap_open"] <= 0 and case["gap_extend"] <= 0


def pruned_topk(case, lens, k):
    """Whether a hits-only search for the k best of the sequences of these lengths is pruned under prune = 2: k within the
    device selection's capacity, and, where the range is one segment, a head of ceil(k / 2) pairs that leaves a rest."""
    pairs = (len(lens) + 1) // 2
    if not structural(case) or k < 1 or k > TOPK_CAPACITY or pairs == 0:
        return False
    return n_segments(lens, len(case["query"]), case["options"]["segment_blocks"]) > 1 or (k + 1) // 2 < pairs


def pruned_above(case, lens):
    """... and a search_above: the structural conditions alone"""
    return structural(case) and len(lens) > 0


def k_value(ask, n):
    return {"n-1": n - 1, "n": n, "n+5": n + 5}.get(ask) or int(ask)


def thresholds(scores, ks):
    """The thresholds of a case from the oracle's scores (of the sequences searched): 1, the k-th best score and one
    above it for every k, the best and one above it, and 4095 .. 4097 where the scores reach them; each at least 1."""
    s = np.sort(np.asarray(scores, dtype=np.int64))[::-1]
    ts = {1, int(s[0]), int(s[0]) + 1}
    for k in ks:
        kth = int(s[min(k, len(s)) - 1])
        ts |= {kth, kth + 1}
    ts |= {t for t in (4095, 4096, 4097) if s[0] >= t}
    return sorted(max(1, t) for t in ts)


def _relative(rng, q, n, hi):
    """n residues that hold a stretch of the query with a few substitutions and single indels"""
    m = min(len(q), n)
    at = int(rng.integers(0, len(q) - m + 1))
    piece = [int(v) for v in q[at:at + m]]
    for _ in range(int(rng.integers(0, 4))):
        if len(piece) > 2:
            p = int(rng.integers(1, len(piece)))
            if rng.random() < 0.5:
                del piece[p]
            else:
                piece.insert(p, int(rng.integers(1, hi + 1)))
    piece = np.array(piece[:n], dtype=np.int8)
    sub_at = rng.random(len(piece)) < 0.05
    piece[sub_at] = rng.integers(1, hi + 1, size=int(sub_at.sum()))
    out = rng.integers(1, hi + 1, size=n).astype(np.int8)
    to = int(rng.integers(0, n - len(piece) + 1))
    out[to:to + len(piece)] = piece
    return out


def _database(rng, family, q, budget):
    """-> list of sequences (int8 arrays); budget: residues the case may hold"""
    lq = len(q)
    n = int(rng.integers(600, 4001))
    hi = 20
    if family == "lognormal" or family == "odd_residues":
        lens = np.clip(rng.lognormal(4.6, 0.7, size=n), 20, 600).astype(np.int64)
    elif family == "equal":
        lens = np.full(n, int(rng.integers(1, 301)), dtype=np.int64)
    elif family == "long_short":
        lens = np.concatenate([rng.integers(900, 1001, size=60), rng.integers(1, 5, size=n - 60)])
    elif family == "chunk_edges":
        lens = np.array([4 * EDGE_BLOCKS[j % len(EDGE_BLOCKS)] - 3 for j in range(n)], dtype=np.int64)
    else:   # copies
        lens = np.full(n, int(rng.integers(8, 201)), dtype=np.int64)
    while lens.sum() > budget and len(lens) > 600:
        lens = lens[:max(600, len(lens) * 3 // 4)]
    if lens.sum() > budget:
        lens = np.maximum(1, lens * budget // lens.sum())
    n = len(lens)
    lens = lens[rng.permutation(n)]
    if family == "copies":
        one = _relative(rng, q, int(lens[0]), hi)
        others = rng.random(n) < (0.0 if rng.random() < 0.5 else 0.5)
        return [rng.integers(1, hi + 1, size=int(L)).astype(np.int8) if o else one.copy() for L, o in zip(lens, others)]
    seqs = [rng.integers(1, hi + 1, size=int(L)).astype(np.int8) for L in lens]
    # relatives of the query: a third of a lognormal database, some twenty elsewhere (among the long ones of long_short)
    if family in ("lognormal", "odd_residues"):
        rel = np.flatnonzero(rng.random(n) < 1 / 3)
    elif family == "long_short":
        rel = np.flatnonzero(lens >= 900)[::3]
    else:
        rel = rng.choice(n, size=20, replace=False)
    for j in rel:
        seqs[j] = _relative(rng, q, int(lens[j]), hi)
    if family == "odd_residues":   # B, Z, X, U, O, J, * and the indices behind them: class 21 of the k-mer tables
        for s in seqs:
            at = rng.random(len(s)) < 0.15
            s[at] = rng.integers(21, 32, size=int(at.sum()))
    return seqs


def _levels(rng, force4):
    """The forced levels: values the option takes, in combinations a context builds (a first-level table of k = 5 beyond 8
    segments is over its budget); the fourth level forced only where asked, with the byte tables and the list it needs."""
    lv = {key: int(rng.choice(vals)) for key, vals in LEVELS.items()}
    if lv["prune_kmer"] == 5 and lv["prune_segments"] > 8:
        lv["prune_segments"] = int(rng.choice([0, 1, 8]))
    lv["prune_refine4"] = 5256 if force4 else int(rng.choice([0, 1]))
    if force4:
        lv["prune_cut"], lv["prune_table_bits"] = 0, 0
    return lv


def case(seed, i):
    """-> dict: seed, i, table_name, table, gap_open, gap_extend, query_kind, query, pssm (or None), family, flat, off,
    segments, options (geometry, f16, segment_blocks and the levels), k_asks, ks, view_seed, expect_pruned
    ({"topk": {k: bool}, "above": bool} for the whole database)."""
    rng = np.random.default_rng([seed, i])
    c = {"seed": int(seed), "i": int(i)}
    c["table_name"] = str(rng.choice(TABLES))
    sub = table(c["table_name"])
    c["table"] = sub
    c["gap_open"], c["gap_extend"] = (int(v) for v in GAPS[int(rng.integers(0, len(GAPS)))])
    c["query_kind"] = str(rng.choice(QUERY_KINDS))
    c["family"] = str(rng.choice(FAMILIES))
    q_hi = 31 if c["family"] == "odd_residues" or rng.random() < 1 / 3 else 20
    # one cell form: a query whose best score stays within the int16 cells
    while True:
        lq = int(rng.choice(LQS))
        q = rng.integers(1, q_hi + 1, size=lq).astype(np.int8)
        if query_bound(sub, q) <= I16_CEILING:
            break
    c["query"] = q
    c["pssm"] = np.ascontiguousarray(sub[q.astype(np.int64)]) if c["query_kind"] == "pssm" else None
    seqs = _database(rng, c["family"], q, MAX_CELLS // lq)
    lens = np.array([len(s) for s in seqs], dtype=np.int64)
    c["flat"] = np.concatenate(seqs).astype(np.int8)
    c["off"] = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    blocks = pair_blocks(lens)
    c["segments"] = str(rng.choice(SEGMENTS))
    total, most = int(blocks.sum()), int(blocks.max())
    seg_blocks = {"one": 0, "two": total * 3 // 5 + most + 1, "many": max(most + 1, total // int(rng.integers(5, 10)))}[c["segments"]]
    # (one case in eight forces the fourth level: its table is 1.32 GB per new query)
    force4 = int(rng.integers(0, 8)) == 0
    c["options"] = dict(GEOMETRY, f16=int(rng.choice(F16)), segment_blocks=int(seg_blocks), **_levels(rng, force4))
    asks = [str(rng.choice(K_ASKS[:2])), str(rng.choice(K_ASKS[2:4])), str(rng.choice(K_ASKS[4:]))]
    if rng.random() < 0.5:
        asks[int(rng.integers(0, 3))] = str(rng.choice(K_ASKS))
    c["k_asks"] = tuple(dict.fromkeys(asks))
    c["ks"] = tuple(k_value(a, len(lens)) for a in c["k_asks"])
    c["view_seed"] = int(rng.integers(1, 1 << 30))
    c["expect_pruned"] = {"topk": {k: pruned_topk(c, lens, k) for k in c["ks"]}, "above": pruned_above(c, lens)}
    return c


def lengths(case):
    return np.diff(case["off"].astype(np.int64))


def view_members(case):
    """The random view of a case: between a quarter and three quarters of the sequences, ascending"""
    rng = np.random.default_rng(case["view_seed"])
    n = len(case["off"]) - 1
    return np.flatnonzero(rng.random(n) < rng.uniform(0.25, 0.75)).astype(np.uint32)


def digest(c):
    """sha256 over everything a case holds"""
    h = hashlib.sha256()
    for key in ("table", "query", "flat", "off"):
        h.update(np.ascontiguousarray(c[key]).tobytes())
    if c["pssm"] is not None:
        h.update(c["pssm"].tobytes())
    rest = {k: v for k, v in c.items() if k not in ("table", "query", "flat", "off", "pssm")}
    h.update(repr(sorted(rest.items())).encode())
    return h.hexdigest()


def slice_digest(seed=None, count=None):
    h = hashlib.sha256()
    for i in range(count or SLICE[1]):
        h.update(digest(case(seed or SLICE[0], i)).encode())
    return h.hexdigest()


def describe(c):
    return "(seed %#x, i %d) %s gaps (%d, %d) %s lq %d %s n %d %s segments, options %s, ks %s" % (
        c["seed"], c["i"], c["table_name"], c["gap_open"], c["gap_extend"], c["query_kind"], len(c["query"]), c["family"],
        len(c["off"]) - 1, c["segments"], c["options"], c["ks"])


# ---- what a case's levels become, from the library's own choice hooks (no device needed) ---------------------------
def realised(swg, c, route="topk", pair_rows=0):
    """The levels a pruned search of the case runs: dict k, S, S2, S3, S4, gate, and admitted (whether a context builds
    the first-level table).  The hooks are asked as plan_prune asks swg_prune_*_choice: the forced options and the widths
    of the tables for this query; under prune_cut = 1 a top-K search (route "topk") runs no level behind the first and no
    gate, a search_above (route "above") does not read that option."""
    o = c["options"]
    rows = c["pssm"] if c["pssm"] is not None else c["table"]
    query = None if c["pssm"] is not None else c["query"]
    bits = {k: 16 if o["prune_table_bits"] == 16 else swg.debug_prune_table_bits(rows, query, k) for k in (4, 5)}
    lq = len(c["query"])
    pair_rows = pair_rows or 4 * int(pair_blocks(lengths(c)).sum())
    k, S, _, admitted = swg.debug_prune_kmer_choice_seg(forced=o["prune_kmer"], segments=o["prune_segments"], lq=lq, pair_rows=pair_rows)
    lv = swg.debug_prune_refine4_choice(forced=o["prune_kmer"], segments=o["prune_segments"], refine=o["prune_refine"], refine3=o["prune_refine3"],
                                        refine4=o["prune_refine4"], table_bits=bits[4], table_bits5=bits[5], lq=lq, pair_rows=pair_rows)
    assert lv[:2] == (k, S)
    gate = swg.debug_prune_gate_choice(forced=o["prune_kmer"], segments=o["prune_segments"], gate=o["prune_gate"], lq=lq, pair_rows=pair_rows)[2]
    if route == "topk" and o["prune_cut"] == 1:
        return {"k": k, "S": S, "S2": 0, "S3": 0, "S4": 0, "gate": False, "admitted": admitted}
    return {"k": k, "S": S, "S2": lv[2], "S3": lv[3], "S4": lv[4], "gate": gate, "admitted": admitted}
