"""Shared by the call-order tests (plain module, no tests of its own): no call's answer may depend on the calls before it.

A swg_ctx and a swg_db remember a great deal between calls -- profile slots, k-mer tables, tuned geometries, the two
hints, layouts, staging buffers, the process-wide long-class switches -- and each remembered thing is dropped by a key
written by hand.  Three tables describe what the tests do about it:

  PROBES   calls whose answer is compared exactly with the CPU's truth for the session's CURRENT query, scoring and
           default options, every output handed over pre-filled (db_kinds_cases: 0x5A);
  MOVERS   valid calls that change something remembered: every probe, a query of the same length and other content, a
           PSSM, the other scoring, the other handles, every forced route and every option flipped away and back;
  Session  one context with its resident handles, the model of what the library must hold now (length, content, PSSM
           or index, scoring) and the list of calls made so far, which every failure message carries.

The world is db_kinds_cases' (677 sequences) plus `tunable` (4096 + 37 sequences: the least the tuner takes, no score
at the f16 cells' ceiling, so neither hint ever moves on it), the world's masked copy, `relatives` (64 near-copies of a 1000-column query: the
first f16 search flags every pair, the heavier scoring passes 32767) and `one` (a single sequence).  Queries of 40, 130
and 600 columns in two contents each, with their PSSM twins; BLOSUM62 at -11/-1 and at -2100/-1, whose gap magnitude
keeps the f16 cells off.  tests/test_call_order_cases_host.py proves all of that on the CPU."""
import functools
import os
import re

import numpy as np

import above_multi_cases as amc
import db_kinds_cases as dk
import evalue_cases as ec
import gapless_cases as gc
import pssm_build_cases as pc
from test_gpu_stats import counts_of

LENS = (40, 130, 600)
SEED = 20263
N_TUNABLE = 4096 + 37
N_LONG = 12                        # tunable's sequences of 700 to 1500 residues
N_RELATIVES = 64
N_TAILED = 20000                   # the handle whose tuned entry has two classes
N_HEAD, N_DEEP = 14, 8             # relatives of each 40-column query in tunable: among the longest, and deep in the order
LQ_REL = 1000
TOP = 16
K = dk.K
ROWS = 5                           # hits an alignment probe takes
MAX_HSPS = 3
SCORINGS = ((-11, -1), (-2100, -1))            # BLOSUM62 both; the second's first gap position is beyond the f16 cells' 2048
HEAVY = 5                                      # relatives' second scoring: 5 x BLOSUM62 (entries -20 .. 55), gaps -11/-1
CALIB = {"calib_seqs": 256, "calib_len": 64, "calib_seed": 1}    # the session's size of a calibration: what the CPU can follow
DBS = ("tunable", "world")
PLAN_FIELDS = ("engine", "cols_per_wave", "group_lanes", "waves", "passes", "path_bits", "cell_form", "streams", "long_pairs",
               "long_cols_per_lane", "work_queue")

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the options swg_set_option accepts ----------------------------------------------------------------------------------
def accepted_options():
    """Every key swg_set_option takes, read from its own chain of comparisons and the table of refinement levels it walks
    (include/swg.h's comment names most of them, not all: long_cols, long_group, f16_pair, bounds_groups, segment_blocks,
    q32_waves and wave_budget are missing there)."""
    src = open(os.path.join(_ROOT, "seq-align-gpu_amd", "csrc", "swg_api.cpp")).read()
    body = src[src.index('extern "C" int swg_set_option'):src.index('extern "C" int swg_set_scoring')]
    keys = re.findall(r'strcmp\(key, "([a-z0-9_]+)"\)', body)
    assert "refine_option_row(key)" in body
    header = open(os.path.join(_ROOT, "seq-align-gpu_amd", "csrc", "swg_host_internal.h")).read()
    keys += sorted(set(re.findall(r'"(prune_refine\d*)"', header)))
    assert len(keys) == len(set(keys)) and len(keys) >= 40, keys
    return keys


# (key, away from the default, the default, the call that READS the option while it is away, the options set beside it so
# that the call takes the route the option belongs to).  "autotune"'s default is the session's own.  The readers:
#   search        swg_search of tunable, scores and top-K
#   pruned        a hits-only swg_search of tunable under prune 2 (plan_prune reads no prune_* option of a search that is
#                 not pruned, and prune 1 prunes nothing below millions of sequences)
#   several_pass  swg_search of the world at 32 columns a pass
#   two_class     swg_search of the world with the long class split off at 1000 rows
#   int32         swg_search of tunable under force_bits 32
#   heavy         swg_search of relatives under the heavier table, where a score passes 32767
#   multi         swg_search_multi of tunable;  above_multi  swg_search_above_multi of tunable
#   calibrate     swg_calibrate
_KMER4 = {"prune_kmer": 4}
_LEVELS = {"prune_kmer": 4, "prune_segments": 32}
_SEVERAL = {"cols_per_wave": 2, "group_lanes": 16, "long_split": -1}
OPTION_MOVES = (
    ("work_queue", 0, 1, "search", {}), ("last_pass", 0, 1, "several_pass", _SEVERAL), ("wide16", 0, 1, "heavy", {}),
    ("f16", 0, 1, "search", {}), ("f16", 2, 1, "search", {}), ("f16_pair", 1, 0, "search", {}), ("f16_pair", 2, 0, "search", {}),
    ("qq", 0, 1, "multi", {}), ("long_helps", 1, 0, "two_class", {"cols_per_wave": 10, "group_lanes": 64, "long_split": 1000}),
    ("batch", 1, 8, "search", {}), ("batch_blocks", 3, 0, "search", {}),
    ("batch_geometry", 1, 0, "multi", {"cols_per_wave": 4, "group_lanes": 16}), ("force_bits", 32, 0, "search", {}),
    ("force_bits", 16, 0, "search", {}), ("prune", 2, 1, "search", {}), ("prune", 0, 1, "search", {}),
    ("prune_kmer", 4, 0, "pruned", {}), ("prune_kmer", 5, 0, "pruned", {}), ("prune_segments", 8, 0, "pruned", _KMER4),
    ("prune_table_bits", 16, 0, "pruned", _KMER4), ("prune_cut", 1, 0, "pruned", _KMER4), ("prune_head", 8, 4, "pruned", _KMER4),
    ("prune_gate", 2, 0, "pruned", dict(_KMER4, prune_segments=8)), ("prune_gate", 1, 0, "pruned", dict(_KMER4, prune_segments=8)),
    ("prune_refine", 64, 0, "pruned", _LEVELS), ("prune_refine", 1, 0, "pruned", _LEVELS),
    ("prune_refine3", 256, 0, "pruned", dict(_LEVELS, prune_refine=128)),
    ("prune_refine4", 5256, 0, "pruned", dict(_LEVELS, prune_refine=128, prune_refine3=256)),
    ("prune_refine5", 5256, 0, "pruned", dict(_LEVELS, prune_refine=128, prune_refine3=256, prune_refine4=5256)),
    ("above_batch", 1, 0, "above_multi", {}), ("above_batch", 2, 0, "above_multi", {}), ("side_readout", 0, 1, "search", {}),
    ("prio_share", 50, 150, "search", {}), ("q32_waves", 8, 0, "int32", {"force_bits": 32}), ("max_waves", 8, 0, "search", {}),
    ("workgroups", 8, 0, "search", {}), ("segment_blocks", 4096, 0, "several_pass", _SEVERAL),
    ("autotune", 0, None, "search", {}), ("calib_seed", 2, 1, "calibrate", {}),
)
DEFAULTS = {"prune_head": 4, "prune": 1, "batch": 8, "prio_share": 150}      # of the options set beside another; every other one: 0
PROCESS_WIDE = (("long_cols", 8, 0), ("long_group", 16, 0))       # written by any context for all of them: set on a second one
# the forced routes (the options of each, all back to 0 afterwards)
FORCED = {
    "two_class": {"cols_per_wave": 10, "group_lanes": 64, "long_split": 1000},     # 640 columns a pass; world's three long ones apart
    "several_pass": {"cols_per_wave": 2, "group_lanes": 16, "long_split": -1},     # 32 columns a pass: 2, 5 and 19 passes
    "systolic": {"engine": 1},
}
EXCLUDED = {
    "calib_seqs": "set once when a session is made: the size of calibration the CPU truth can follow (CALIB)",
    "calib_len": "set once when a session is made, with calib_seqs",
    "pssm_msa_mb": "read by swg_pssm_build_multi* alone, which no probe calls; tests/test_gpu_pssm_build.py moves it",
    "pssm_blocks": "changes swg_pssm_build's own answer and nothing remembered; tests/test_gpu_pssm_blocks.py",
    "pssm_purge": "changes swg_pssm_build's own answer and nothing remembered; tests/test_gpu_pssm_blocks.py",
    "bounds_groups": "read inside one swg_align_bounds launch, nothing remembered; tests/test_gpu_bounds.py",
    "wave_budget": "goes unchecked into the workgroup count of a launch (q32_waves is checked against the kernel's wavefronts "
                   "and its LDS before it is used): no value is known to make a valid call",
}


def option_names():
    """Every option a mover names."""
    names = [m[0] for m in OPTION_MOVES + PROCESS_WIDE]
    for opts in list(FORCED.values()) + [m[4] for m in OPTION_MOVES]:
        names += list(opts)
    return names


# ---- the world ------------------------------------------------------------------------------------------------------------
def _plant(rng, seqs, i, core):
    seqs[i] = dk._fit(rng, core, len(seqs[i]))


@functools.lru_cache(maxsize=None)
def cases():
    w = dk.world()
    rng = np.random.default_rng(SEED)
    sub = w["sub"]
    other = [pc.random_seq(rng, n) for n in LENS]                      # the second content of each length
    queries = [(w["queries"][li], other[li]) for li in range(3)]
    c = dict(sub=sub, queries=queries, pssms=[tuple(amc.pssms(sub, qs)) for qs in queries])
    c["heavy"] = np.clip(HEAVY * sub.astype(np.int64), -128, 127).astype(np.int8)
    # tunable: mostly 8 .. 90 residues, a handful of 700 .. 1500.  Relatives of every query: three of each 130- and 600-column
    # one (those of 600 columns so far off that nothing reaches the f16 cells' ceiling); of each 40-column one N_HEAD at
    # a tenth substituted in sequences of 86 .. 90 residues, which a pruned search fills unpruned with the other longest
    # ones and takes its threshold from, and N_DEEP all but exact in sequences of 41 .. 60, deep in the length order: they
    # belong to the K best, and a k-mer table of ANOTHER query bounds them below that threshold
    # (tests/test_call_order_cases_host.py)
    lens = np.concatenate([rng.integers(8, 91, size=N_TUNABLE - N_LONG), rng.integers(700, 1501, size=N_LONG)])
    lens = lens[rng.permutation(N_TUNABLE)]
    seqs = [pc.random_seq(rng, int(n)) for n in lens]
    long_ones = np.nonzero(lens >= 700)[0]
    short_ones = np.nonzero((lens >= 86) & (lens <= 90))[0]
    deep_ones = rng.permutation(np.nonzero((lens >= 41) & (lens <= 60))[0])
    assert len(long_ones) == N_LONG and len(short_ones) >= 6 + 2 * N_HEAD and len(deep_ones) >= 2 * N_DEEP
    for ci in range(2):
        for n in range(N_HEAD):
            _plant(rng, seqs, int(short_ones[6 + ci * N_HEAD + n]), pc.relative(rng, queries[0][ci], 0.1))
        for n in range(N_DEEP):
            _plant(rng, seqs, int(deep_ones[ci * N_DEEP + n]), pc.relative(rng, queries[0][ci], 0.025 if n % 2 else 0.0))
        for n in range(3):
            _plant(rng, seqs, int(short_ones[ci * 3 + n]), pc.relative(rng, queries[1][ci], (0.05, 0.15, 0.25)[n]))
            _plant(rng, seqs, int(long_ones[(3 * ci + n) * 2]), pc.relative(rng, queries[2][ci], (0.35, 0.4, 0.45)[n]))
    c["tunable"] = pc.pack(seqs)
    # relatives: near-copies of one rich query (8 a column on average against itself)
    qrel = pc.random_seq(rng, LQ_REL)
    rich = rng.random(LQ_REL) < 0.8
    qrel[rich] = rng.choice([pc.idx(ch) for ch in "WCHYP"], size=int(rich.sum()), p=[0.3, 0.25, 0.2, 0.125, 0.125])
    rel = [pc.relative(rng, qrel, 0.002 * n, lo=0, hi=LQ_REL - int(rng.integers(0, 60))) for n in range(N_RELATIVES)]
    rel[0] = qrel.copy()
    c["qrel"], c["relatives"] = qrel, pc.pack(rel)
    c["one"] = pc.pack([pc.relative(rng, queries[1][0], 0.2)])
    c["world"] = (w["flat"][0], w["off"])
    # tailed: outside tunable's length bounds, for the one thing tunable cannot be.  20 000 sequences of swg_synth_db's
    # protein-like lengths (median 290, up to 5000): at 130 columns the bulk's work per SIMD is of the order of the longest
    # chain, and the cost model splits 776 long pairs off into a class of their own, which the tuner then stores and replays
    import swg_loader
    c["tailed"] = swg_loader.load().synth_db(SEED + 7, N_TAILED)
    c["masked"] = (w["flat"][1], w["off"])                             # what swg_db_mask makes of the world (db_kinds_cases)
    # the reference-shaped batches of swg_fill_batches16: 32 sequences, longest first
    b16 = sorted((pc.random_seq(rng, int(n)) for n in rng.integers(20, 80, size=32)), key=len, reverse=True)
    c["batches16"] = pc.pack(b16)
    lrng = np.random.default_rng(SEED + 1)
    c["lists"] = {}
    for name in DBS:
        n = len(c[name][1]) - 1
        for ci in range(2):
            tops = [[i for _, i in top(name, li, ci, 0, False, _c=c)] for li in range(3)]
            c["lists"][name, ci] = [np.concatenate([t, lrng.choice(n, size=60, replace=False), t[:5]]).astype(np.int64) for t in tops]
    return c


_TRUTH = {}


def truth(name, li, ci, si, gapless=False, _c=None):
    """The CPU's scores of query (li, ci) under scoring si against database `name`; computed once."""
    key = (name, li, ci, 0 if gapless else si, gapless)
    if key not in _TRUTH:
        import swg_loader
        orc = swg_loader.oracle()
        c = _c or cases()
        flat, off = c[name]
        q = c["queries"][li][ci]
        _TRUTH[key] = gc.oracle_gapless(orc, q, flat, off, c["sub"]) if gapless else orc.score_db(q, flat, off, c["sub"], *SCORINGS[si])
        _TRUTH[key].setflags(write=False)
    return _TRUTH[key]


def top(name, li, ci, si, gapless=False, k=TOP, _c=None):
    return amc.above(truth(name, li, ci, si, gapless, _c=_c), 1 - (1 << 30))[:k]


@functools.lru_cache(maxsize=None)
def relatives_truth(heavy):
    import swg_loader
    c = cases()
    flat, off = c["relatives"]
    return swg_loader.oracle().score_db(c["qrel"], flat, off, c["heavy"] if heavy else c["sub"], *SCORINGS[0])


def all_truths():
    """Everything the GPU module compares searches with (the host test bounds the time it takes)."""
    for name in DBS + ("one", "masked"):
        for li in range(3):
            for ci in range(2):
                for si in range(2):
                    truth(name, li, ci, si)
                truth(name, li, ci, 0, True)
    relatives_truth(False), relatives_truth(True)


def _seq(name, i):
    flat, off = cases()[name]
    return flat[int(off[i]):int(off[i + 1])]


@functools.lru_cache(maxsize=None)
def trace(li, ci, si, i):
    """The oracle's alignment of the query with sequence i of the world, as align_stats' dict with the path."""
    import swg_loader
    q, d = cases()["queries"][li][ci], _seq("world", i)
    score, (qb, qe, db_, de), ops = swg_loader.oracle().pair_trace(q, d, cases()["sub"], *SCORINGS[si])
    a = {"score": score, "index": int(i), "q_begin": qb, "q_end": qe, "d_begin": db_, "d_end": de, "n_ops": len(ops), "reserved": 0}
    a.update(zip(dk.CNT.names, counts_of(q, d, qb, db_, ops)))
    a["ops"] = ops
    return a


@functools.lru_cache(maxsize=None)
def hsps(li, ci, si, i):
    import swg_loader
    c = cases()
    out = swg_loader.load().align_hsps_host(c["sub"], *SCORINGS[si], _seq("world", i), MAX_HSPS, dk.MIN_HSP, query=c["queries"][li][ci],
                                            want_counts=True)
    return [dict(a, index=int(i), reserved=0) for a in out]


@functools.lru_cache(maxsize=None)
def built_pssm(li, ci, si):
    import swg_loader
    swg, orc, c = swg_loader.load(), swg_loader.oracle(), cases()
    flat, off = c["world"]
    q = c["queries"][li][ci]
    als = pc.align(orc, q, flat, off, hit_row(li, ci, si), c["sub"], SCORINGS[si])
    return dk.Pssm(*swg.pssm_from_paths(c["sub"], q, flat, off, als, want_values=True))


@functools.lru_cache(maxsize=None)
def calibration(li, ci, si, seed=CALIB["calib_seed"]):
    import swg_loader
    c = cases()
    return ec.truth(swg_loader.load(), swg_loader.oracle(), c["queries"][li][ci], c["sub"], SCORINGS[si], CALIB["calib_seqs"], CALIB["calib_len"],
                    seed=seed)


def hit_row(li, ci, si):
    """The hits the alignment probes take: the world's best ROWS under the current query and scoring."""
    return [i for _, i in top("world", li, ci, si)[:ROWS]]


# ---- a session ------------------------------------------------------------------------------------------------------------
class _Env:
    """What db_kinds_cases' raw calls run with: the three lengths of one content as the batch."""

    def __init__(self, swg, ctx, ci):
        c = cases()
        self.swg, self.ctx = swg, ctx
        self.w = {"queries": [c["queries"][li][ci] for li in range(3)]}
        self.qoff = np.zeros(4, dtype=np.uint64)
        self.qoff[1:] = np.cumsum(LENS)
        self.qflat = np.ascontiguousarray(np.concatenate(self.w["queries"]), dtype=np.int8)
        self.pflat = np.ascontiguousarray(np.concatenate([c["pssms"][li][ci] for li in range(3)]), dtype=np.int8)

    def packed(self, pssm):
        return self.pflat if pssm else self.qflat


class Session:
    """One context at default options (autotune as given) with the four handles resident, the model of its state and
    the names of the calls made on it."""

    def __init__(self, swg, assert_pssm, autotune=1):
        self.swg, self.c, self.assert_pssm, self.autotune = swg, cases(), assert_pssm, autotune
        self.ctx = swg.Context(0)
        self.other = None                                            # the second context, made when a mover first needs it
        for key, v in CALIB.items():
            self.ctx.set_option(key, v)
        self.ctx.set_option("autotune", autotune)
        self.envs = [_Env(swg, self.ctx, ci) for ci in range(2)]
        self.db = {name: swg.Database(*self.c[name]).upload(self.ctx) for name in DBS + ("relatives", "one")}
        self.db["masked"] = self.db["world"].mask(self.ctx)         # the masked twin, made on the device, resident like the rest
        self.li, self.ci, self.pssm, self.si = 0, 0, False, 0
        self.ticket, self.hits_alone = None, False
        self.log, self.stats, self.evidence = [], {}, {}
        self.apply_scoring()
        self.apply_query()

    def close(self):
        if self.ticket:
            self.end_ticket()
        for d in self.db.values():
            d.close()
        if self.other:
            self.other.close()
        self.ctx.close()

    # the model
    state = property(lambda self: (self.li, self.ci, self.si))
    e = property(lambda self: self.envs[self.ci])
    lib = property(lambda self: self.swg.lib)

    def apply_scoring(self):
        self.ctx.set_scoring(self.c["sub"], *SCORINGS[self.si])

    def apply_query(self):
        if self.pssm:
            self.ctx.set_query_pssm(self.c["pssms"][self.li][self.ci])
        else:
            self.ctx.set_query(self.c["queries"][self.li][self.ci])

    def set_state(self, li, ci, pssm, si):
        self.li, self.ci, self.pssm, self.si = li, ci, pssm, si
        self.apply_scoring()
        self.apply_query()

    def where(self, what):
        return "%s at (lq %d, content %d, %s, gaps %s) after %d calls: %s" % (
            what, LENS[self.li], self.ci, "PSSM" if self.pssm else "index", SCORINGS[self.si], len(self.log), " > ".join(self.log))

    def same(self, got, want, what):
        dk.same(got, want, self.where(what), self.assert_pssm)

    def option(self, key, value):
        """An option of the mover list.  Under prune = 2 a search that asks for scores reports 0 for what it skipped
        (include/swg.h: diagnostic), so the movers' searches ask for hits alone while it is set."""
        self.ctx.set_option(key, self.autotune if value is None else value)
        if key == "prune":
            self.hits_alone = value == 2

    # a search queued and left outstanding
    def begin_ticket(self):
        if self.ticket is None:
            self.ticket = (self.ctx.search_begin(self.db["tunable"], k=K, want_scores=True)[0], self.state)

    def end_ticket(self):
        (t, state), self.ticket = self.ticket, None
        db = self.db["tunable"]
        got, _ = dk._search_raw(self.e, db, lambda c, d, s, h, k, nh, st: self.lib.swg_search_end(c, t, s, h, nh, st), K)
        self.same(got, want_search("tunable", state), "the ticket begun earlier, ended now")

    def run_probe(self, name):
        if self.ticket and name not in IN_FLIGHT_OK:
            self.end_ticket()
        self.log.append(name)
        self._named(name, PROBES[name])
        if self.ticket:
            self.end_ticket()

    def run_mover(self, name):
        if self.ticket:
            self.end_ticket()
        self.log.append(name)
        self._named(name, MOVERS[name])

    def _named(self, name, call):
        """A call that is refused fails inside the raw call, on the library's own message: the pair and the calls so far
        are put in front of it."""
        try:
            call(self)
        except (AssertionError, self.swg.SwgError) as err:
            if "calls: " in str(err):
                raise
            raise AssertionError(self.where(name) + ": " + str(err)) from err

    def search(self, name, what, k=K):
        """A plain search of a handle compared with the truth -> its stats (what the movers run under their options)."""
        got, st = dk._search_raw(self.e, self.db[name], self.lib.swg_search, k, want_scores=not self.hits_alone)
        self.same(got, want_search(name, self.state, k, scores=not self.hits_alone), "%s: search[%s]" % (what, name))
        return st


# ---- what truth says ------------------------------------------------------------------------------------------------------
def _hits(pairs):
    return [dk.H(s, i) for s, i in pairs]


def want_search(name, state, k=K, scores=True, gapless=False):
    t = truth(name, *state, gapless)
    out = {"hits": _hits(amc.above(t, 1 - (1 << 30))[:k]), "tail": True}
    if scores:
        out["scores"] = dk.ByIndex(np.asarray(t, dtype=np.int32))
    return out


# ---- probes ---------------------------------------------------------------------------------------------------------------
def _probe_search(name):
    def probe(s):
        got, st = dk._search_raw(s.e, s.db[name], s.lib.swg_search, K)
        s.stats["search", name] = st
        s.same(got, want_search(name, s.state), "search[%s]" % name)
    return probe


def _probe_hits_only(name, kmer):
    """Hits and no scores, pruned wherever the plan allows it (prune 2: the size rule of prune 1 needs millions of
    sequences), by the bound the library picks or by the k-mer table of k = 4."""
    def probe(s):
        s.ctx.set_option("prune", 2)
        s.ctx.set_option("prune_kmer", 4 if kmer else 0)
        try:
            got, st = dk._search_raw(s.e, s.db[name], s.lib.swg_search, K, want_scores=False)
            s.stats["hits_only_kmer" if kmer else "hits_only", name] = dict(st, **s.ctx.prune_last())
        finally:
            s.ctx.set_option("prune_kmer", 0)
            s.ctx.set_option("prune", 1)
        s.same(got, want_search(name, s.state, scores=False), "hits_only%s[%s]" % ("_kmer" if kmer else "", name))
    return probe


def _probe_above(name):
    def probe(s):
        t = truth(name, *s.state)
        T = max(1, int(np.sort(t)[-10]))
        db = s.db[name]
        got = dk._above_raw(s.e, db, False, T, db.count + 1)
        want = _hits(amc.above(t, T))
        s.same(got, {"hits": want, "n_total": len(want), "tail": True}, "search_above[%s] at %d" % (name, T))
    return probe


def _probe_gapless(name):
    def probe(s):
        got, st = dk._search_raw(s.e, s.db[name], s.lib.swg_search_gapless, K)
        s.stats["search_gapless", name] = st
        s.same(got, want_search(name, s.state, gapless=True), "search_gapless[%s]" % name)
    return probe


def _probe_multi(name):
    def probe(s):
        fn = s.lib.swg_search_multi_pssm if s.pssm else s.lib.swg_search_multi
        got = dk._multi_raw(s.e, s.db[name], fn, s.pssm, K)
        ts = [truth(name, li, s.ci, s.si) for li in range(3)]
        want = {"scores": dk.ByIndex(np.stack(ts).astype(np.int32)), "hits": [_hits(amc.above(t, 1 - (1 << 30))[:K]) for t in ts], "tail": True}
        s.same(got, want, "search_multi[%s]" % name)
    return probe


def _probe_lists(name):
    def probe(s):
        lists = s.c["lists"][name, s.ci]
        got = dk._lists_raw(s.e, s.db[name], s.pssm, lists, K)
        ts = [truth(name, li, s.ci, s.si) for li in range(3)]
        want = {"scores": [np.asarray(t[l], dtype=np.int32) for t, l in zip(ts, lists)],
                "hits": [_hits(amc.above(t, 1 - (1 << 30), np.unique(l))[:K]) for t, l in zip(ts, lists)], "tail": True}
        s.same(got, want, "search_lists[%s]" % name)
    return probe


def _probe_align(call, mode):
    keys = {"hits": dk.ALN.names + ("ops",), "bounds": dk.ALN.names, "stats": dk.ALN.names + dk.CNT.names,
            "hsps": dk.ALN.names + dk.CNT.names + ("ops",)}[mode]

    def probe(s):
        row = hit_row(*s.state)
        got = dk._align_raw(s.e, s.db["world"], call, [row], mode, s.pssm, MAX_HSPS if mode == "hsps" else 0)
        if mode == "hsps":
            want = [[{k: a[k] for k in keys} for a in hsps(*s.state, i)] for i in row]
        else:
            want = [{k: trace(*s.state, i)[k] for k in keys} for i in row]
        s.same(got, {"rows": [want], "tail": True}, call)
    return probe


def _probe_pssm_build(s):
    got = dk._pssm_build_raw(s.e, s.db["world"], [hit_row(*s.state)], s.pssm, (s.li,))
    s.same(got, {"rows": [built_pssm(*s.state)]}, "swg_pssm_build")


def _probe_calibrate(s, seed=CALIB["calib_seed"]):
    """lambda, mu and K within evalue_cases.REL (the bound tests/test_gpu_calibrate.py holds them to), the rest equal."""
    got = s.ctx.calibrate()
    want, want_it = calibration(*s.state, seed)
    ec.assert_same(got, s.ctx.debug_calib_iters()[0], want, want_it, s.where("calibrate"))


PROBES = {}
for _name in DBS:
    PROBES["search[%s]" % _name] = _probe_search(_name)
    PROBES["hits_only[%s]" % _name] = _probe_hits_only(_name, False)
    PROBES["hits_only_kmer[%s]" % _name] = _probe_hits_only(_name, True)
    PROBES["search_above[%s]" % _name] = _probe_above(_name)
    PROBES["search_gapless[%s]" % _name] = _probe_gapless(_name)
    PROBES["search_multi[%s]" % _name] = _probe_multi(_name)
    PROBES["search_lists[%s]" % _name] = _probe_lists(_name)
PROBES["search[masked]"] = _probe_search("masked")
PROBES["align_hits"] = _probe_align("swg_align_hits", "hits")
PROBES["align_bounds"] = _probe_align("swg_align_bounds", "bounds")
PROBES["align_stats"] = _probe_align("swg_align_stats", "stats")
PROBES["align_hsps"] = _probe_align("swg_align_hsps", "hsps")
PROBES["pssm_build"] = _probe_pssm_build
PROBES["calibrate"] = _probe_calibrate
# the probes include/swg.h allows beside a search in flight: swg_search itself (every other family answers SWG_ERR_STATE)
IN_FLIGHT_OK = tuple(n for n in PROBES if n.startswith(("search[", "hits_only")))


# ---- movers ---------------------------------------------------------------------------------------------------------------
def _m_other_content(s):
    s.ci ^= 1
    s.apply_query()


def _m_pssm_or_index(s):
    s.pssm = not s.pssm
    s.apply_query()


def _m_next_length(s):
    s.li = (s.li + 1) % 3
    s.apply_query()


def _m_other_scoring(s):
    s.si ^= 1
    s.apply_scoring()


def _m_relatives(s):
    """Twice under BLOSUM62 -11/-1 (the first flags every pair and sets both hints, the second runs under the veto), once
    under the heavier table; then the session's own scoring and query again."""
    db, sub = s.db["relatives"], s.c["sub"]
    try:
        s.ctx.set_scoring(sub, *SCORINGS[0])
        s.ctx.set_query(s.c["qrel"])
        forms = []
        for n in range(2):
            got, st = dk._search_raw(s.e, db, s.lib.swg_search, K)
            forms.append((st["cell_form"], st["n_rescored"]))
            s.same(got["scores"], dk.ByIndex(relatives_truth(False).astype(np.int32)), "relatives, search %d" % n)
        s.evidence["relatives"] = forms
        s.ctx.set_scoring(s.c["heavy"], *SCORINGS[0])
        got, st = dk._search_raw(s.e, db, s.lib.swg_search, K)
        s.evidence["relatives, heavy"] = (st["cell_form"], st["n_rescored"])
        s.same(got["scores"], dk.ByIndex(relatives_truth(True).astype(np.int32)), "relatives, the heavier scoring")
    finally:
        s.apply_scoring()
        s.apply_query()


def _m_one_sequence(s):
    s.search("one", "a database of one sequence")


def _m_forced(route):
    def mover(s):
        opts = FORCED[route]
        for key, v in opts.items():
            s.ctx.set_option(key, v)
        try:
            st = s.search("world", route)
            s.evidence.setdefault(route, []).append({k: st[k] for k in ("engine", "passes", "long_pairs", "work_queue")})
            s.search("tunable", route)
        finally:
            for key in opts:
                s.ctx.set_option(key, 0)
    return mover


def _read_pruned(s):
    """A hits-only search of tunable under prune 2 -> what swg_prune_last and the test hooks say it ran."""
    keep = s.hits_alone
    s.ctx.set_option("prune", 2)
    s.hits_alone = True
    try:
        st = s.search("tunable", "hits only under prune 2")
        read = s.ctx.debug_prune_refine_read(s.db["tunable"])
        tables = s.ctx.debug_prune_tables()
        ev = dict(s.ctx.prune_last(), k=read["k"], segments=read["segments"], refine=read["refine"],
                  head_end=int(read["stages"][0][1]) if read["stages"] else 0, lists=[len(x[3]) for x in read["stages"]],
                  refine3=tables["refine3"], bits=tables["bits"], gate=s.ctx.debug_prune_gate(), refine4=s.ctx.debug_prune_tables4(),
                  refine5=s.ctx.debug_prune_tables5(), passes=st["passes"])
    finally:
        s.ctx.set_option("prune", 1)
        s.hits_alone = keep
    return ev


def _read_heavy(s):
    try:
        s.ctx.set_scoring(s.c["heavy"], *SCORINGS[0])
        s.ctx.set_query(s.c["qrel"])
        got, st = dk._search_raw(s.e, s.db["relatives"], s.lib.swg_search, K)
        s.same(got["scores"], dk.ByIndex(relatives_truth(True).astype(np.int32)), "relatives, the heavier scoring")
    finally:
        s.apply_scoring()
        s.apply_query()
    return st


def _read_above_multi(s):
    ts = [truth("tunable", li, s.ci, s.si) for li in range(3)]
    T = [max(1, int(np.sort(t)[-10])) for t in ts]
    fn = s.lib.swg_search_above_multi_pssm if s.pssm else s.lib.swg_search_above_multi
    got = dk._above_multi_raw(s.e, s.db["tunable"], fn, s.pssm, T, s.db["tunable"].count + 1)
    want = [_hits(amc.above(t, x)) for t, x in zip(ts, T)]
    s.same(got, {"hits": want, "n_total": [len(w) for w in want], "tail": True}, "search_above_multi[tunable]")
    return {}


def _plan_of(st):
    return {k: st[k] for k in PLAN_FIELDS + ("fill_launches", "last_pass_cols")}


READERS = {
    "search": lambda s: _plan_of(s.search("tunable", "search")),
    "int32": lambda s: _plan_of(s.search("tunable", "search under force_bits 32")),
    "several_pass": lambda s: _plan_of(s.search("world", "several passes")),
    "two_class": lambda s: _plan_of(s.search("world", "two classes")),
    "pruned": _read_pruned,
    "heavy": lambda s: _plan_of(_read_heavy(s)),
    "multi": lambda s: PROBES["search_multi[tunable]"](s) or {},
    "above_multi": _read_above_multi,
    "calibrate": lambda s: _probe_calibrate(s, seed=2) or {},
}


def _m_option(key, away, default, reader, beside):
    """The option away from its default, the options `beside` it set, the call that reads it, everything back."""
    def mover(s):
        for k, v in beside.items():
            s.option(k, v)
        s.option(key, away)
        try:
            s.evidence[key, away] = READERS[reader](s)
        finally:
            s.option(key, default)
            for k in beside:
                s.option(k, DEFAULTS.get(k, 0))
    return mover


def _m_fixed_streams(s):
    s.option("work_queue", 0)
    try:
        s.evidence["fixed streams"] = [_plan_of(s.search(name, "work_queue = 0")) for name in DBS]
    finally:
        s.option("work_queue", 1)


def _m_process_wide(key, away, default):
    def mover(s):
        if s.other is None:
            s.other = s.swg.Context(0)
        s.other.set_option(key, away)
        try:
            s.search("world", "%s = %d on a second context" % (key, away))
            s.search("tunable", "%s = %d on a second context" % (key, away))
        finally:
            s.other.set_option(key, default)
    return mover


def _m_ticket(s):
    s.begin_ticket()


def _m_refused_arg(s):
    """A hit outside the handle: SWG_ERR_ARG and nothing written."""
    got = dk._align_raw(s.e, s.db["world"], "swg_align_hits", [[dk.N + 5]], "hits", s.pssm)
    s.same(got, dk.refused_arg(s.swg), "swg_align_hits of a hit outside the handle")


def _m_refused_state(s):
    """A batch call while a ticket is out: SWG_ERR_STATE; the ticket's own answer afterwards."""
    s.begin_ticket()
    try:
        s.ctx.search_multi(s.db["tunable"], s.e.w["queries"], k=K)
        code = s.swg.SWG_OK
    except s.swg.SwgError as err:
        code = err.code
    assert code == s.swg.SWG_ERR_STATE, s.where("swg_search_multi beside a search in flight: %d" % code)
    s.end_ticket()


def _m_mask(s):
    m = s.db["world"].mask(s.ctx)
    try:
        dk._search_raw(s.e, m, s.lib.swg_search, K)
    finally:
        m.close()


def _m_view(s):
    for name in DBS:
        n = s.db[name].total_count
        v = s.db[name].view(s.ctx, np.arange(0, n, 3))
        try:
            got, _ = dk._search_raw(s.e, v, s.lib.swg_search, K)
            t = truth(name, *s.state)
            s.same(got["scores"], dk.ByIndex.of(n, np.arange(0, n, 3), t[::3]), "a view of every third of %s" % name)
        finally:
            v.close()


def _m_batches16(s):
    import swg_loader
    batches = swg_loader.oracle().db_to_batches16(*s.c["batches16"])
    s.ctx.fill_batches16([(b, 16) for b in batches])


MOVERS = {name: (lambda s, _n=name: PROBES[_n](s)) for name in PROBES}
MOVERS.update({
    "set_query: other content": _m_other_content, "set_query_pssm / set_query": _m_pssm_or_index, "set_query: next length": _m_next_length,
    "set_scoring: the other": _m_other_scoring, "search relatives": _m_relatives, "search one sequence": _m_one_sequence,
    "two-class search": _m_forced("two_class"), "several-pass search": _m_forced("several_pass"), "systolic search": _m_forced("systolic"),
    "fixed-streams search": _m_fixed_streams,
    "search_begin, ticket left out": _m_ticket, "refused: a hit outside the handle": _m_refused_arg,
    "refused: a batch beside a ticket": _m_refused_state, "db.mask and close": _m_mask, "db.view and close": _m_view,
    "fill_batches16": _m_batches16,
})
OPTION_MOVERS = {"%s = %d" % m[:2]: m for m in OPTION_MOVES}
for _name, _m in OPTION_MOVERS.items():
    MOVERS[_name] = _m_option(*_m)
for _key, _away, _default in PROCESS_WIDE:
    MOVERS["%s = %d" % (_key, _away)] = _m_process_wide(_key, _away, _default)
# the movers that change what the session holds: a probe runs in front of each of them too, so that whatever the probe
# remembered is remembered under the state the mover leaves behind
STATE_MOVERS = ("set_query: other content", "set_query_pssm / set_query", "set_query: next length", "set_scoring: the other")


def reset_process_wide(swg):
    """long_cols and long_group back to 0, whatever a failing test left."""
    c = swg.Context(0)
    try:
        for key, _, default in PROCESS_WIDE:
            c.set_option(key, default)
    finally:
        c.close()


def walk(s, rng, steps):
    """`steps` calls drawn from the movers and the probes; every probe compared with the truth."""
    movers, probes = sorted(MOVERS), sorted(PROBES)
    for _ in range(steps):
        if rng.random() < 0.5:
            s.run_probe(probes[int(rng.integers(len(probes)))])
        else:
            s.run_mover(movers[int(rng.integers(len(movers)))])
