"""Inputs of the masking tests (test_mask_host.py, test_gpu_mask.py, the tool's tests): generated here, no fixtures.

reference_mask is an independent numpy restatement of the rule of include/swg.h: it builds T and the thresholds itself,
RECOUNTS every window (no sliding), finds the maximal runs of window starts low at K2, keeps those with a start low at K1
and covers [s, s + W) of every kept start.  The library's twin (swg.seg_mask) is compared against it on the CPU, the
device against the twin on the GPU."""
import numpy as np

X, B, Z, STAR = 24, 2, 26, 31
# the 20 standard amino acids as table indices (A = 1 .. Z = 26)
STANDARD = np.array([1, 18, 14, 4, 3, 17, 5, 7, 8, 9, 12, 11, 13, 6, 16, 19, 20, 23, 25, 22], dtype=np.int8)
DEFAULT = dict(window=12, trigger=2.2, extend=2.5, replace=X)
PARAM_SETS = {
    "default": DEFAULT,
    "w4": dict(window=4, trigger=0.9, extend=1.6, replace=X),
    "w64": dict(window=64, trigger=3.0, extend=3.9, replace=X),
    "k1_eq_k2": dict(window=12, trigger=2.5, extend=2.5, replace=X),
    "replace_A": dict(window=12, trigger=2.2, extend=2.5, replace=1),
}
BOUNDARIES = (64, 128, 256, 1024, 4096)          # the lengths of the structural cases, taken as positions
LENGTHS = (0, 1, 11, 12, 13, 14, 23, 30, 63, 64, 65, 66, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097)
LONG = 70001


def tables(window, trigger, extend):
    c = np.arange(1, window + 1, dtype=np.float64)
    T = np.zeros(65, dtype=np.int64)
    T[1:window + 1] = np.rint(c * np.log2(c) * 65536.0).astype(np.int64)
    thr = [int(np.ceil(window * (np.log2(float(window)) - k) * 65536.0)) for k in (trigger, extend)]
    return T, thr[0], thr[1]


def window_flags(seq, window=12, trigger=2.2, extend=2.5, **_):
    """(low at K1, low at K2) per window start, every window recounted."""
    seq = np.asarray(seq, dtype=np.int64)
    nw = len(seq) - window + 1
    if nw <= 0:
        return np.zeros(0, dtype=bool), np.zeros(0, dtype=bool)
    T, thr1, thr2 = tables(window, trigger, extend)
    win = np.lib.stride_tricks.sliding_window_view(seq, window)
    S = np.zeros(nw, dtype=np.int64)
    for a in range(32):
        S += T[(win == a).sum(axis=1)]
    return S >= thr1, S >= thr2


def runs_of(flags):
    """[(begin, end)] of the maximal runs of True, end exclusive."""
    f = np.concatenate([[0], np.asarray(flags, dtype=np.int8), [0]])
    d = np.diff(f)
    return list(zip(np.flatnonzero(d == 1).tolist(), np.flatnonzero(d == -1).tolist()))


def reference_mask(seq, window=12, trigger=2.2, extend=2.5, **_):
    """-> (bool mask, kept runs of window starts as [(begin, end)])."""
    low1, low2 = window_flags(seq, window, trigger, extend)
    mask = np.zeros(len(seq), dtype=bool)
    kept = []
    for b, e in runs_of(low2):
        if low1[b:e].any():
            kept.append((b, e))
            mask[b:e - 1 + window] = True
    return mask, kept


def apply_mask(seq, mask, replace=X, **_):
    return np.where(mask, np.int8(replace), np.asarray(seq, dtype=np.int8)).astype(np.int8)


# ---- building blocks ---------------------------------------------------------------------------------------------------
def high(n, phase=0):
    """n residues in which every window of up to 20 holds distinct letters: never low."""
    return STANDARD[(np.arange(n) + phase) % 20]


# a period of 12 with residue counts 3, 3, 2, 2, 1, 1 (entropy 2.459: low at 2.5, not at 2.2), its singleton first
PERIOD = np.array([6, 1, 1, 1, 4, 4, 4, 3, 3, 5, 5, 7], dtype=np.int8)


def middle(n):
    return np.tile(PERIOD, n // 12 + 1)[:n]


def first_trigger(n_windows):
    """A run of n_windows starts, all low at K2, whose ONLY start low at K1 is the first: the period with its leading
    singleton turned into a fourth A (counts 4, 3, 2, 2, 1: weight 1098048 against the threshold 1089179)."""
    s = middle(n_windows + 11).copy()
    s[0] = 1
    return s


def homopolymer(n, a=17):
    return np.full(n, a, dtype=np.int8)


def one_window_gap():
    """Two kept runs with exactly one window between them that is not low.  Three consecutive windows of 14 residues:
    counts 3, 3, 2, 2, 1, 1 (weight 885376, low at K2), then one of the threes leaves and a new letter enters (3, 2, 2, 2,
    1, 1, 1: 704832, not low), then a singleton leaves and a fourth A enters (4, 2, 2, 2, 1, 1: 917504, low again).  A's
    on both sides take each run down to a trigger."""
    a, b, c, d, e, f, g = 1, 3, 4, 5, 6, 7, 8
    core = [b, e, a, c, a, d, b, c, a, d, b, f, g, a]
    return np.array([a] * 12 + core + [a] * 12, dtype=np.int8)


def has_one_window_gap(low1, low2):
    kept = [(b, e) for b, e in runs_of(low2) if low1[b:e].any()]
    return any(b2 - e1 == 1 for (_, e1), (b2, _) in zip(kept, kept[1:]))


def straddlers():
    """One long sequence that is never low but for a homopolymer of 30 across each boundary position."""
    s = high(BOUNDARIES[-1] + 200).copy()
    for p in BOUNDARIES:
        s[p - 15:p + 15] = 17
    return s


def structural_cases(seed=3):
    """{name: sequence} -- the lengths at which the kernels change path, random over few letters (rich in runs, triggers
    and near misses) and as homopolymers; the planted runs; the letters X, B, Z and *."""
    rng = np.random.default_rng(seed)
    cases = {}
    for n in LENGTHS:
        cases["few%d" % n] = rng.integers(1, 2 + rng.integers(2, 6), size=n).astype(np.int8)
        cases["iid%d" % n] = STANDARD[rng.integers(0, 20, size=n)]
        if n in (12, 13, 64, 65, 1025, 4097):
            cases["homo%d" % n] = homopolymer(n)
    cases["few%d" % LONG] = rng.integers(1, 5, size=LONG).astype(np.int8)
    cases["homo%d" % LONG] = homopolymer(LONG)
    cases["first_trigger"] = first_trigger(100)
    cases["last_trigger"] = first_trigger(100)[::-1].copy()
    cases["first_trigger_in_high"] = np.concatenate([first_trigger(100), high(40)])
    cases["last_trigger_in_high"] = np.concatenate([high(40), first_trigger(100)[::-1]])
    cases["stretch5000_first"] = first_trigger(5000)
    cases["stretch5000_last"] = first_trigger(5000)[::-1].copy()
    cases["stretch5000_none"] = middle(5011)
    cases["one_window_gap"] = one_window_gap()
    cases["straddlers"] = straddlers()
    odd = rng.choice(np.array([X, B, Z, STAR, 1, 17], dtype=np.int8), size=300)
    cases["xbz_star"] = odd
    cases["x_run"] = np.concatenate([high(30), homopolymer(25, X), high(30), homopolymer(25, STAR), high(7)])
    return cases


def flat_of(seqs):
    seqs = [np.asarray(s, dtype=np.int8) for s in seqs]
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    flat = np.concatenate(seqs) if seqs else np.zeros(0, dtype=np.int8)
    return (flat if flat.size else np.zeros(1, dtype=np.int8)), off


# ---- the end-to-end case ------------------------------------------------------------------------------------------------
E2E_SEED = 3
N_IID, N_DECOY, N_REL = 300, 20, 5
Q, E = 17, 5
# a letter distribution close to Swiss-Prot's over the 20 standard amino acids (A R N D C Q E G H I L K M F P S T W Y V)
BACKGROUND = np.array([8.25, 5.53, 4.06, 5.45, 1.37, 3.93, 6.75, 7.07, 2.27, 5.96, 9.66, 5.84, 2.42, 3.86, 4.70, 6.56, 5.34, 1.08, 2.92, 6.87])


def _iid(rng, n):
    return STANDARD[rng.choice(20, size=n, p=BACKGROUND / BACKGROUND.sum())]


def _qe(rng, n):
    return np.where(rng.random(n) < 0.5, Q, E).astype(np.int8)


def end_to_end(seed=E2E_SEED):
    """-> dict(query, seqs, decoys, relatives): a query of 200 with a 30-residue Q/E stretch at 60..90; 300 iid sequences;
    20 decoys, iid but for a 40-residue Q/E-rich run; 5 relatives, iid flanks around a copy of query[110:170] in which 60 %
    of the positions were redrawn (about 40 % identity).  Decoys and relatives are dealt among the iid sequences."""
    rng = np.random.default_rng(1000 + seed)
    query = _iid(rng, 200)
    query[60:90] = _qe(rng, 30)
    seqs = [_iid(rng, int(rng.integers(150, 400))) for _ in range(N_IID)]
    decoys, relatives = [], []
    for _ in range(N_DECOY):
        s = _iid(rng, int(rng.integers(150, 400)))
        at = int(rng.integers(0, len(s) - 40))
        s[at:at + 40] = _qe(rng, 40)
        decoys.append(s)
    for _ in range(N_REL):
        core = query[110:170].copy()
        redraw = rng.random(60) < 0.6
        core[redraw] = _iid(rng, int(redraw.sum()))
        relatives.append(np.concatenate([_iid(rng, int(rng.integers(50, 150))), core, _iid(rng, int(rng.integers(50, 150)))]))
    everything = seqs + decoys + relatives
    perm = rng.permutation(len(everything))
    out = [everything[i] for i in perm]
    where = np.argsort(perm)
    return dict(query=query, seqs=out, decoys=set(int(v) for v in where[N_IID:N_IID + N_DECOY]),
                relatives=set(int(v) for v in where[N_IID + N_DECOY:]))


def iid_database(n=400, seed=1, lo=20, hi=400):
    """n sequences of lo..hi residues, iid from BACKGROUND."""
    rng = np.random.default_rng(seed)
    return [_iid(rng, int(rng.integers(lo, hi + 1))) for _ in range(n)]


def top_hits(scores, k):
    """The library's order: higher score first, ties by lower index -> [(score, index)]."""
    return [(-s, i) for s, i in sorted((-int(v), i) for i, v in enumerate(scores))[:k]]
