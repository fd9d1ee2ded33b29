"""The cases of the composition-based score adjustment's tests (swg_comp_adjust*): seeded, small, no fixture
file.  A case is one query (index query or PSSM) under one scoring system, background and scale F, with its subject
sequences and the hit list the calls get (indices into the subjects; may repeat).  `expect` names what the numpy model
(comp_model.py) must give for every hit of the case -- test_comp_host.py asserts it, so a seed that stops delivering
it fails there and is replaced, never exempted:
    floor     status 0 and ratio16 == 32768          cap      status 0 and ratio16 == 65536
    between   status 0 and 32768 < ratio16 < 65536   none     status 1 (no adjustment)
The instantiation cases hold, for every (G, K) class of the fill kernel and each of its edge lengths, subjects of 1, 2
and G + 3 residues and one subject per lane-local column k whose best cells all lie in columns = k mod K (a copy of the
query's residues in front of such a column: test_comp_host.py proves it with the model)."""
import functools

import numpy as np

import pssm_build_cases as pc

CLASSES = ((16, 4), (16, 8), (32, 8), (64, 8), (64, 16), (64, 32))    # the fill kernel's (G, K), narrowest first
COLS = 2048                                                          # its column limit
SCALES = (1, 2, 32, 64)
STD = np.array([pc.idx(ch) for ch in pc.STANDARD], dtype=np.int8)
X = pc.idx("X")
SEED = 20260


def _rng(*key):
    return np.random.default_rng([SEED] + [int(k) for k in key])


def _p_background():
    f = pc.builtin_freq()[STD.astype(np.int64)]
    return f / f.sum()


def background_seq(rng, n):
    return STD[rng.choice(20, size=n, p=_p_background())]


def biased_seq(rng, n, rich, share):
    """n residues: with probability `share` one of the letters `rich` (uniform), else a draw from the background."""
    out = background_seq(rng, n)
    pick = rng.random(n) < share
    out[pick] = np.array([pc.idx(ch) for ch in rich], dtype=np.int8)[rng.integers(0, len(rich), size=int(pick.sum()))]
    return out


def shuffled_composition(rng, n, rich, share):
    """A shuffle of a fixed biased composition: exactly round(share n) residues of `rich`, dealt evenly, the rest background."""
    m = int(round(share * n))
    head = np.array([pc.idx(rich[i % len(rich)]) for i in range(m)], dtype=np.int8)
    out = np.concatenate([head, background_seq(rng, n - m)])
    rng.shuffle(out)
    return out


def pssm31(rng, lq, lo=-128, hi=127):
    """A random position-specific query of at most 31 distinct columns -> (pssm[lq, 32], q', sub'): the construction of
    tests/test_gpu_pssm.py, so the oracle can score it as the index query q' under sub'."""
    subp = np.zeros((32, 32), dtype=np.int8)
    subp[1:, 1:] = rng.integers(lo, hi + 1, size=(31, 31))
    qp = rng.integers(1, 32, size=lq).astype(np.int8)
    return subp[qp.astype(np.int64)], qp, subp


def _case(name, seqs, gaps=(-11, -1), sub="BLOSUM62", query=None, pssm=None, freq=None, F=32, hits=None, expect=None, **extra):
    c = dict(name=name, sub=pc.table(sub) if isinstance(sub, str) else sub, gap_open=gaps[0], gap_extend=gaps[1], query=query, pssm=pssm,
             freq=freq, F=F, seqs=[np.asarray(s, dtype=np.int8) for s in seqs], expect=expect)
    c["hits"] = list(range(len(seqs))) if hits is None else list(hits)
    c.update(extra)
    assert len(c["hits"]) <= 64 and (query is None) != (pssm is None)
    return c


QEK, OPPOSITE = "QEK", "LIVFWCM"
UNBIASED_BETWEEN = (1, 5, 10, 13, 16, 18, 21, 23)


def qek_query():
    return biased_seq(_rng(1), 120, QEK, 0.35)


def bias_cases():
    q = qek_query()
    same = [shuffled_composition(_rng(2, i), 150 + 30 * i, QEK, 0.35) for i in range(8)]
    opposite = [biased_seq(_rng(3, i), 150 + 30 * i, OPPOSITE, 0.6) for i in range(8)]
    mild = [shuffled_composition(_rng(4, i), 150 + 30 * i, QEK, 0.10) for i in range(8)]
    zero_l = pc.builtin_freq()
    zero_l[pc.idx("L")] = 0.0
    cases = [
        _case("qek_same_bias", same, query=q, expect="floor", hits=list(range(8)) + [3, 3]),          # (a hit listed three times)
        _case("qek_opposite_bias", opposite, query=q, expect="cap"),
        _case("x_only_subject", [np.full(40, X, dtype=np.int8), np.full(1, X, dtype=np.int8)], query=q, expect="none"),
        _case("freq_zero_weight", mild + [np.full(30, pc.idx("L"), dtype=np.int8)], query=q, freq=zero_l, expect=None),
    ]
    cases += [_case("qek_mild_bias_F%d" % F, mild, query=q, F=F, expect="between") for F in SCALES]
    # unbiased on both sides: a background query against draws from the background.  Such a subject's lambda lands on
    # either side of lambda_std (about half of all draws exceed it and meet the cap); UNBIASED_BETWEEN names the draws of
    # this seed that fall short of it, which is the half the "between" expectation is about.
    qb = background_seq(_rng(16), 150)
    cases.append(_case("unbiased_between", [background_seq(_rng(17, i), 200 + 5 * i) for i in UNBIASED_BETWEEN], query=qb, expect="between"))
    return cases


def gap_cases():
    q = background_seq(_rng(5), 48)
    seqs = [background_seq(_rng(6, i), 20 + 7 * i) for i in range(6)] + [q[5:40].copy()]
    return [_case("gaps_%d_%d_F%d" % (go, ge, F), seqs, gaps=(go, ge), query=q, F=F)
            for go, ge in ((0, 1), (2, 3), (0, 0), (1, -3), (-1, 0)) for F in (1, 32)]


def pssm_cases():
    b62 = pc.table("BLOSUM62")
    w = pc.idx("W")
    all_w = np.full(40, w, dtype=np.int8)
    q_w = np.where(_rng(7).random(60) < 0.5, w, background_seq(_rng(7, 1), 60)).astype(np.int8)
    bg = [background_seq(_rng(8, i), 90 + 40 * i) for i in range(4)]
    full = np.clip(np.rint(_rng(9).normal(-25.0, 55.0, size=(64, 32))), -128, 127).astype(np.int8)
    full[0, 1], full[1, 2] = 127, -128
    no_pos = np.minimum(full, 0).astype(np.int8)
    p31, qp, subp = pssm31(_rng(10), 70)
    p31s, qps, subps = pssm31(_rng(11), 70, lo=-9, hi=6)
    any31 = [_rng(12, i).integers(1, 32, size=50 + 25 * i).astype(np.int8) for i in range(5)]
    cases = [
        # lambda_std exists (the W rows against the background), lambda_hit against the all-W subject does not
        _case("pssm_positive_against_subject", [all_w], pssm=b62[q_w.astype(np.int64)], expect="none"),
        _case("pssm_as_index_query", bg, pssm=b62[q_w.astype(np.int64)], index_form=(q_w, b62)),
        _case("pssm_no_positive_entry", bg[:2], pssm=no_pos, expect="none"),
        _case("pssm_full_int8", bg + [all_w], pssm=full),
    ]
    for F in (1, 32):
        every = np.ones(32)
        every[0] = 0.0
        cases.append(_case("pssm31_wide_F%d" % F, any31, pssm=p31, F=F, freq=every, index_form=(qp, subp)))
        cases.append(_case("pssm31_narrow_F%d" % F, any31, pssm=p31s, F=F, freq=every, index_form=(qps, subps), gaps=(-5, -1)))
    return cases


def class_lengths(G, K):
    return ((G - 1) * K + 1, G * K - 1, G * K)


def class_of(lq):
    return next((i for i, (G, K) in enumerate(CLASSES) if lq <= G * K), -1)


def _instantiation(G, K, lq, pssm):
    rng = _rng(13, G, K, lq, pssm)
    q = background_seq(rng, lq)
    seqs = [background_seq(rng, n) for n in (1, 2, G + 3)]
    pinned = {}
    for k in range(min(K, lq)):
        e = (lq - 1 - k) // K * K + k                     # the last column of lane-local index k
        seqs.append(q[max(0, e - 5):e + 1].copy())
        pinned[k] = len(seqs) - 1
    kw = dict(pssm=pc.table("BLOSUM62")[q.astype(np.int64)], index_form=(q, pc.table("BLOSUM62"))) if pssm else dict(query=q)
    return _case("inst_G%d_K%d_lq%d_%s" % (G, K, lq, "pssm" if pssm else "index"), seqs, G=G, K=K, pinned=pinned, **kw)


def instantiation_cases():
    cases = [_instantiation(16, 4, 1, False), _instantiation(16, 4, 1, True)]
    for G, K in CLASSES:
        for lq in class_lengths(G, K):
            # the two forms are instantiations of their own, with their own table paths: both at all three lengths
            cases += [_instantiation(G, K, lq, f) for f in (False, True)]
    return cases


def limit_cases():
    d = [background_seq(_rng(14), 64)]
    out = []
    for lq in (COLS, COLS + 1):
        q = background_seq(_rng(15, lq), lq)
        out.append(_case("limit_lq%d_index" % lq, d, query=q, over=lq > COLS))
        out.append(_case("limit_lq%d_pssm" % lq, d, pssm=pc.table("BLOSUM62")[q.astype(np.int64)], over=lq > COLS, index_form=(q, pc.table("BLOSUM62"))))
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = bias_cases() + gap_cases() + pssm_cases() + instantiation_cases() + limit_cases()
    names = [c["name"] for c in cases]
    assert len(names) == len(set(names))
    return tuple(cases)


def lq_of(c):
    return len(c["query"]) if c["query"] is not None else c["pssm"].shape[0]


def database(c):
    """(flat, offsets) of a case's subjects, as swg.Database takes them."""
    off = np.zeros(len(c["seqs"]) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in c["seqs"]])
    return np.concatenate(c["seqs"]).astype(np.int8), off
