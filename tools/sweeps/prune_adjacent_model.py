"""The host model of a fifth pruning level -- the fourth level's walk with the query columns jumped over between two blocks
charged as a gap (profiles/prune_adjacent_ab.txt, section 0).  No GPU.

    python tools/sweeps/prune_adjacent_model.py [--nseq N] [--threshold T] [--explicit N ...]

The sequences, query, pairing, threshold and unpruned first stage of tools/sweeps/prune_deep_model.py and
prune_gate_model.py.  A pair's bound is the least of the four levels' mirrors and the new one
(swg_debug_prune_kmer_refine5), which runs on the pairs the fourth level leaves at or above T, in the first stage and
behind it, the shorter sequence padded to the pair's length as the device pads it.  The new mirror is run in its exact
form (every number of segments between two chains' ends taken one by one) and with the first N taken one by one and the
rest through two prefix maxima, for each N asked for: the form a kernel would compute.  rows_kept_frac is the share of the
pair rows still filled: the first stage whole and the pairs behind it whose bound reaches T."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import swg_loader  # noqa: E402

swg = swg_loader.load()

HEADLINE_ROWS = 1938193684            # pair rows of the headline (swg_prune_last)
HEADLINE_BLOCKS = HEADLINE_ROWS // 4  # ... and its token blocks
SEGMENT_BLOCKS = (1 << 26) - 64       # of one launch segment (SWG_DYN_SEG_BLOCKS)
LQ = 3000
GO_AHEAD = 0.155                      # the most rows the kernel's form may keep for the level to be worth building


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nseq", type=int, default=200000)
    ap.add_argument("--threshold", type=int, default=2466)
    ap.add_argument("--explicit", type=int, nargs="*", default=[1, 2, 4, swg.REFINE5_EXPLICIT])
    a = ap.parse_args()
    seed = 0x5EED0004
    q = swg.synth_query(seed, LQ)
    sh = swg.synth_db_shard(seed, a.nseq, 0, 1, query=None, fraction=0.0, subst=0.05)
    flat, off = sh["flat"], sh["offsets"].astype(np.int64)
    sub = np.asarray(swg.load_scoring("BLOSUM62").table(), dtype=np.int8).reshape(32, 32)
    lens = np.diff(off)
    order = np.argsort(-lens, kind="stable")
    if len(order) & 1:
        order = order[:-1]
    x, y = order[0::2], order[1::2]
    blocks = (2 + lens[x] + 3) // 4          # (the longer sequence of the pair)
    head = int(np.searchsorted(np.cumsum(blocks), blocks.sum() * SEGMENT_BLOCKS / HEADLINE_BLOCKS))
    T = a.threshold
    rows = blocks.astype(np.float64)
    behind = np.arange(len(x)) >= head

    def pair(u):
        u = u.astype(np.int64)
        return np.maximum(u[x], u[y])

    def padded(walk):
        seqs, offs = [], [0]
        for p in walk:
            lx = int(lens[x[p]])
            for s in (x[p], y[p]):
                r = np.zeros(lx, dtype=np.int8)
                r[:lens[s]] = flat[off[s]:off[s + 1]]
                seqs.append(r)
                offs.append(offs[-1] + lx)
        return np.concatenate(seqs), np.array(offs, dtype=np.uint64)

    def kept(bound):
        return round(float(rows[(bound >= T) | ~behind].sum() / rows.sum()), 4)

    bound = pair(swg.debug_prune_kmer_seg(sub, q, -2, -1, 4, 32, flat, off, table=False)[1])
    for S in (128, 256):
        bound = np.minimum(bound, pair(swg.debug_prune_kmer_refine(sub, q, -2, -1, S, flat, off, table=False)[1]))
    walk = np.nonzero(bound >= T)[0]
    f4, o4 = padded(walk)
    u4 = swg.debug_prune_kmer_refine4(sub, q, -2, -1, 256, f4, o4).astype(np.int64)
    four = bound.copy()
    four[walk] = np.minimum(bound[walk], np.maximum(u4[0::2], u4[1::2]))
    walk5 = np.nonzero(four >= T)[0]
    f5, o5 = padded(walk5)
    band = behind & (four >= T)
    out = {"nseq": a.nseq, "threshold": T, "pairs": len(x), "head_pairs": head, "head_shortest_rows": int(lens[x[head - 1]]) if head else 0,
           "rows_first_stage_share": round(float(rows[:head].sum() / rows.sum()), 4),
           "four_levels": {"rows_kept_frac": kept(four), "band_rows_share": round(float(rows[band].sum() / rows.sum()), 4),
                           "band_shortest_rows": int(lens[x[band]].min()) if band.any() else 0},
           "pairs_walked_by_the_fifth": len(walk5), "forms": []}
    exact = None
    for N in [256] + [n for n in a.explicit if n < 256]:
        u5 = swg.debug_prune_kmer_refine5(sub, q, -2, -1, 256, f5, o5, explicit=N).astype(np.int64)
        five = four.copy()
        five[walk5] = np.minimum(four[walk5], np.maximum(u5[0::2], u5[1::2]))
        assert np.all(np.maximum(u5[0::2], u5[1::2]) <= np.maximum(u4[0::2], u4[1::2])[four[walk] >= T])
        if exact is None:
            exact = five
        assert np.all(five >= exact)      # (a relaxed form is never below the exact one)
        left = behind & (five >= T)
        out["forms"].append({
            "explicit": "exact" if N >= 256 else N, "rows_kept_frac": kept(five), "within_of_exact": round(kept(five) - kept(exact), 4),
            "band_rows_share": round(float(rows[left].sum() / rows.sum()), 4), "band_shortest_rows": int(lens[x[left]].min()) if left.any() else 0,
            "first_stage_pairs_below_T": int(np.sum(five[:head] < T)),
            "first_stage_rows_below_T_share": round(float(rows[:head][five[:head] < T].sum() / rows.sum()), 4),
            "bound_per_row_1040_to_1139": round(float(np.median((five / lens[x])[(lens[x] >= 1040) & (lens[x] <= 1139)])), 3),
            "go_on": bool(kept(five) <= GO_AHEAD)})
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
