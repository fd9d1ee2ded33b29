"""The host model of the gate in front of the first pruning level (profiles/prune_gate_ab.txt, section 0).  No GPU.

    python tools/sweeps/prune_gate_model.py [--nseq N] [--threshold T]

The sequences, query, pairing, threshold and unpruned first stage of tools/sweeps/prune_deep_model.py.  Two questions:

  * how much of the first level's walk is left: the gated launch runs behind the first stage and walks a pair only where
    U_1 = max(U_1x, U_1y), the colmax sum (swg_debug_prune_bound), reaches T.  walked_share_of_all is the pair rows it still
    walks over the rows of all pairs -- the ungated launch walks all of them, so the walk's time is predicted to fall to
    that share; walked_share_behind_head is the same over the rows behind the first stage.
  * whether a shorter first stage (or cutting the first stage under a T found earlier) could save anything: the pairs of the
    first stage whose bound -- the least of the four levels' mirrors -- is below T.  None: the first stage stays whole.

The fourth level's mirror runs on the pairs the three levels of k = 4 leave at or above T, as the device walks them (the
shorter sequence padded to the pair's length), in the first stage and behind it."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nseq", type=int, default=200000)
    ap.add_argument("--threshold", type=int, default=2466)
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

    u1 = pair(swg.debug_prune_bound(sub, q, flat, off)[1])
    bound = pair(swg.debug_prune_kmer_seg(sub, q, -2, -1, 4, 32, flat, off, table=False)[1])
    assert np.all(bound <= u1)    # (a block adds the lesser of its entry and its colmax sum)
    first = bound.copy()
    for S in (128, 256):
        bound = np.minimum(bound, pair(swg.debug_prune_kmer_refine(sub, q, -2, -1, S, flat, off, table=False)[1]))
    walk = np.nonzero(bound >= T)[0]
    seqs, offs = [], [0]
    for p in walk:
        lx = int(lens[x[p]])
        for s in (x[p], y[p]):
            r = np.zeros(lx, dtype=np.int8)
            r[:lens[s]] = flat[off[s]:off[s + 1]]
            seqs.append(r)
            offs.append(offs[-1] + lx)
    u4 = swg.debug_prune_kmer_refine4(sub, q, -2, -1, 256, np.concatenate(seqs), np.array(offs, dtype=np.uint64)).astype(np.int64)
    final = bound.copy()
    final[walk] = np.minimum(bound[walk], np.maximum(u4[0::2], u4[1::2]))
    walked = behind & (u1 >= T)
    kept = (final >= T) | ~behind
    longest = np.argsort(-rows, kind="stable")[:max(1, len(x) // 100)]
    print(json.dumps({
        "nseq": a.nseq, "threshold": T, "pairs": len(x), "head_pairs": head, "head_shortest_rows": int(lens[x[head - 1]]) if head else 0,
        "rows_first_stage_share": round(float(rows[:head].sum() / rows.sum()), 4),
        "rows_u1_reaches_T_share_of_all": round(float(rows[u1 >= T].sum() / rows.sum()), 4),
        "walked_share_of_all": round(float(rows[walked].sum() / rows.sum()), 4),
        "walked_share_behind_head": round(float(rows[walked].sum() / rows[behind].sum()), 4),
        "pairs_left_at_gate_share": round(float(np.sum(behind & (u1 < T))) / float(behind.sum()), 4),
        "gate_changes_no_list": bool(np.all(first[behind & (u1 < T)] < T)),
        "first_stage_pairs_below_T": {"first_level": int(np.sum(first[:head] < T)), "three_levels": int(np.sum(bound[:head] < T)),
                                      "four_levels": int(np.sum(final[:head] < T))},
        "first_stage_rows_below_T_share": round(float(rows[:head][final[:head] < T].sum() / rows.sum()), 4),
        "least_final_bound_of_longest_percent": int(final[longest].min()),
        "final_bound_per_row_of_longest_percent": round(float(np.median(final[longest] / (4.0 * rows[longest]))), 2),
        "rows_kept_frac": round(float(rows[kept].sum() / rows.sum()), 4)}), flush=True)


if __name__ == "__main__":
    main()
