"""The host model of the headline's pruned search, level by level (profiles/prune_bytes_ab.txt, section 0).  No GPU.

    python tools/sweeps/prune_bytes_model.py [--nseq N] [--threshold T]

N sequences (default 1M) of the headline's generator and its 3000-column query under BLOSUM62, gaps -2 / -1, paired in
length order the way the database pairs them; the host mirrors of the first level (k = 4 in 32 segments), the second
(128 segments) and the third (256); the final threshold of the headline, T = 2466; the first stage -- the longest pairs,
as many token blocks of the whole as one launch segment is of the headline's -- unpruned.  Prints the share of the pair
rows each level keeps: a pair is filled where the least of its bounds so far reaches T."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import swg_loader  # noqa: E402

swg = swg_loader.load()

HEADLINE_BLOCKS = 1938193684 // 4     # token blocks of the headline's pairs (swg_prune_last: pair_rows)
SEGMENT_BLOCKS = (1 << 26) - 64       # of one launch segment (SWG_DYN_SEG_BLOCKS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nseq", type=int, default=1000000)
    ap.add_argument("--lq", type=int, default=3000)
    ap.add_argument("--threshold", type=int, default=2466)
    a = ap.parse_args()
    seed = 0x5EED0004
    q = swg.synth_query(seed, a.lq)
    sh = swg.synth_db_shard(seed, a.nseq, 0, 1, query=None, fraction=0.0, subst=0.05)
    flat, off = sh["flat"], sh["offsets"]
    sub = np.asarray(swg.load_scoring("BLOSUM62").table(), dtype=np.int8).reshape(32, 32)
    lens = np.diff(off.astype(np.int64))
    order = np.argsort(-lens, kind="stable")
    if len(order) & 1:
        order = order[:-1]
    x, y = order[0::2], order[1::2]
    blocks = (2 + lens[x] + 3) // 4          # (the longer sequence of the pair)
    head = int(np.searchsorted(np.cumsum(blocks), blocks.sum() * SEGMENT_BLOCKS / HEADLINE_BLOCKS))
    kept = np.ones(len(x), dtype=bool)
    bound = None
    for name, S in (("first, 32 segments", 32), ("second, 128 segments", 128), ("third, 256 segments", 256)):
        if S == 32:
            _, u = swg.debug_prune_kmer_seg(sub, q, -2, -1, 4, 32, flat, off, table=False)
        else:
            _, u = swg.debug_prune_kmer_refine(sub, q, -2, -1, S, flat, off, table=False)
        u = u.astype(np.int64)
        pair = np.maximum(u[x], u[y])
        bound = pair if bound is None else np.minimum(bound, pair)
        kept = bound >= a.threshold
        kept[:head] = True
        print(json.dumps({"level": name, "nseq": a.nseq, "threshold": a.threshold, "head_pairs": head, "pairs": len(x),
                          "rows_kept_frac": round(float(blocks[kept].sum()) / float(blocks.sum()), 4)}), flush=True)


if __name__ == "__main__":
    main()
