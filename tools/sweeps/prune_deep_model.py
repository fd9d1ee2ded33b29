"""The host model of a fourth pruning level -- blocks of 5 residues over 128 or 256 segments -- behind the headline's
three (profiles/prune_deep_ab.txt, section 0).  No GPU.

    python tools/sweeps/prune_deep_model.py [--nseq N] [--threshold T]

The sequences, query, pairing, threshold and unpruned first stage of tools/sweeps/prune_bytes_model.py; the mirrors of
the first level (k = 4 in 32 segments), the second (128) and the third (256), then the mirror of the new level
(swg_debug_prune_kmer_refine4) on the pairs the levels in front of it leave at or above T, the shorter sequence of a pair
padded to the longer one's length as the device pads it (a block of 5 lies where the PAIR's token blocks put it).  Three
candidates: (5, 128) and (5, 256) behind the third level, and (5, 256) behind the second with the third left out.  Each
is priced by the rule of the other levels: the table's build and the walk may cost at most half of what the cut saves."""
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
TABLE_RATE = 4.6e12                   # SWG_KMER_TABLE_RATE: the table kernel's cell updates per second
FILL_ROW = 1239.98e-3 / HEADLINE_ROWS  # the unpruned headline per pair row (profiles/prune_bytes_ab.txt, section 2)
WALK_ROW = 1.74e-12                   # the third level's walk per pair row of the range (the same file, section 3)
BUILD_CELLS = 22 ** 4 * (4 + 22) * LQ  # a thread per 4-class prefix: its four rows once, the 22 fifth rows each
THIRD_COST = 22 ** 4 * 4 * LQ / TABLE_RATE + WALK_ROW * HEADLINE_ROWS   # what leaving the third level out gives back


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nseq", type=int, default=1000000)
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

    def rows_kept(bound):
        kept = bound >= T
        kept[:head] = True
        return float(blocks[kept].sum()) / float(blocks.sum())

    def say(name, frac, **more):
        print(json.dumps(dict({"level": name, "nseq": a.nseq, "threshold": T, "head_pairs": head, "pairs": len(x),
                               "rows_kept_frac": round(frac, 4)}, **more)), flush=True)

    levels = {}
    bound = None
    for name, S in (("first, 32 segments", 32), ("second, 128 segments", 128), ("third, 256 segments", 256)):
        if S == 32:
            _, u = swg.debug_prune_kmer_seg(sub, q, -2, -1, 4, 32, flat, off, table=False)
        else:
            _, u = swg.debug_prune_kmer_refine(sub, q, -2, -1, S, flat, off, table=False)
        u = u.astype(np.int64)
        pair = np.maximum(u[x], u[y])
        bound = pair if bound is None else np.minimum(bound, pair)
        levels[S] = bound
        say(name, rows_kept(bound))

    def fourth(before, S4):
        """min(before, the (5, S4) bound) on the pairs behind the head that `before` leaves at or above T"""
        walk = np.nonzero(before >= T)[0]
        walk = walk[walk >= head]
        seqs, offs = [], [0]
        for p in walk:
            lx = int(lens[x[p]])
            for s in (x[p], y[p]):
                r = np.zeros(lx, dtype=np.int8)
                r[:lens[s]] = flat[off[s]:off[s + 1]]
                seqs.append(r)
                offs.append(offs[-1] + lx)
        u = swg.debug_prune_kmer_refine4(sub, q, -2, -1, S4, np.concatenate(seqs), np.array(offs, dtype=np.uint64)).astype(np.int64)
        out = before.copy()
        out[walk] = np.minimum(before[walk], np.maximum(u[0::2], u[1::2]))
        return out, len(walk)

    for name, before, S4, back in (("fourth, (5, 128) behind the third", levels[256], 128, 0.0),
                                   ("fourth, (5, 256) behind the third", levels[256], 256, 0.0),
                                   ("fourth, (5, 256) behind the second, no third", levels[128], 256, THIRD_COST)):
        b4, walked = fourth(before, S4)
        frac, base = rows_kept(b4), rows_kept(levels[256])
        # at the headline's size: the build at the prefix-shared kernel's cell count, the walk at the third level's rate
        cost = BUILD_CELLS / TABLE_RATE + WALK_ROW * HEADLINE_ROWS - back
        gain = (base - frac) * HEADLINE_ROWS * FILL_ROW
        say(name, frac, pairs_walked=walked, rows_cut=round(base - frac, 4), cost_ms=round(1e3 * cost, 2), gain_ms=round(1e3 * gain, 2),
            pays=bool(cost <= 0.5 * gain), net_ms=round(1e3 * (gain - cost), 2))


if __name__ == "__main__":
    main()
