"""A view of a resident database beside the only other route to a subset: cut it out on the host, pack and upload it.

Config 2's database (100 000 sequences, PAM250, 367-residue query).  For selections of 1 %, 10 % and 100 %, in ONE process
with the two routes alternating (ROUNDS times each): the time to have the subset searchable (swg_db_view; host cut +
swg_db_pack + swg_db_upload), the first search of it, and the steady-state search (median of REPEATS wall times around a
search that ends in the read-out).  The parent's own steady state is timed in every round as well: its spread is what
the 100 % view's search time is compared against.  Scores of both routes are checked against each other.

    python tools/sweeps/view_vs_repack.py [out.txt]      (GPU box)
"""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import swg_loader  # noqa: E402

ROUNDS, REPEATS, N, LQ, SEED = 5, 15, 100000, 367, 0x5EED0002


def ms(f):
    t0 = time.perf_counter()
    r = f()
    return (time.perf_counter() - t0) * 1e3, r


def steady(ctx, db):
    ts = []
    for _ in range(REPEATS):
        t, _ = ms(lambda: ctx.search(db, want_scores=False, k=100))
        ts.append(t)
    return statistics.median(ts)


def main():
    swg = swg_loader.load()
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()

    sc = swg.load_scoring("PAM250")
    q = swg.synth_query(SEED, LQ)
    flat, off = swg.synth_db(SEED, N)
    off_i = off.astype(np.int64)
    lens = np.diff(off_i)
    ctx = swg.Context(0)
    ctx.set_scoring(sc, -2, -1)
    ctx.set_query(q)
    t_pack, db = ms(lambda: swg.Database(flat, off))
    t_up, _ = ms(lambda: db.upload(ctx))
    t_first, (truth, _, _) = ms(lambda: ctx.search(db, k=100))
    say("config 2: %d sequences, %d residues, query %d; whole database: pack %.1f ms, upload %.1f ms (%d bytes), first search "
        "%.1f ms" % (N, len(flat), LQ, t_pack, t_up, db.packed_bytes, t_first))
    rng = np.random.default_rng(1)
    rows = {}
    parent_steady = []
    for rnd in range(ROUNDS):
        parent_steady.append(steady(ctx, db))
        for pct in (1, 10, 100):
            sel = np.sort(rng.choice(N, size=N * pct // 100, replace=False)) if pct < 100 else np.arange(N)
            r = rows.setdefault(pct, {k: [] for k in ("view_make", "view_first", "view_steady", "cut", "pack", "upload",
                                                      "repack_first", "repack_steady", "view_bytes", "repack_bytes")})
            for route in (("view", "repack") if rnd % 2 == 0 else ("repack", "view")):
                if route == "view":
                    t, v = ms(lambda: db.view(ctx, sel))
                    r["view_make"].append(t)
                    t, (s_v, h_v, _) = ms(lambda: ctx.search(v, k=100))
                    r["view_first"].append(t)
                    r["view_steady"].append(steady(ctx, v))
                    r["view_bytes"].append(v.packed_bytes)
                    assert np.array_equal(s_v[sel], truth[sel])
                    v.close()
                else:
                    def cut():      # gather the selected records: work proportional to the selection
                        so = np.zeros(len(sel) + 1, dtype=np.uint64)
                        so[1:] = np.cumsum(lens[sel])
                        idx = np.arange(int(so[-1]), dtype=np.int64) + np.repeat(off_i[sel] - so[:-1].astype(np.int64), lens[sel])
                        return flat[idx], so
                    t, (sf, so) = ms(cut)
                    r["cut"].append(t)
                    t, d2 = ms(lambda: swg.Database(sf, so))
                    r["pack"].append(t)
                    t, _ = ms(lambda: d2.upload(ctx))
                    r["upload"].append(t)
                    t, (s_r, h_r, _) = ms(lambda: ctx.search(d2, k=100))
                    r["repack_first"].append(t)
                    r["repack_steady"].append(steady(ctx, d2))
                    r["repack_bytes"].append(d2.packed_bytes)
                    assert np.array_equal(s_r, truth[sel])
                    d2.close()
    med = statistics.median
    say("parent steady-state search (median of %d, per round): %s ms  -> median %.3f, spread %.3f .. %.3f" % (
        REPEATS, " ".join("%.3f" % t for t in parent_steady), med(parent_steady), min(parent_steady), max(parent_steady)))
    say("medians over %d alternating rounds, ms (min .. max in brackets)" % ROUNDS)
    for pct, r in rows.items():
        f = lambda k: "%.2f [%.2f .. %.2f]" % (med(r[k]), min(r[k]), max(r[k]))
        say("%3d %%  view:   make %s  first search %s  steady %s  bytes to GPU %d" % (pct, f("view_make"), f("view_first"),
                                                                                   f("view_steady"), r["view_bytes"][0]))
        say("       repack: cut %s  pack %s  upload %s  (pack + upload %.2f, with the cut %.2f)  first search %s  steady %s  bytes to GPU %d" % (
            f("cut"), f("pack"), f("upload"), med(r["pack"]) + med(r["upload"]), med(r["cut"]) + med(r["pack"]) + med(r["upload"]),
            f("repack_first"),
            f("repack_steady"), r["repack_bytes"][0]))
    db.close()
    ctx.close()


if __name__ == "__main__":
    main()
