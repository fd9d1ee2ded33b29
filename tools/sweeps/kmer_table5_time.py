"""The table kernel of k = 5 as a first-level table (profiles/prune_deep_ab.txt, section 3).

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/sweeps/kmer_table5_time.py

Builds the tables of (5, 8) and (5, 1) for the headline's 3000-column query on a 2000-sequence database, as bytes and as
uint16_t, three new queries each: the table kernel's rows of the kernel statistics give the time per table.  SWG_ROOT
names another built tree to load the library from (the parent of an A/B)."""
import os
import sys

sys.path.insert(0, os.environ.get("SWG_ROOT") or os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import swg_loader  # noqa: E402

swg = swg_loader.load()
q = swg.synth_query(0x5EED0004, 3000)
flat, off = swg.synth_db(0x5EED0E03, 2000, median=60, max_len=300)
ctx = swg.Context(0)
ctx.set_scoring(swg.load_scoring("BLOSUM62"), -2, -1)
ctx.set_query(q)
ctx.set_option("autotune", 0)
db = swg.Database(flat, off).upload(ctx)
ctx.set_option("prune", 2)
ctx.set_option("prune_kmer", 5)
ctx.set_option("prune_refine", 1)
ctx.set_option("prune_refine3", 1)
for bits in (0, 16):
    ctx.set_option("prune_table_bits", bits)
    for S in (8, 1):
        ctx.set_option("prune_segments", S)
        for rep in range(3):
            ctx.set_query(q)
            _, hits, _ = ctx.search(db, want_scores=False, k=10)
        print("bits", bits or 8, "S", S, "pruned", ctx.prune_last()["pruned"], ctx.debug_prune_tables()["bits"], flush=True)
db.close()
