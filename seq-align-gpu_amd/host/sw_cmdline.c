/*
 * sw_cmdline.c -- the `smith_waterman` tool over libswg (plain C host code).
 *
 * Same command line, same stdout as the reference's tool (flags:
 * reference src/alignment_cmdline.c:205-292, output: src/tools/sw_cmdline.c:38-75
 * and src/alignment_cmdline.c:274,529-530), with the whole timed
 * fill region (src/alignment_cmdline.c:503-509) replaced by one swg_search()
 * on the GPU.  Deliberate differences, all from SURVEY A.7:
 *   - the database need not be length-sorted nor a multiple of 16 records;
 *   - "Entry #n" is always the true 0-based record index (A.7-3);
 *   - the substitution matrix is mandatory and undefined pairs score 0 (A.7-1,2);
 *   - scores above 32767 are exact instead of wrapped (A.4);
 *   - --topk K appends a ranked report, --align the alignments of those K (the traceback the
 *     reference's fork removed, re-run for the reported pairs only: swg_align_hits);
 *     --gpu N selects the device; --gpus N shards the database over devices 0..N-1 (one RCCL
 *     all-reduce merges the top-K lists); --pssm F scores the query by a PSI-BLAST ASCII PSSM
 *     (swg_pssm_load, swg_set_query_pssm) instead of the matrix (the matrix still fills the PSSM's
 *     unnamed columns); --pssmlist F does the same for every record of --allqueries, one PSSM file
 *     named per line (the records after the first go through swg_search_multi_pssm); --seqidlist F searches only
 *     the database entries whose numbers F lists (a view of the resident database: swg_db_view, swg_group_select);
 *     --allqueries --candidates F searches every query record against its own entries, F's `query entry` lines (one
 *     pass for all records: swg_search_lists); --gapless reports the gapless prefilter score (best ungapped diagonal
 *     segment: swg_search_gapless) instead of the alignment score; --prefilter N --topk K closes the pipeline: per query
 *     the gapless top-N become the candidate list of swg_search_lists, whose K best are reported (and aligned);
 *     --bounds with --topk K appends the coordinates and the length of every reported hit's alignment without its
 *     path (swg_align_bounds, with --allqueries swg_align_bounds_multi / _multi_pssm: no traceback is run);
 *     --tabular with --topk K appends one tab-separated line per reported hit in the columns of BLAST's -outfmt 6 up to
 *     the coordinates, then the raw score (swg_align_stats, with --allqueries swg_align_stats_multi / _multi_pssm: the
 *     identities and gap openings come from the same forward pass, no traceback is run);
 *     --maxhsps N with --align, --bounds or --tabular reports up to N non-overlapping alignments of every reported hit, of
 *     score --hspscore S or more, best first, in those reports' own formats (swg_align_hsps, the records after the first
 *     through swg_align_hsps_multi / _multi_pssm, a record per call);
 *     --minscore S reports every entry that scores at least S, best first, in --topk's block (swg_search_above: no score
 *     array, so no Entry lines), with --topk K the best K of them; under --gpus N each device searches its shard and the
 *     lists are merged by swg_hit_key;
 *     --allqueries --minscorelist F --topk K does the same for every record at its own least score, line i of F being
 *     record i's: the count of the entries at or above it, then the best min(K, count) of them (the records after the
 *     first go through swg_search_above_multi / _multi_pssm, with --gapless swg_search_gapless_above_multi / _pssm);
 *     --evalue E derives those least scores itself: the query -- with --allqueries every record, in one
 *     swg_calibrate_multi / _multi_pssm -- is calibrated on the device against random sequences (swg_calibrate), E becomes a
 *     raw score per query over the residues of what is searched (swg_evalue_min_score), and --minscore's / --minscorelist's
 *     searches run at those; --compfromdb draws the random sequences from the searched entries' own composition
 *     (swg_db_composition); --tabular then prints BLAST's twelve columns, evalue and bitscore included;
 *     --iterations N searches N times, PSI-BLAST's way: each iteration but the last calibrates the current query, turns
 *     --inclusion's E-value into a least score, collects up to --maxincluded hits at or above it (swg_search_above), builds
 *     their PSSM on the device (swg_pssm_build) and makes it the query; the last iteration is the report above with that
 *     PSSM as the query, and --out_pssm writes it in the layout --pssm reads; --psiblocks and --purge P set the
 *     construction's options "pssm_blocks" and "pssm_purge" (per-column blocks, near-identical hits dropped); --compstats [F]
 *     scores every entry an iteration would include again under its composition-adjusted scores (swg_comp_adjust) and
 *     keeps it only if the E-value of the adjusted score is within --inclusion; in the reports it ranks --topk's hits again
 *     by adjusted score (both scores printed), keeps --evalue's hits by the adjusted E-value and prints --tabular's evalue,
 *     bitscore and score columns adjusted (comp_rerank below; swg_comp_adjust_multi / _multi_pssm under --allqueries);
 *     --translatedb [CODE] takes a NUCLEOTIDE database: its six frames are translated on the device after the upload
 *     (swg_db_translate), every stage reads the translation, and a hit is printed as the nucleotide record, its frame and,
 *     in --bounds and --tabular, its nucleotide coordinates (swg_translate_hit, swg_translate_coords).
 * There is no CPU backend: without a GPU the tool fails with a message.
 */
#define _POSIX_C_SOURCE 200809L
#include "../../include/swg.h"
#include "../../include/swg_host.h"

#include <limits.h>
#include <math.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <strings.h>
#include <time.h>
#include <unistd.h>
#ifndef CLOCK_BOOTTIME
#define CLOCK_BOOTTIME 7
#endif

static void usage(const char *argv0, const char *err)
{
    if (err) fprintf(stderr, "Error: %s\n", err);
    fprintf(stderr,
            "usage: %s [OPTIONS] --substitution_matrix <file> --files <query> <database>\n"
            "  Smith-Waterman optimal local alignment score of one query against every\n"
            "  record of a database (FASTA/FASTQ/plain, gzip ok), on an AMD MI355X.\n\n"
            "  OPTIONS:\n"
            "    --files <f1> <f2>    query file (first record) and database file\n"
            "    --pssm <file>        score the query by this PSI-BLAST ASCII PSSM (-out_ascii_pssm; its residues must be the query's)\n"
            "    --pssmlist <file>    with --allqueries: line i names the PSSM of query record i (each must spell its record)\n"
            "    --substitution_matrix <file>  scoring matrix (see data/*.txt)\n"
            "    --gapopen <score>    [default: -2]\n"
            "    --gapextend <score>  [default: -1]   gap of length N costs open + N*extend\n"
            "    --match <score> --mismatch <score>   accepted, unused with a matrix\n"
            "    --printseq           print sequences\n"
            "    --printfasta         print record names\n"
            "    --printmatrices --pretty --colour --scoring <x>   accepted, no effect\n"
            "    --topk <K>           append the K best hits (score, index, name)\n"
            "    --align              with --topk: append the alignment of every reported hit\n"
            "                         (query line over database line, '-' = gap; coordinates 0-based, end exclusive)\n"
            "    --bounds             with --topk: append one line per reported hit, `Bounds #i: entry E score S query a..b entry c..d\n"
            "                         length N` (the alignment's coordinates, 0-based, end exclusive, and its number of steps; no\n"
            "                         alignment text); not with --align, --gapless or --gpus\n"
            "    --tabular            with --topk: append `# Fields: query, entry, pident, length, mismatch, gapopen, qstart, qend, sstart,\n"
            "                         send, score` and one tab-separated line per reported hit of positive score (identity in\n"
            "                         percent of the alignment's length, coordinates 1-based and inclusive, the raw score; a\n"
            "                         PSSM's identity is against its consensus); not with --align, --bounds, --gapless or --gpus\n"
            "    --maxhsps <N>        with --align, --bounds or --tabular: up to N (1 to 64) alignments per reported hit instead of its best\n"
            "                         one -- every non-overlapping local alignment of the pair (no aligned residue pair is shared;\n"
            "                         a later alignment may cross an earlier one through a gap), best first, as blocks or lines of the\n"
            "                         same format, a hit's own one after another under the hit's number; --tabular under --evalue gives\n"
            "                         each line its own evalue and bitscore; works with --topk, --minscore, --minscorelist, --evalue,\n"
            "                         --allqueries, --pssm and --pssmlist; not with --gapless, --gpus, --iterations, --candidates or\n"
            "                         --prefilter\n"
            "    --hspscore <S>       with --maxhsps: the least score (1 or more) of an alignment [default: --minscore's S, the record's\n"
            "                         score of --minscorelist, the score --evalue's E becomes for the query, else 1]\n"
            "    --timing             wall time of every phase (reading, packing, upload, search, printing) on stderr\n"
            "    --gpu <N>            HIP device ordinal [default: 0]\n"
            "    --gpus <N>           shard the database over GPUs 0..N-1 (RCCL top-K merge)\n"
            "    --savedb <file>      also write the packed database (sorted, binned, dword-packed)\n"
            "    --packed             the database file is such a packed database: no parsing,\n"
            "                         no sorting; record names and sequences are not in it\n"
            "    --allqueries         every record of the query file against the resident database\n"
            "                         (one block of output per query, headed `Query #n: name`)\n"
            "    --seqidlist <file>   search only the listed database entries: one entry number per line, the\n"
            "                         numbers of the `Entry #n` lines ('#' starts a comment, blank lines are skipped);\n"
            "                         the Entry lines, Total Entries, --topk and --align report the listed entries only\n"
            "    --candidates <file>  with --allqueries: every query record against its own candidates, all records in one\n"
            "                         pass: one `query_record_number entry_number` pair per line, numbered as `Query #n` and\n"
            "                         `Entry #n` ('#' starts a comment, blank lines are skipped); a record without lines has an\n"
            "                         empty list; per query the Entry lines, Total Entries, --topk and --align report its own\n"
            "                         entries only\n"
            "    --gapless            report the gapless score (best ungapped diagonal segment; the gap scores are not used)\n"
            "                         instead of the alignment score; not with --align, --candidates or --gpus\n"
            "    --minscore <S>       report every entry that scores at least S (1 or more), best first, in --topk's block (no Entry\n"
            "                         lines are printed: no score array is made); with --topk K the best K of them; --align, --bounds and\n"
            "                         --tabular then report those hits; with --gpus N every GPU searches its shard and the lists are\n"
            "                         merged; not with --allqueries, --candidates or --prefilter\n"
            "    --minscorelist <file> with --allqueries --topk K: line i is the least score (1 or more) of query record i; every\n"
            "                         record reports how many entries score at least that, then the best K of them as --minscore\n"
            "                         does; works with --pssmlist, --gapless, --seqidlist, --align, --bounds and --tabular; not with\n"
            "                         --minscore, --candidates, --prefilter or --gpus\n"
            "    --evalue <E>         report every entry whose E-value is at most E (above 0): the query -- with --allqueries --topk K every\n"
            "                         record -- is calibrated on the GPU against random sequences, E becomes a least score over the\n"
            "                         residues of the entries searched (--seqidlist: the listed ones; --gpus N: all shards), and the\n"
            "                         report is --minscore's / --minscorelist's at that score; --tabular then prints the columns\n"
            "                         `..., send, evalue, bitscore, score`; works with --topk, --pssm, --pssmlist, --gapless, --align,\n"
            "                         --bounds; not with --minscore, --minscorelist, --candidates or --prefilter\n"
            "    --compfromdb         with --evalue: the random sequences follow the composition of the entries searched instead of\n"
            "                         the built-in amino-acid frequencies\n"
            "    --iterations <N>     search N times (2 or more): every iteration but the last calibrates the current query, includes the\n"
            "                         entries whose E-value is at most --inclusion (the best --maxincluded of them), builds their\n"
            "                         position-specific scoring matrix on the GPU and makes it the query; the last iteration is the\n"
            "                         usual report (--topk, --align, --tabular, --evalue, ...) with that PSSM as the query; an iteration\n"
            "                         that includes nothing new ends the iterations (said on stderr); --compfromdb gives the\n"
            "                         background; one query record, one GPU: not with --allqueries, --gpus N > 1, --candidates,\n"
            "                         --prefilter or --gapless\n"
            "    --inclusion <E>      with --iterations: the largest E-value of an included entry [default: 0.002]\n"
            "    --maxincluded <M>    with --iterations: the most entries included per iteration [default: 500]\n"
            "    --out_pssm <file>    with --iterations: write the last PSSM (readable by --pssm)\n"
            "    --psiblocks          with --iterations: PSI-BLAST's per-column alignment blocks (option pssm_blocks) instead of one block,\n"
            "                         the whole query, for every column\n"
            "    --compstats [F]      composition-based score adjustment of the reported hits (swg_comp_adjust, PSI-BLAST's\n"
            "                         composition-based statistics): each is scored again under scores scaled by the ratio of the\n"
            "                         ungapped lambdas of its own composition and of the background, at scale F (1 to 64) [default: 32].\n"
            "                         --topk K: the K hits are ranked again by adjusted score (ties: the lower entry) and the block prints\n"
            "                         `adjusted score, score, entry, name`; --evalue E: the unadjusted cut finds the candidates, a hit is\n"
            "                         kept only if the E-value of its ADJUSTED score is within E; --tabular: the evalue, bitscore and\n"
            "                         score columns are the adjusted ones; --iterations N: an entry is included only if the E-value of\n"
            "                         its adjusted score is within --inclusion (the entries that leave are named on stderr); works\n"
            "                         with --allqueries, --pssm, --pssmlist and --seqidlist; not with --gapless, --gpus, --candidates,\n"
            "                         --prefilter or --maxhsps, nor where there is nothing to adjust (the plain Entry lines).\n"
            "                         Alignments, bounds and counts stay those of the unadjusted scores\n"
            "    --purge <P>          with --iterations: drop a hit that is P percent (50 to 100; PSI-BLAST: 94) identical to a kept hit, or\n"
            "                         identical to the query, before the PSSM is built (option pssm_purge)\n"
            "    --prefilter <N>      with --topk K: per query (every record with --allqueries) the N best entries by gapless\n"
            "                         score are searched with gaps and the K best of those reported (--align: aligned);\n"
            "                         no Entry lines are printed; not with --gpus, --candidates or --gapless\n"
            "    --maskdb [W,K1,K2]   mask the low-complexity regions of the database on the GPU, after the upload or the --packed\n"
            "                         load: windows of W residues [12] whose entropy is at most K2 bits [2.5] form runs, a run with\n"
            "                         a window of at most K1 bits [2.2] is masked with X (SEG's trigger and extension stages); every\n"
            "                         stage then reads the masked copy, and --savedb writes it; one GPU: not with --gpus N > 1\n"
            "    --softmask           with --prefilter N: only the gapless prefilter reads the masked copy (--maskdb's parameters, or the\n"
            "                         defaults); the gapped search of the candidates and the alignments read the database as it is\n"
            "    --maskquery          mask every query record the same way on the host before it is searched; not with --pssm or\n"
            "                         --pssmlist\n"
            "    --translatedb [CODE] the database file is NUCLEOTIDE (A C G T/U; anything else is no base): its six reading frames are\n"
            "                         translated on the GPU, after the upload or the --packed load, under NCBI genetic code CODE (1, 2, 3,\n"
            "                         4, 5, 6 or 11) [1], and every stage reads the translation (tblastn's question).  A codon with a\n"
            "                         non-base is X; a stop is `*` in place.  Hits name the nucleotide record and its frame (+1 +2 +3 -1\n"
            "                         -2 -3): the --topk block prints `score, entry, frame, name`, --bounds and --tabular print subject\n"
            "                         coordinates in nucleotides, 1-based and inclusive, start above end on a minus frame, and\n"
            "                         --tabular gains a last column sframe; --align prints the frame's protein alignment.  E-values count\n"
            "                         over the nucleotide residues / 3 (tblastn's convention: the six frames / 6).  Give --topk K,\n"
            "                         --minscore S or --evalue E: no Entry lines are printed.  Works with --allqueries, --pssm,\n"
            "                         --pssmlist, --maskdb (which masks the translation) and --compfromdb (the translation's\n"
            "                         composition); not with --gpus N > 1, --savedb, --seqidlist, --candidates, --prefilter, --softmask,\n"
            "                         --iterations, --compstats or --maxhsps\n",
            argv0);
    exit(EXIT_FAILURE);
}

static double now_ms(void)
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}

/* Milliseconds this process had been alive when called (its start time: /proc/self/stat field 22, in clock ticks
 * since boot): what the dynamic loader and the libraries' static initialisers took before main(). */
static double ms_since_process_start(void)
{
    FILE *f = fopen("/proc/self/stat", "r");
    if (!f) return -1.0;
    char buf[1024];
    const size_t n = fread(buf, 1, sizeof buf - 1, f);
    fclose(f);
    buf[n] = 0;
    const char *p = strrchr(buf, ')'); /* the command name may hold spaces */
    if (!p) return -1.0;
    unsigned long long start = 0;
    int field = 2;
    for (p++; *p && field < 22; p++)
        if (*p == ' ') field++;
    if (sscanf(p, "%llu", &start) != 1) return -1.0;
    struct timespec ts;
    clock_gettime(CLOCK_BOOTTIME, &ts);
    return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6 - (double)start * 1e3 / (double)sysconf(_SC_CLK_TCK);
}

/* The HIP runtime's start-up (most of a one-shot run: ~200 ms) needs nothing of the input: it runs on a thread of
 * its own while the main thread reads, converts, sorts and packs the files. */
typedef struct {
    swg_config cfg;
    swg_ctx *ctx;
    int rc;
    char err[512];
    double ms;
} ctx_job;
static void *ctx_job_run(void *arg)
{
    ctx_job *j = (ctx_job *)arg;
    const double t0 = now_ms();
    j->rc = swg_create(&j->cfg, &j->ctx);
    if (j->rc != SWG_OK) snprintf(j->err, sizeof j->err, "%s", swg_global_error()); /* (thread-local text) */
    j->ms = now_ms() - t0;
    return NULL;
}

static pthread_t g_job_thread;
static int g_job_started = 0;
/* every way out of main() after the thread has started waits for it: the process must not run its exit handlers
 * while another thread is inside the HIP runtime's start-up */
static int leave(int code)
{
    if (g_job_started) {
        pthread_join(g_job_thread, NULL);
        g_job_started = 0;
    }
    return code;
}

/* --timing: wall time of the phases the reference leaves out of its `Total Time`, on stderr */
static int timing = 0;
static double phase_t0;
static void phase(const char *what)
{
    const double t = now_ms();
    if (timing) fprintf(stderr, "[timing] %-28s %9.2f ms\n", what, t - phase_t0);
    phase_t0 = t;
}

static int parse_int(const char *s, long lo, long hi, long *out)
{
    char *end = NULL;
    const long v = strtol(s, &end, 10);
    if (end == s || *end != '\0' || v < lo || v > hi) return 0;
    *out = v;
    return 1;
}

/* --maxhsps: the alignments of one record's hits (swg_align_hsps*): hit i's r-th of n[i] at al / ct [i*per + r], its path
 * at ops + (i*per + r)*stride.  One record per call: qoff == NULL takes the context's query, else src is the record's
 * index bytes or (pssm) PSSM rows at qoff[0] .. qoff[1]. */
struct hsps {
    swg_alignment *al;
    swg_align_counts *ct;
    uint32_t *n;
    char *ops;
    size_t per, stride;
};

static int hsps_run(struct hsps *h, swg_ctx *ctx, const swg_db *sdb, const int8_t *src, int pssm, const uint64_t *qoff, const swg_hit *hits,
                    size_t n_hits, long maxhsps, long least)
{
    free(h->al), free(h->ct), free(h->n), free(h->ops);
    h->per = (size_t)maxhsps;
    h->stride = qoff ? swg_align_ops_bound_multi(sdb, qoff, 1) : swg_align_ops_bound(ctx, sdb);
    h->al = (swg_alignment *)calloc(n_hits * h->per, sizeof *h->al);
    h->ct = (swg_align_counts *)calloc(n_hits * h->per, sizeof *h->ct);
    h->n = (uint32_t *)calloc(n_hits, sizeof *h->n);
    h->ops = (char *)malloc(n_hits * h->per * h->stride);
    if (!h->al || !h->ct || !h->n || !h->ops) {
        fprintf(stderr, "Error: out of memory\n");
        return SWG_ERR_NOMEM;
    }
    const int rc = !qoff ? swg_align_hsps(ctx, sdb, hits, n_hits, (uint32_t)maxhsps, (int32_t)least, h->al, h->n, h->ct, h->ops, h->stride)
                   : pssm ? swg_align_hsps_multi_pssm(ctx, sdb, src, qoff, 1, hits, n_hits, &n_hits, (uint32_t)maxhsps, (int32_t)least, h->al,
                                                      h->n, h->ct, h->ops, h->stride)
                          : swg_align_hsps_multi(ctx, sdb, src, qoff, 1, hits, n_hits, &n_hits, (uint32_t)maxhsps, (int32_t)least, h->al, h->n,
                                                 h->ct, h->ops, h->stride);
    if (rc != SWG_OK) fprintf(stderr, "Error: %s\n", swg_last_error(ctx));
    return rc;
}

/* --compstats: the hits of nq records -- row r's at hits[r*k .. r*k + nh[r]) -- scored again under their composition-adjusted
 * scores (swg_comp_adjust for the context's query when src is NULL, else the batch call), adj[r*k + j] beside hit j of row r.
 * ev != NULL: a hit stays only if the E-value of its adjusted score, by its record's fit, is within E.  Each row is then
 * ranked by adjusted score, ties by the lower entry.  The hits keep their unadjusted scores. */
static int comp_rerank(swg_ctx *ctx, const swg_db *sdb, long F, const int8_t *src, int pssm, const uint64_t *qoff, size_t nq, swg_hit *hits,
                       size_t k, size_t *nh, const double *freq, int32_t *adj, const swg_evalue_params *ev, uint64_t residues, double E)
{
    size_t total = 0;
    for (size_t r = 0; r < nq; r++) total += nh[r];
    if (total == 0) return SWG_OK;
    swg_comp_result *cr = (swg_comp_result *)calloc(nq * k, sizeof *cr);
    if (!cr) return SWG_ERR_NOMEM;
    int rc = swg_set_option(ctx, "comp_scale", F);
    if (rc == SWG_OK)
        rc = !src ? swg_comp_adjust(ctx, sdb, hits, nh[0], freq, cr, NULL)
                  : pssm ? swg_comp_adjust_multi_pssm(ctx, sdb, src, qoff, nq, hits, k, nh, freq, cr, NULL)
                         : swg_comp_adjust_multi(ctx, sdb, src, qoff, nq, hits, k, nh, freq, cr, NULL);
    for (size_t r = 0; rc == SWG_OK && r < nq; r++) {
        swg_hit *h = hits + r * k;
        int32_t *a = adj + r * k;
        size_t kept = 0;
        for (size_t j = 0; j < nh[r]; j++) {
            const int32_t s = cr[r * k + j].adj_score;
            if (ev && swg_evalue(&ev[r], residues, s) > E) continue;
            const swg_hit moved = h[j]; /* (read before the shift below, which may write slot j) */
            size_t at = kept++;         /* insertion: the rows are short and nearly in order already */
            for (; at > 0 && (a[at - 1] < s || (a[at - 1] == s && h[at - 1].index > moved.index)); at--) h[at] = h[at - 1], a[at] = a[at - 1];
            h[at] = moved, a[at] = s;
        }
        nh[r] = kept;
    }
    free(cr);
    return rc;
}

static void die_illegal(char c)
{
    /* reference src/alignment_scoring.c:78-79 */
    printf("Error: %c is not a legal character for the substitution matrix!\n", c);
    (void)leave(0);
    exit(1);
}

/* --evalue: the context's query (n_rec == 1 without qx / pssms), or every record of the query file in one batch call, is
 * calibrated on ctx -- against the composition `counts` where --compfromdb gave one -- and E becomes each record's least
 * score over `residues` (least[i]).  A record without a fit is refused by name.  Returns 0 after an error message. */
static int evalue_scores(swg_ctx *ctx, const swg_seqs *q, size_t n_rec, const int8_t *qx, const int8_t *pssms, int gapless,
                         const uint64_t *counts, uint64_t residues, double E, swg_evalue_params *ev, int32_t *least)
{
    double freq[32];
    for (int r = 0; r < 32; r++) freq[r] = counts ? (double)counts[r] : 0.0;
    const double *fq = counts ? freq : NULL;
    const int rc = pssms ? swg_calibrate_multi_pssm(ctx, pssms, q->seq_off, n_rec, fq, gapless, ev)
                   : qx  ? swg_calibrate_multi(ctx, qx, q->seq_off, n_rec, fq, gapless, ev)
                         : swg_calibrate(ctx, fq, gapless, ev);
    if (rc != SWG_OK) {
        fprintf(stderr, "Error: %s\n", swg_last_error(ctx));
        return 0;
    }
    for (size_t i = 0; i < n_rec; i++) {
        if (ev[i].status != 0) {
            fprintf(stderr, "Error: query #%lu (%s) has no E-value statistics: %s\n", (unsigned long)i, q->names + q->name_off[i],
                    ev[i].status == 1 ? "its scores against the random sequences are all the same"
                                      : "the fit of its scores against the random sequences did not converge");
            return 0;
        }
        least[i] = swg_evalue_min_score(&ev[i], residues, E);
        if (least[i] < 1) {
            fprintf(stderr, "Error: query #%lu (%s): no score has an E-value of %g or less\n", (unsigned long)i, q->names + q->name_off[i], E);
            return 0;
        }
    }
    return 1;
}

/* --maskquery: the masked positions of a query record take the replacement residue */
/* --translatedb: a hit's entry is frame (index % 6) of the nucleotide record (index / 6); BLAST's names of the frames */
static const char *const frame_names[6] = {"+1", "+2", "+3", "-1", "-2", "-3"};

/* the nucleotides an alignment in a frame covers, 1-based and inclusive, the start above the end on a minus frame */
static void nt_span(int frame, uint32_t nt_len, const swg_alignment *a, uint32_t *start, uint32_t *end)
{
    uint32_t b = 0, e = 0;
    *start = *end = 0;
    if (swg_translate_coords(frame, nt_len, a->d_begin, a->d_end, &b, &e) != SWG_OK) return; /* (a score of 0: no alignment) */
    *start = frame < 3 ? b + 1 : e;
    *end = frame < 3 ? e : b + 1;
}

/* the length of nucleotide record `rec`: from the FASTA's offsets, or for a --packed database from its host image */
static uint32_t nt_length(const swg_db *ntdb, const swg_seqs *db, int packed, uint32_t rec)
{
    size_t len = 0;
    if (!packed) return (uint32_t)(db->seq_off[rec + 1] - db->seq_off[rec]);
    (void)swg_db_sequence(ntdb, rec, NULL, 0, &len); /* (no room given: the length alone comes back) */
    return (uint32_t)len;
}

/* the letters of one frame of nt[len] (table indices), NUL-terminated; NULL: out of memory */
static char *frame_letters(const int8_t *nt, size_t len, int frame, const swg_translate_params *tp)
{
    int8_t *buf = (int8_t *)malloc(6 * (len / 3) + 1), *out[6];
    size_t n[6];
    char *s = (char *)malloc(len / 3 + 1);
    for (int g = 0; g < 6; g++) out[g] = buf ? buf + (size_t)g * (len / 3) : NULL;
    if (!buf || !s || swg_translate_seq(nt, len, tp, out, n) != SWG_OK) {
        free(buf);
        free(s);
        return NULL;
    }
    for (size_t k = 0; k < n[frame]; k++) s[k] = (char)swg_index_letter(out[frame][k]);
    s[n[frame]] = 0;
    free(buf);
    return s;
}

static int mask_query(int8_t *idx, size_t n, const swg_mask_params *mp)
{
    uint8_t *m = (uint8_t *)malloc(n ? n : 1);
    size_t n_masked = 0;
    if (!m) return SWG_ERR_NOMEM;
    const int rc = swg_seg_mask(idx, n, mp, m, &n_masked);
    for (size_t i = 0; rc == SWG_OK && n_masked && i < n; i++)
        if (m[i]) idx[i] = (int8_t)mp->replace;
    free(m);
    return rc;
}

int main(int argc, char **argv)
{
    swg_scoring sc;
    swg_scoring_init(&sc);
    const char *qpath = NULL, *dbpath = NULL, *savedb = NULL, *pssm_path = NULL, *pssmlist_path = NULL, *idlist_path = NULL, *cand_path = NULL;
    const char *mslist_path = NULL;
    int print_seq = 0, print_fasta = 0, have_matrix = 0, packed = 0, allq = 0;
    long topk = 0, gpu = 0, gpus = 0, prefilter = 0, minscore = 0, v;
    long maxhsps = 0, hspscore = 0;
    int align = 0, gapless = 0, bounds = 0, tabular = 0, have_evalue = 0, compfromdb = 0;
    double evalue = 0.0, inclusion = 0.002;
    long iterations = 0, maxincluded = 500;
    long compstats = 0; /* --compstats [F]: the scale of the composition-based adjustment, 0 = off */
    int have_inclusion = 0, have_maxincluded = 0, psiblocks = 0;
    long purge = 0;
    const char *out_pssm = NULL;
    int maskdb = 0, softmask = 0, maskquery = 0;
    int translatedb = 0; /* --translatedb [CODE]: the database is nucleotide, its six frames are what is searched */
    swg_translate_params tp;
    (void)swg_codon_table(1, &tp);
    swg_mask_params mp;
    swg_mask_params_default(&mp);
    if (argc == 1) usage(argv[0], NULL);
    for (int i = 1; i < argc; i++)
        if (!strcasecmp(argv[i], "--help") || !strcasecmp(argv[i], "-help") || !strcasecmp(argv[i], "-h"))
            usage(argv[0], NULL);
    for (int i = 1; i < argc; i++) {
        const char *a = argv[i];
        if (!strcasecmp(a, "--printseq")) print_seq = 1;
        else if (!strcasecmp(a, "--printfasta")) print_fasta = 1;
        else if (!strcasecmp(a, "--printmatrices") || !strcasecmp(a, "--pretty") || !strcasecmp(a, "--colour")) {
        } else if (!strcasecmp(a, "--stdin")) {
            /* reference src/alignment_cmdline.c:219-222: cmdline_set_files(cmd, "", NULL) -- a query path
             * and NO database, which its cmdline_new then refuses with "No input specified" (:303-305) */
            qpath = "";
            dbpath = NULL;
        } else if (!strcasecmp(a, "--packed")) { /* this tool's flag-only options: valid in last position too */
            packed = 1;
        } else if (!strcasecmp(a, "--align")) {
            align = 1;
        } else if (!strcasecmp(a, "--gapless")) {
            gapless = 1;
        } else if (!strcasecmp(a, "--bounds")) {
            bounds = 1;
        } else if (!strcasecmp(a, "--tabular")) {
            tabular = 1;
        } else if (!strcasecmp(a, "--compfromdb")) {
            compfromdb = 1;
        } else if (!strcasecmp(a, "--psiblocks")) {
            psiblocks = 1;
        } else if (!strcasecmp(a, "--compstats")) { /* the scale is optional: a number 1 to 64 behind the flag is taken as it */
            long f;
            compstats = 32;
            if (i + 1 < argc && parse_int(argv[i + 1], LONG_MIN, LONG_MAX, &f)) { /* (any whole number behind the flag is meant as F) */
                if (f < 1 || f > 64) usage(argv[0], "Invalid --compstats argument: the scale F of the adjusted scores, 1 to 64");
                compstats = f, i++;
            }
        } else if (!strcasecmp(a, "--timing")) {
            timing = 1;
        } else if (!strcasecmp(a, "--allqueries")) {
            allq = 1;
        } else if (!strcasecmp(a, "--softmask")) {
            softmask = 1;
        } else if (!strcasecmp(a, "--maskquery")) {
            maskquery = 1;
        } else if (!strcasecmp(a, "--translatedb")) { /* the code is optional: a whole number behind the flag is taken as it */
            long code;
            translatedb = 1;
            if (i + 1 < argc && parse_int(argv[i + 1], LONG_MIN, LONG_MAX, &code)) {
                if (code < INT_MIN || code > INT_MAX || swg_codon_table((int)code, &tp) != SWG_OK)
                    usage(argv[0], "Invalid --translatedb argument: an NCBI genetic code, one of 1, 2, 3, 4, 5, 6 and 11");
                i++;
            }
        } else if (!strcasecmp(a, "--maskdb")) {
            maskdb = 1;
            /* the parameters are optional: W,K1,K2 in one argument that starts with a digit and holds a comma */
            if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9' && strchr(argv[i + 1], ',')) {
                long w = 0;
                double k1 = 0.0, k2 = 0.0;
                char tail = 0;
                int32_t T[65];
                int64_t t1, t2;
                const int got = sscanf(argv[i + 1], "%ld,%lf,%lf%c", &w, &k1, &k2, &tail);
                if (got == 3 && w >= INT_MIN && w <= INT_MAX) mp.window = (int32_t)w, mp.trigger = k1, mp.extend = k2;
                if (got != 3 || swg_mask_tables(&mp, T, &t1, &t2) != SWG_OK)
                    usage(argv[0], "Invalid --maskdb argument: W,K1,K2 with a window W of 4..64 residues and 0 <= K1 <= K2 bits");
                i++;
            }
        } else if (i == argc - 1) {
            char msg[256];
            snprintf(msg, sizeof msg, "Unknown argument without parameter: %s", a);
            usage(argv[0], msg);
        } else if (!strcasecmp(a, "--scoring")) {
            i++;
        } else if (!strcasecmp(a, "--substitution_matrix")) {
            char err[512];
            if (swg_scoring_load_matrix(&sc, argv[i + 1], err, sizeof err) != SWG_OK) {
                fprintf(stderr, "Error: %s\n", err);
                return EXIT_FAILURE;
            }
            have_matrix = 1;
            i++;
        } else if (!strcasecmp(a, "--match") || !strcasecmp(a, "--mismatch")) {
            if (!parse_int(argv[i + 1], INT_MIN, INT_MAX, &v)) usage(argv[0], "Invalid --match/--mismatch argument, must be an int");
            if (!strcasecmp(a, "--match")) sc.match = (int)v; else sc.mismatch = (int)v;
            i++;
        } else if (!strcasecmp(a, "--gapopen") || !strcasecmp(a, "--gapextend")) {
            /* the reference's score_t is int16 (src/alignment_cmdline.c:255-267) */
            if (!parse_int(argv[i + 1], SHRT_MIN, SHRT_MAX, &v)) usage(argv[0], "Invalid --gapopen/--gapextend argument, must be an int");
            if (!strcasecmp(a, "--gapopen")) sc.gap_open = (int)v; else sc.gap_extend = (int)v;
            i++;
        } else if (!strcasecmp(a, "--topk")) {
            if (!parse_int(argv[i + 1], 0, 1 << 20, &topk)) usage(argv[0], "Invalid --topk argument");
            i++;
        } else if (!strcasecmp(a, "--minscore")) {
            if (!parse_int(argv[i + 1], 1, INT_MAX, &minscore)) usage(argv[0], "Invalid --minscore argument: the least score to report, 1 or more");
            i++;
        } else if (!strcasecmp(a, "--maxhsps")) {
            if (!parse_int(argv[i + 1], 1, SWG_MAX_HSPS, &maxhsps)) usage(argv[0], "Invalid --maxhsps argument: the most alignments per reported hit, 1 to 64");
            i++;
        } else if (!strcasecmp(a, "--hspscore")) {
            if (!parse_int(argv[i + 1], 1, INT_MAX, &hspscore)) usage(argv[0], "Invalid --hspscore argument: the least score of an alignment, 1 or more");
            i++;
        } else if (!strcasecmp(a, "--minscorelist")) {
            mslist_path = argv[++i];
        } else if (!strcasecmp(a, "--evalue")) {
            char *end = NULL;
            evalue = strtod(argv[i + 1], &end);
            if (end == argv[i + 1] || *end != '\0' || !(evalue > 0.0) || isinf(evalue))
                usage(argv[0], "Invalid --evalue argument: the largest E-value to report, a number above 0");
            have_evalue = 1;
            i++;
        } else if (!strcasecmp(a, "--iterations")) {
            if (!parse_int(argv[i + 1], 2, 1000, &iterations)) usage(argv[0], "Invalid --iterations argument: the number of searches, 2 or more");
            i++;
        } else if (!strcasecmp(a, "--inclusion")) {
            char *end = NULL;
            inclusion = strtod(argv[i + 1], &end);
            if (end == argv[i + 1] || *end != '\0' || !(inclusion > 0.0) || isinf(inclusion))
                usage(argv[0], "Invalid --inclusion argument: the largest E-value of an included entry, a number above 0");
            have_inclusion = 1;
            i++;
        } else if (!strcasecmp(a, "--maxincluded")) {
            if (!parse_int(argv[i + 1], 1, 1 << 20, &maxincluded)) usage(argv[0], "Invalid --maxincluded argument: the most entries included per iteration, 1 or more");
            have_maxincluded = 1;
            i++;
        } else if (!strcasecmp(a, "--out_pssm")) {
            out_pssm = argv[++i];
        } else if (!strcasecmp(a, "--purge")) {
            if (!parse_int(argv[i + 1], 50, 100, &purge)) usage(argv[0], "Invalid --purge argument: the percent identity at which a hit is dropped, 50 to 100");
            i++;
        } else if (!strcasecmp(a, "--prefilter")) {
            if (!parse_int(argv[i + 1], 1, 1 << 20, &prefilter)) usage(argv[0], "Invalid --prefilter argument: the number of candidates per query, 1 or more");
            i++;
        } else if (!strcasecmp(a, "--pssm")) {
            pssm_path = argv[++i];
        } else if (!strcasecmp(a, "--pssmlist")) {
            pssmlist_path = argv[++i];
        } else if (!strcasecmp(a, "--seqidlist")) {
            idlist_path = argv[++i];
        } else if (!strcasecmp(a, "--candidates")) {
            cand_path = argv[++i];
        } else if (!strcasecmp(a, "--savedb")) {
            if (i >= argc - 1) usage(argv[0], "--savedb takes a file name");
            savedb = argv[++i];
        } else if (!strcasecmp(a, "--file")) {
            /* reference src/alignment_cmdline.c:268-270: cmdline_set_files(cmd, argv[argi + 1], NULL) */
            qpath = argv[i + 1];
            dbpath = NULL;
            i++;
        } else if (!strcasecmp(a, "--gpus")) {
            if (!parse_int(argv[i + 1], 1, 64, &gpus)) usage(argv[0], "Invalid --gpus argument");
            i++;
        } else if (!strcasecmp(a, "--gpu")) {
            if (!parse_int(argv[i + 1], 0, 1023, &gpu)) usage(argv[0], "Invalid --gpu argument");
            i++;
        } else if (!strcasecmp(a, "--files")) {
            if (i >= argc - 2) usage(argv[0], "--files option takes 2 arguments");
            /* reference src/alignment_cmdline.c:274 */
            printf("Query File=%s and Database File=%s\n", argv[i + 1], argv[i + 2]);
            qpath = argv[i + 1];
            dbpath = argv[i + 2];
            i += 2;
        } else {
            char msg[256];
            snprintf(msg, sizeof msg, "Unknown argument '%s'", a);
            usage(argv[0], msg);
        }
    }
    if (!qpath || !dbpath) usage(argv[0], "No input specified"); /* reference src/alignment_cmdline.c:303-305 */
    if (!have_matrix) usage(argv[0], "--substitution_matrix is required (the fill scores from the matrix only)");
    if (translatedb) { /* what a translated search does not combine with: each by name, before a device is opened */
        if (gpus > 1) usage(argv[0], "--translatedb works with one GPU (--gpu): it does not combine with --gpus N > 1");
        if (savedb) usage(argv[0], "--translatedb does not combine with --savedb (the file would hold the translation, not the database given)");
        if (idlist_path) usage(argv[0], "--translatedb does not combine with --seqidlist (the entries searched are frames, not the records listed)");
        if (cand_path) usage(argv[0], "--translatedb does not combine with --candidates (the entries searched are frames, not the records listed)");
        if (prefilter) usage(argv[0], "--translatedb does not combine with --prefilter");
        if (softmask) usage(argv[0], "--translatedb does not combine with --softmask (--maskdb masks the translation)");
        if (iterations) usage(argv[0], "--translatedb does not combine with --iterations");
        if (compstats) usage(argv[0], "--translatedb does not combine with --compstats");
        if (maxhsps) usage(argv[0], "--translatedb does not combine with --maxhsps");
        if (topk == 0 && !minscore && !mslist_path && !have_evalue)
            usage(argv[0], "--translatedb reports hits, not the Entry lines of every frame: give --topk K, --minscore S or --evalue E");
        if (gpus == 1) gpus = 0; /* (one GPU either way: the translation is made on a context) */
    }
    if (maxhsps && !align && !bounds && !tabular)
        usage(argv[0], "--maxhsps N reports up to N alignments per hit of --align, --bounds or --tabular: give one of them");
    if (maxhsps && (gapless || gpus > 0 || iterations || cand_path || prefilter))
        usage(argv[0], "--maxhsps does not combine with --gapless, --gpus, --iterations, --candidates or --prefilter");
    if (hspscore && !maxhsps) usage(argv[0], "--hspscore is the least score of --maxhsps' alignments: give --maxhsps N");
    if (packed && (print_seq || print_fasta)) usage(argv[0], "--printseq/--printfasta need the FASTA database, not --packed");
    if (pssmlist_path && !allq) usage(argv[0], "--pssmlist names the PSSMs of --allqueries' records: give --allqueries");
    if (pssmlist_path && pssm_path) usage(argv[0], "--pssmlist and --pssm do not combine (the list names the first record's PSSM too)");
    if (pssmlist_path && gpus > 0) usage(argv[0], "--pssmlist works with one GPU (--gpu)");
    if ((packed || savedb || allq) && gpus > 0) usage(argv[0], "--packed/--savedb/--allqueries work with one GPU (--gpu)");
    if (have_evalue && (minscore || mslist_path)) usage(argv[0], "--evalue derives the least score itself: it does not combine with --minscore or --minscorelist");
    if (have_evalue && (cand_path || prefilter)) usage(argv[0], "--evalue does not combine with --candidates or --prefilter");
    if (have_evalue && allq && topk == 0) usage(argv[0], "--allqueries --evalue reports up to --topk K hits per record: give --topk K");
    if (compfromdb && !have_evalue && !iterations) usage(argv[0], "--compfromdb chooses the background of --evalue's calibration: give --evalue E");
    if (!iterations && (have_inclusion || have_maxincluded || out_pssm))
        usage(argv[0], "--inclusion, --maxincluded and --out_pssm belong to the iterated search: give --iterations N");
    if (compstats && !iterations && topk == 0 && !minscore && !have_evalue && !mslist_path)
        usage(argv[0], "--compstats adjusts the scores of reported hits: give --topk K, --evalue E, --minscore S or --iterations N (the plain "
                       "Entry lines have nothing to adjust)");
    if (compstats && (gapless || gpus > 0 || cand_path || prefilter || maxhsps))
        usage(argv[0], "--compstats does not combine with --gapless, --gpus, --candidates, --prefilter or --maxhsps");
    if (!iterations && psiblocks) usage(argv[0], "--psiblocks chooses the model of the iterated search's PSSM: give --iterations N");
    if (!iterations && purge) usage(argv[0], "--purge drops near-identical hits from the iterated search's PSSM: give --iterations N");
    if (iterations && allq) usage(argv[0], "--iterations iterates one query record: it does not combine with --allqueries");
    if (iterations && gpus > 1) usage(argv[0], "--iterations works with one GPU (--gpu): it does not combine with --gpus N > 1");
    if (iterations && cand_path) usage(argv[0], "--iterations makes its own lists of included entries: it does not combine with --candidates");
    if (iterations && prefilter) usage(argv[0], "--iterations makes its own lists of included entries: it does not combine with --prefilter");
    if (iterations && gapless) usage(argv[0], "--iterations builds its PSSM from gapped alignments: it does not combine with --gapless");
    if (softmask && !prefilter) usage(argv[0], "--softmask masks what the gapless prefilter reads: give --prefilter N");
    if (softmask) maskdb = 1;
    if (maskdb && gpus > 1) usage(argv[0], "--maskdb works with one GPU (--gpu): it does not combine with --gpus N > 1");
    if (maskquery && (pssm_path || pssmlist_path)) usage(argv[0], "--maskquery masks residues: it does not combine with --pssm or --pssmlist");
    if (maskdb && gpus == 1) gpus = 0; /* (one GPU either way: the copy is made on a context) */
    if (iterations && gpus == 1) gpus = 0; /* (one GPU either way: the iterations run on a context, not on a group of one) */
    /* --evalue: the searches of --minscore (one query) or of --minscorelist (every record) at scores the calibration gives;
     * until it has run, 1 stands for them */
    const int ev_batch = have_evalue && allq;
    if (have_evalue && !allq) minscore = 1;
    if (minscore && mslist_path) usage(argv[0], "--minscorelist does not combine with --minscore, --candidates, --prefilter or --gpus");
    if (minscore && (allq || cand_path || prefilter)) usage(argv[0], "--minscore reports one query's hits: it does not combine with --allqueries, --candidates or --prefilter");
    if (mslist_path && !allq) usage(argv[0], "--minscorelist gives the least score of each of --allqueries' records: give --allqueries");
    if (mslist_path && topk == 0) usage(argv[0], "--minscorelist reports up to --topk K hits per record: give --topk K");
    if (mslist_path && (cand_path || prefilter || gpus > 0))
        usage(argv[0], "--minscorelist does not combine with --minscore, --candidates, --prefilter or --gpus");
    if (align && topk == 0 && !minscore) usage(argv[0], "--align reports the alignments of the --topk hits: give --topk K");
    if (bounds && topk == 0 && !minscore) usage(argv[0], "--bounds reports the alignment coordinates of the --topk hits: give --topk K");
    if (bounds && align) usage(argv[0], "--bounds reports coordinates without the alignments: it does not combine with --align (whose headers carry them)");
    if (bounds && gapless) usage(argv[0], "--bounds reports coordinates of gapped alignments: it does not combine with --gapless");
    if (bounds && gpus > 0) usage(argv[0], "--bounds works with one GPU (--gpu)");
    if (tabular && topk == 0 && !minscore) usage(argv[0], "--tabular reports one tabular line for each of the --topk hits: give --topk K");
    if (tabular && align) usage(argv[0], "--tabular reports counts without the alignments: it does not combine with --align");
    if (tabular && bounds) usage(argv[0], "--tabular carries the coordinates itself: it does not combine with --bounds");
    if (tabular && gapless) usage(argv[0], "--tabular reports gapped alignments: it does not combine with --gapless");
    if (tabular && gpus > 0) usage(argv[0], "--tabular works with one GPU (--gpu)");
    if (pssm_path && allq) usage(argv[0], "--pssm scores one query: it does not combine with --allqueries");
    if (cand_path && !allq) usage(argv[0], "--candidates lists the entries of --allqueries' records: give --allqueries");
    if (cand_path && gpus > 0) usage(argv[0], "--candidates works with one GPU (--gpu)");
    if (cand_path && idlist_path) usage(argv[0], "--candidates and --seqidlist do not combine (the candidates are the entries to search)");
    if (cand_path && pssm_path) usage(argv[0], "--candidates and --pssm do not combine (--pssmlist names a PSSM per record)");
    if (gapless && align) usage(argv[0], "--gapless reports scores of ungapped segments: it does not combine with --align");
    if (gapless && ((gpus > 0 && !minscore) || cand_path)) usage(argv[0], "--gapless works with one GPU (--gpu) and without --candidates");
    if (prefilter && topk == 0) usage(argv[0], "--prefilter N reports the --topk hits among the N gapless candidates: give --topk K");
    if (prefilter && gpus > 0) usage(argv[0], "--prefilter works with one GPU (--gpu)");
    if (prefilter && (cand_path || gapless)) usage(argv[0], "--prefilter makes the candidate lists itself: it does not combine with --candidates or --gapless");

    char err[512];
    swg_seqs q, db;
    if (timing) fprintf(stderr, "[timing] %-28s %9.2f ms\n", "process start to main()", ms_since_process_start());
    /* one GPU: the context is created beside the reading and packing (several GPUs: swg_group_create, below) */
    ctx_job job;
    memset(&job, 0, sizeof job);
    if (gpus == 0) {
        job.cfg.device = (int)gpu;
        g_job_started = pthread_create(&g_job_thread, NULL, ctx_job_run, &job) == 0;
    }
    phase_t0 = now_ms();
    if (swg_seqs_read(qpath, allq ? 0 : 1, &q, err, sizeof err) != SWG_OK) {
        fprintf(stderr, "Error: couldn't open query file %s\n", qpath);
        return leave(EXIT_SUCCESS); /* the reference returns from the driver and exits 0 */
    }
    if (q.n == 0 || q.seq_off[1] == 0) {
        fprintf(stderr, "Error: Query file %s is empty or invalid\n", qpath);
        return leave(EXIT_SUCCESS);
    }
    swg_db *pdb = NULL;
    memset(&db, 0, sizeof db);
    if (packed) {
        if (swg_db_load(dbpath, &pdb) != SWG_OK) {
            fprintf(stderr, "Error: %s\n", swg_global_error());
            return leave(EXIT_SUCCESS);
        }
        db.n = swg_db_total_count(pdb);
    } else if (swg_seqs_read(dbpath, 0, &db, err, sizeof err) != SWG_OK) {
        fprintf(stderr, "Error: couldn't open database file %s\n", dbpath);
        return leave(EXIT_SUCCESS);
    }
    phase(packed ? "read query, load packed db" : "read query and database");
    /* the entries searched, scored and numbered in hits: the records, or with --translatedb their six frames each */
    const size_t n_entries = translatedb ? 6 * db.n : db.n;
    /* --seqidlist: the entries to search, and a mark per entry for the printing */
    uint32_t *ids = NULL;
    size_t n_ids = 0, n_listed = 0;
    unsigned char *listed = NULL;
    if (idlist_path) {
        FILE *lf = fopen(idlist_path, "r");
        if (!lf) {
            fprintf(stderr, "Error: couldn't open the entry list %s\n", idlist_path);
            return leave(EXIT_FAILURE);
        }
        listed = (unsigned char *)calloc(db.n ? db.n : 1, 1);
        size_t cap = 0;
        unsigned long line_no = 0;
        char line[4096];
        while (listed && fgets(line, sizeof line, lf)) {
            line_no++;
            char *b = line, *e = strchr(line, '#');
            if (!e) e = line + strlen(line);
            while (*b == ' ' || *b == '\t') b++;
            while (e > b && (e[-1] == '\n' || e[-1] == '\r' || e[-1] == ' ' || e[-1] == '\t')) e--;
            if (e <= b) continue;
            *e = 0;
            char *end = NULL;
            const unsigned long long num = strtoull(b, &end, 10);
            if (*b < '0' || *b > '9' || *end != 0 || num >= (unsigned long long)db.n) {
                char msg[512];
                snprintf(msg, sizeof msg, "--seqidlist %s line %lu: '%s' is not an entry number of this database (0..%lu)", idlist_path,
                         line_no, b, (unsigned long)db.n - 1);
                (void)leave(0);
                usage(argv[0], msg);
            }
            if (n_ids == cap) {
                cap = cap ? 2 * cap : 1024;
                uint32_t *grown = (uint32_t *)realloc(ids, cap * sizeof *ids);
                if (!grown) return leave(EXIT_FAILURE);
                ids = grown;
            }
            ids[n_ids++] = (uint32_t)num;
            if (!listed[num]) listed[num] = 1, n_listed++;
        }
        fclose(lf);
        if (!listed || (!ids && !(ids = (uint32_t *)malloc(sizeof *ids)))) { /* (an empty list is a list: ids is not NULL) */
            fprintf(stderr, "Error: out of memory\n");
            return leave(EXIT_FAILURE);
        }
    }
    /* --minscorelist: line i is the least score of query record i; from here on `minscore` is the current record's */
    int32_t *mslist = NULL;
    if (mslist_path) {
        FILE *lf = fopen(mslist_path, "r");
        if (!lf) {
            fprintf(stderr, "Error: couldn't open the score list %s\n", mslist_path);
            return leave(EXIT_FAILURE);
        }
        mslist = (int32_t *)calloc(q.n, sizeof *mslist);
        if (!mslist) return leave(EXIT_FAILURE);
        size_t n_read = 0;
        unsigned long line_no = 0;
        char line[4096], msg[512];
        while (fgets(line, sizeof line, lf)) {
            line_no++;
            char *b = line, *e = line + strlen(line);
            while (*b == ' ' || *b == '\t') b++;
            while (e > b && (e[-1] == '\n' || e[-1] == '\r' || e[-1] == ' ' || e[-1] == '\t')) e--;
            *e = 0;
            if (e <= b && feof(lf)) break; /* (a trailing empty line is no line) */
            long val = 0;
            if (n_read >= q.n) {
                snprintf(msg, sizeof msg, "--minscorelist %s line %lu: the query file has %lu records, one line each", mslist_path, line_no,
                         (unsigned long)q.n);
                (void)leave(0);
                usage(argv[0], msg);
            }
            if (!parse_int(b, 1, INT_MAX, &val)) {
                snprintf(msg, sizeof msg, "--minscorelist %s line %lu: '%s' is not a least score (an integer of 1 or more)", mslist_path, line_no, b);
                (void)leave(0);
                usage(argv[0], msg);
            }
            mslist[n_read++] = (int32_t)val;
        }
        fclose(lf);
        if (n_read < q.n) {
            snprintf(msg, sizeof msg, "--minscorelist %s line %lu is missing: the query file has %lu records, one line each", mslist_path,
                     (unsigned long)n_read + 1, (unsigned long)q.n);
            (void)leave(0);
            usage(argv[0], msg);
        }
        minscore = mslist[0];
    } else if (ev_batch) {
        mslist = (int32_t *)calloc(q.n, sizeof *mslist);
        if (!mslist) return leave(EXIT_FAILURE);
        minscore = 1;
    }
    /* --evalue: every record's fit, the residues E counts over, and with --allqueries every record as table indices */
    swg_evalue_params *ev = NULL;
    uint64_t ev_residues = 0;
    int8_t *ev_qx = NULL;
    if (have_evalue && !(ev = (swg_evalue_params *)calloc(q.n, sizeof *ev))) return leave(EXIT_FAILURE);
    /* --candidates: record r's entries are cands[c_off[r] .. c_off[r + 1]) in the file's order; lsc is parallel to cands
     * (swg_search_lists' scores_out), and `listed` marks the current record's entries for the printing */
    uint32_t *cands = NULL;
    uint64_t *c_off = NULL;
    int32_t *lsc = NULL;
    if (cand_path) {
        FILE *lf = fopen(cand_path, "r");
        if (!lf) {
            fprintf(stderr, "Error: couldn't open the candidate list %s\n", cand_path);
            return leave(EXIT_FAILURE);
        }
        uint32_t *rec = NULL, *ent = NULL; /* the lines as they come */
        size_t n_lines = 0, cap = 0;
        unsigned long line_no = 0;
        char line[4096];
        while (fgets(line, sizeof line, lf)) {
            line_no++;
            char *b = line, *e = strchr(line, '#');
            if (!e) e = line + strlen(line);
            while (*b == ' ' || *b == '\t') b++;
            while (e > b && (e[-1] == '\n' || e[-1] == '\r' || e[-1] == ' ' || e[-1] == '\t')) e--;
            if (e <= b) continue;
            *e = 0;
            char *t2 = b;
            while (*t2 && *t2 != ' ' && *t2 != '\t') t2++;
            if (*t2) *t2++ = 0;
            while (*t2 == ' ' || *t2 == '\t') t2++;
            char *end = NULL;
            const unsigned long long rn = strtoull(b, &end, 10);
            if (*b < '0' || *b > '9' || *end != 0 || rn >= (unsigned long long)q.n) {
                char msg[512];
                snprintf(msg, sizeof msg, "--candidates %s line %lu: '%s' is not a query record number of this query file (0..%lu)",
                         cand_path, line_no, b, (unsigned long)q.n - 1);
                (void)leave(0);
                usage(argv[0], msg);
            }
            const unsigned long long en = strtoull(t2, &end, 10);
            if (*t2 < '0' || *t2 > '9' || *end != 0 || en >= (unsigned long long)db.n) {
                char msg[512];
                snprintf(msg, sizeof msg, "--candidates %s line %lu: '%s' is not an entry number of this database (0..%lu)", cand_path,
                         line_no, t2, (unsigned long)db.n - 1);
                (void)leave(0);
                usage(argv[0], msg);
            }
            if (n_lines == cap) {
                cap = cap ? 2 * cap : 1024;
                uint32_t *g1 = (uint32_t *)realloc(rec, cap * sizeof *rec);
                if (g1) rec = g1;
                uint32_t *g2 = (uint32_t *)realloc(ent, cap * sizeof *ent);
                if (g2) ent = g2;
                if (!g1 || !g2) return leave(EXIT_FAILURE);
            }
            rec[n_lines] = (uint32_t)rn;
            ent[n_lines++] = (uint32_t)en;
        }
        fclose(lf);
        c_off = (uint64_t *)calloc(q.n + 2, sizeof *c_off);
        cands = (uint32_t *)malloc((n_lines ? n_lines : 1) * sizeof *cands);
        lsc = (int32_t *)calloc(n_lines ? n_lines : 1, sizeof *lsc);
        listed = (unsigned char *)calloc(db.n ? db.n : 1, 1);
        if (!c_off || !cands || !lsc || !listed) {
            fprintf(stderr, "Error: out of memory\n");
            return leave(EXIT_FAILURE);
        }
        for (size_t l = 0; l < n_lines; l++) c_off[rec[l] + 2]++; /* (counting sort by record, the file's order kept) */
        for (size_t r = 0; r < q.n; r++) c_off[r + 2] += c_off[r + 1];
        for (size_t l = 0; l < n_lines; l++) cands[c_off[rec[l] + 1]++] = ent[l];
        free(rec);
        free(ent);
    }
    /* --prefilter: the lists are made by the gapless search, record by record as the chunks come; they take the place
     * of --candidates' lists from there on (pf_hits: the gapless top-N of one chunk's records) */
    const size_t pf_n = prefilter ? ((size_t)prefilter < db.n ? (size_t)prefilter : db.n) : 0;
    swg_hit *pf_hits = NULL;
    size_t *pf_nhits = NULL;
    if (prefilter) {
        const size_t cap = q.n * (pf_n ? pf_n : 1);
        c_off = (uint64_t *)calloc(q.n + 2, sizeof *c_off);
        cands = (uint32_t *)malloc(cap * sizeof *cands);
        lsc = (int32_t *)calloc(cap, sizeof *lsc);
        if (!listed) listed = (unsigned char *)calloc(db.n ? db.n : 1, 1);
        if (!c_off || !cands || !lsc || !listed) {
            fprintf(stderr, "Error: out of memory\n");
            return leave(EXIT_FAILURE);
        }
    }
    const size_t lq = (size_t)q.seq_off[1];
    int8_t *qidx = (int8_t *)malloc(lq);
    int8_t *didx = (int8_t *)malloc(db.n && !packed ? (size_t)db.seq_off[db.n] + 1 : 1);
    if (!qidx || !didx) {
        fprintf(stderr, "Error: out of memory\n");
        return leave(EXIT_FAILURE);
    }
    char bad = 0;
    {
        swg_seqs q1 = q;
        q1.n = 1;
        if (swg_seqs_to_indices(&q1, qidx, &bad) != SWG_OK) die_illegal(bad);
    }
    /* --pssm: the PSSM's residue column must spell the query record (case aside) */
    int8_t *pssm = NULL;
    if (pssm_path) {
        int8_t *pq = NULL;
        size_t plq = 0;
        if (swg_pssm_load(pssm_path, &sc, &pssm, &pq, &plq, err, sizeof err) != SWG_OK) {
            fprintf(stderr, "Error: %s\n", err);
            return leave(EXIT_FAILURE);
        }
        size_t at = 0;
        while (at < lq && at < plq && pq[at] == qidx[at]) at++;
        swg_pssm_free(NULL, pq);
        if (at < lq || plq != lq) {
            fprintf(stderr, "Error: the PSSM %s (%lu positions) does not spell the query (%lu residues): they differ at position %lu\n",
                    pssm_path, (unsigned long)plq, (unsigned long)lq, (unsigned long)at + 1);
            return leave(EXIT_FAILURE);
        }
    }
    /* --pssmlist: one PSSM per query record, line i of the list names record i's; each must spell its record.
     * Every record's rows go into one array, record i's from row q.seq_off[i] on (a batch's offsets are its records'). */
    int8_t *plist = NULL;
    if (pssmlist_path) {
        FILE *lf = fopen(pssmlist_path, "r");
        if (!lf) {
            fprintf(stderr, "Error: couldn't open the PSSM list %s\n", pssmlist_path);
            return leave(EXIT_FAILURE);
        }
        char **names = NULL;
        size_t n_names = 0, cap = 0;
        char line[4096];
        while (fgets(line, sizeof line, lf)) {
            char *b = line, *e = line + strlen(line);
            while (*b == ' ' || *b == '\t') b++;
            while (e > b && (e[-1] == '\n' || e[-1] == '\r' || e[-1] == ' ' || e[-1] == '\t')) e--;
            if (e == b) continue; /* (blank lines name nothing) */
            *e = 0;
            if (n_names == cap) {
                cap = cap ? 2 * cap : 64;
                char **grown = (char **)realloc(names, cap * sizeof *names);
                if (!grown) return leave(EXIT_FAILURE);
                names = grown;
            }
            if (!(names[n_names++] = strdup(b))) return leave(EXIT_FAILURE);
        }
        fclose(lf);
        if (n_names != q.n) {
            fprintf(stderr, "Error: the PSSM list %s names %lu PSSMs for %lu query records\n", pssmlist_path,
                    (unsigned long)n_names, (unsigned long)q.n);
            return leave(EXIT_FAILURE);
        }
        plist = (int8_t *)malloc((size_t)q.seq_off[q.n] * 32);
        if (!plist) {
            fprintf(stderr, "Error: out of memory\n");
            return leave(EXIT_FAILURE);
        }
        for (size_t r = 0; r < q.n; r++) {
            int8_t *pr = NULL, *pq = NULL;
            size_t plq = 0;
            if (swg_pssm_load(names[r], &sc, &pr, &pq, &plq, err, sizeof err) != SWG_OK) {
                fprintf(stderr, "Error: PSSM list entry %lu (query record #%lu): %s\n", (unsigned long)r + 1, (unsigned long)r, err);
                return leave(EXIT_FAILURE);
            }
            const char *rs = q.seq + q.seq_off[r];
            const size_t rl = (size_t)(q.seq_off[r + 1] - q.seq_off[r]);
            size_t at = 0;
            for (; at < rl && at < plq; at++) {
                const int c = swg_letter_index((unsigned char)rs[at]);
                if (c < 0) die_illegal(rs[at]);
                if (pq[at] != c) break;
            }
            if (at < rl || plq != rl) {
                fprintf(stderr, "Error: the PSSM %s (list entry %lu, %lu positions) does not spell query record #%lu (%lu residues): "
                        "they differ at position %lu\n", names[r], (unsigned long)r + 1, (unsigned long)plq, (unsigned long)r,
                        (unsigned long)rl, (unsigned long)at + 1);
                return leave(EXIT_FAILURE);
            }
            memcpy(plist + (size_t)q.seq_off[r] * 32, pr, rl * 32);
            swg_pssm_free(pr, pq);
            free(names[r]);
        }
        free(names);
    }
    const int8_t *pssm0 = pssm ? pssm : plist; /* the first record's PSSM, if any */
    int8_t *iter_pssm = NULL;                  /* --iterations: the PSSM of the last iteration that built one (then pssm0) */
    swg_query_sanitize(&sc, qidx, lq); /* reference src/alignment_cmdline.c:391-396 */
    if (maskquery && mask_query(qidx, lq, &mp) != SWG_OK) {
        fprintf(stderr, "Error: %s\n", swg_global_error());
        return leave(EXIT_FAILURE);
    }
    if (!packed && swg_seqs_to_indices(&db, didx, &bad) != SWG_OK) die_illegal(bad);

    phase("letters to table indices");
    int32_t *scores = (int32_t *)calloc(n_entries ? n_entries : 1, sizeof(int32_t));
    /* --minscore without --topk: room for every entry searched */
    const size_t hit_cap = topk ? (size_t)topk : minscore ? (ids ? n_ids : n_entries) : 0;
    swg_hit *hits = (swg_hit *)calloc(hit_cap ? hit_cap : 1, sizeof(swg_hit));
    int32_t *adj = (int32_t *)calloc(hit_cap ? hit_cap : 1, sizeof(int32_t)); /* --compstats: the adjusted scores beside the current record's hits */
    double comp_freq[32];                                                     /* ... and its background under --compfromdb */
    if (!scores || !hits) {
        fprintf(stderr, "Error: out of memory\n");
        return leave(EXIT_FAILURE);
    }
    size_t n_hits = 0;
    uint64_t n_above = 0; /* --minscore: the entries at or above it, reported or not */
    double total_ms = 0.0;
    swg_ctx *ctx = NULL;
    swg_group *grp = NULL;
    swg_db *sdb = NULL; /* what is searched: the database, or with --seqidlist the view of its listed entries */
    swg_db *mdb = NULL; /* --softmask: the masked copy, */
    swg_db *ntdb = NULL; /* --translatedb: the nucleotide database the frames were made from */
    swg_db *gdb = NULL; /* ... and what the gapless prefilter reads: the copy, or with --seqidlist the view of its listed entries */
    /* --minscore --gpus N: a context, a shard and what is searched of it per GPU; sh_of[i] = the shard hit i came from */
    size_t sh_n = 0;
    swg_ctx **sh_ctx = NULL;
    swg_db **sh_db = NULL, **sh_sdb = NULL;
    uint32_t *sh_of = NULL;
    if (gpus > 0 && minscore) {
        /* --minscore over several GPUs: every GPU searches its shard (swg_search_above has no group form), the shards'
         * lists are merged in the library's order */
        sh_n = (size_t)gpus;
        sh_ctx = (swg_ctx **)calloc(sh_n, sizeof *sh_ctx);
        sh_db = (swg_db **)calloc(sh_n, sizeof *sh_db);
        sh_sdb = (swg_db **)calloc(sh_n, sizeof *sh_sdb);
        sh_of = (uint32_t *)calloc(hit_cap ? hit_cap : 1, sizeof *sh_of);
        uint64_t *keys = (uint64_t *)malloc((hit_cap ? hit_cap : 1) * sh_n * sizeof *keys);
        uint32_t *key_sh = (uint32_t *)malloc((hit_cap ? hit_cap : 1) * sh_n * sizeof *key_sh);
        if (!sh_ctx || !sh_db || !sh_sdb || !sh_of || !keys || !key_sh) return leave(EXIT_FAILURE);
        int rc = swg_db_pack_shards(didx, db.seq_off, db.n, (int)gpus, sh_db);
        if (rc != SWG_OK) {
            fprintf(stderr, "Error: %s\n", swg_global_error());
            return leave(EXIT_FAILURE);
        }
        phase("sort, shard and pack");
        size_t n_keys = 0;
        for (size_t g = 0; g < sh_n; g++) {
            swg_config cfg;
            memset(&cfg, 0, sizeof cfg);
            cfg.device = (int)g;
            if (swg_create(&cfg, &sh_ctx[g]) != SWG_OK) {
                fprintf(stderr, "Error: %s\n", swg_global_error());
                return leave(EXIT_FAILURE);
            }
            swg_ctx *c = sh_ctx[g];
            rc = swg_set_option(c, "autotune", 0);
            if (rc == SWG_OK) rc = swg_set_scoring(c, (const int8_t(*)[32])sc.sub, sc.gap_open, sc.gap_extend);
            if (rc == SWG_OK) rc = pssm0 ? swg_set_query_pssm(c, pssm0, lq) : swg_set_query(c, qidx, lq);
            if (rc == SWG_OK) rc = swg_db_upload(c, sh_db[g]);
            sh_sdb[g] = sh_db[g];
            if (rc == SWG_OK && ids) rc = swg_db_view(c, sh_db[g], ids, n_ids, &sh_sdb[g]); /* (the entries of other shards are ignored) */
            if (rc != SWG_OK) {
                fprintf(stderr, "Error: %s\n", swg_last_error(c));
                return leave(EXIT_FAILURE);
            }
        }
        if (have_evalue) { /* calibrated once, on the first GPU; E counts over the residues of all shards */
            uint64_t counts[32] = {0}, part[32];
            for (size_t g = 0; g < sh_n; g++) {
                ev_residues += swg_db_residues(sh_sdb[g]);
                if (!compfromdb) continue;
                if (swg_db_composition(sh_ctx[g], sh_sdb[g], part) != SWG_OK) {
                    fprintf(stderr, "Error: %s\n", swg_last_error(sh_ctx[g]));
                    return leave(EXIT_FAILURE);
                }
                for (int r = 0; r < 32; r++) counts[r] += part[r];
            }
            int32_t one = 0;
            if (!evalue_scores(sh_ctx[0], &q, 1, NULL, NULL, gapless, compfromdb ? counts : NULL, ev_residues, evalue, ev, &one))
                return leave(EXIT_FAILURE);
            minscore = one;
            phase("calibrate (E-value to least score)");
        }
        for (size_t g = 0; g < sh_n; g++) {
            swg_ctx *c = sh_ctx[g];
            swg_stats st;
            memset(&st, 0, sizeof st);
            size_t got = 0;
            uint64_t above = 0;
            rc = gapless ? swg_search_gapless_above(c, sh_sdb[g], (int32_t)minscore, hits, hit_cap, &got, &above, &st)
                         : swg_search_above(c, sh_sdb[g], (int32_t)minscore, hits, hit_cap, &got, &above, &st);
            if (rc != SWG_OK) {
                fprintf(stderr, "Error: %s\n", swg_last_error(c));
                return leave(EXIT_FAILURE);
            }
            for (size_t i = 0; i < got; i++) keys[n_keys] = swg_hit_key(hits[i].score, hits[i].index), key_sh[n_keys++] = (uint32_t)g;
            n_above += above;
            total_ms += st.total_ms; /* (one after another) */
        }
        phase("search (shard by shard)");
        /* the best hit_cap of the shards' lists, each sorted already: pick the largest head hit_cap times */
        size_t *head = (size_t *)calloc(sh_n + 1, sizeof *head), *end = (size_t *)calloc(sh_n + 1, sizeof *end);
        if (!head || !end) return leave(EXIT_FAILURE);
        for (size_t i = 0, g = 0; g < sh_n; g++) {
            head[g] = i;
            while (i < n_keys && key_sh[i] == g) i++;
            end[g] = i;
        }
        for (n_hits = 0; n_hits < hit_cap; n_hits++) {
            size_t best = sh_n;
            for (size_t g = 0; g < sh_n; g++)
                if (head[g] < end[g] && (best == sh_n || keys[head[g]] > keys[head[best]])) best = g;
            if (best == sh_n) break;
            swg_key_hit(keys[head[best]++], &hits[n_hits]);
            sh_of[n_hits] = (uint32_t)best;
        }
        free(head);
        free(end);
        free(keys);
        free(key_sh);
    } else if (gpus > 0) {
        /* database sharded over several GPUs of this process */
        swg_stats *st = (swg_stats *)calloc((size_t)gpus, sizeof(swg_stats));
        if (!st) return leave(EXIT_FAILURE);
        int rc = swg_group_create(NULL, (int)gpus, 0, &grp);
        if (rc != SWG_OK) {
            fprintf(stderr, "Error: %s\n", swg_global_error());
            return leave(EXIT_FAILURE);
        }
        phase("create contexts");
        /* one search per query length: timing candidate geometries first would cost more than it saves */
        rc = swg_group_set_option(grp, "autotune", 0);
        if (rc == SWG_OK) rc = swg_group_set_scoring(grp, (const int8_t(*)[32])sc.sub, sc.gap_open, sc.gap_extend);
        if (rc == SWG_OK) rc = pssm0 ? swg_group_set_query_pssm(grp, pssm0, lq) : swg_group_set_query(grp, qidx, lq);
        if (rc == SWG_OK) rc = swg_group_load(grp, didx, db.seq_off, db.n);
        phase("pack, shard and upload");
        if (rc == SWG_OK && ids) {
            rc = swg_group_select(grp, ids, n_ids);
            phase("select the listed entries");
        }
        if (rc == SWG_OK) rc = swg_group_search(grp, scores, hits, (size_t)topk, &n_hits, st);
        phase("search");
        if (rc != SWG_OK) {
            fprintf(stderr, "Error: %s\n", swg_group_last_error(grp));
            return leave(EXIT_FAILURE);
        }
        for (long g = 0; g < gpus; g++)
            if (st[g].total_ms > total_ms) total_ms = st[g].total_ms; /* the GPUs run side by side */
        free(st);
    } else {
        swg_stats st;
        memset(&st, 0, sizeof st);
        int rc = SWG_OK;
        if (!packed) { /* host only: still beside the context's creation */
            rc = swg_db_pack(didx, db.seq_off, db.n, 0, 1, &pdb);
            if (rc != SWG_OK) fprintf(stderr, "Error: %s\n", swg_global_error());
            phase("sort and pack");
        }
        if (g_job_started) {
            (void)leave(0);
        } else {
            ctx_job_run(&job);
        }
        ctx = job.ctx;
        if (job.rc != SWG_OK) {
            fprintf(stderr, "Error: %s\n", job.err);
            return leave(EXIT_FAILURE);
        }
        if (timing) fprintf(stderr, "[timing] %-28s %9.2f ms (on its own thread, beside the phases above)\n", "create context", job.ms);
        phase("wait for the context");
        /* one search per query length: timing candidate geometries first would cost more than it saves */
        if (rc == SWG_OK) rc = swg_set_option(ctx, "autotune", 0);
        if (rc == SWG_OK) rc = swg_set_scoring(ctx, (const int8_t(*)[32])sc.sub, sc.gap_open, sc.gap_extend);
        if (rc == SWG_OK) rc = pssm0 ? swg_set_query_pssm(ctx, pssm0, lq) : swg_set_query(ctx, qidx, lq);
        if (rc == SWG_OK && savedb && !(maskdb && !softmask)) {
            if (swg_db_save(pdb, savedb) != SWG_OK) {
                fprintf(stderr, "Error: %s\n", swg_global_error());
                return leave(EXIT_FAILURE);
            }
            fprintf(stderr, "packed database written to %s\n", savedb);
        }
        if (rc == SWG_OK) rc = swg_db_upload(ctx, pdb);
        phase("upload");
        if (rc == SWG_OK && translatedb) { /* every stage reads the six frames; the nucleotide database stays for its records' lengths */
            swg_translate_info ti;
            ntdb = pdb;
            pdb = NULL;
            rc = swg_db_translate(ctx, ntdb, &tp, &pdb);
            if (rc == SWG_OK && swg_db_translate_info(pdb, &ti) == SWG_OK) {
                fprintf(stderr, "translated %lu entries into %lu frames: %llu codons, %llu stops, %llu with a non-base\n", (unsigned long)swg_db_count(ntdb),
                        (unsigned long)swg_db_count(pdb), (unsigned long long)ti.codons, (unsigned long long)ti.stops,
                        (unsigned long long)ti.unknown_codons);
                if (timing)
                    fprintf(stderr, "[timing] %-28s %9.2f ms of kernel, %.2f ms for the host image\n", "translate the database", ti.kernel_ms,
                            ti.host_image_ms);
            }
            phase("translate the database");
        }
        if (rc == SWG_OK && maskdb) {
            swg_mask_info mi;
            rc = swg_db_mask(ctx, pdb, &mp, &mdb);
            if (rc == SWG_OK && swg_db_mask_info(mdb, &mi) == SWG_OK) {
                fprintf(stderr, "masked %llu residues in %llu of %lu entries (%llu regions; window %d, %g / %g bits)\n",
                        (unsigned long long)mi.residues_masked, (unsigned long long)mi.sequences_masked, (unsigned long)swg_db_count(mdb),
                        (unsigned long long)mi.segments, (int)mp.window, mp.trigger, mp.extend);
                if (timing)
                    fprintf(stderr, "[timing] %-28s %9.2f ms of kernels, %.2f ms for the host image\n", "mask the database", mi.kernel_ms,
                            mi.host_image_ms);
            }
            if (rc == SWG_OK && !softmask) { /* every stage reads the masked copy */
                swg_db_free(pdb);
                pdb = mdb;
                mdb = NULL;
                if (savedb) {
                    if (swg_db_save(pdb, savedb) != SWG_OK) {
                        fprintf(stderr, "Error: %s\n", swg_global_error());
                        return leave(EXIT_FAILURE);
                    }
                    fprintf(stderr, "packed database (masked) written to %s\n", savedb);
                }
            }
            phase("mask the database");
        }
        sdb = pdb;
        if (rc == SWG_OK && ids) {
            rc = swg_db_view(ctx, pdb, ids, n_ids, &sdb);
            phase("select the listed entries");
        }
        gdb = sdb;
        if (rc == SWG_OK && mdb) { /* --softmask: the same selection of the masked copy */
            gdb = mdb;
            if (ids) rc = swg_db_view(ctx, mdb, ids, n_ids, &gdb);
        }
        if (rc == SWG_OK && iterations) { /* every iteration but the last: calibrate, include, build the PSSM, make it the query */
            uint64_t counts[32];
            double freq[32];
            if (compfromdb) rc = swg_db_composition(ctx, sdb, counts);
            for (int r = 0; r < 32; r++) freq[r] = compfromdb && rc == SWG_OK ? (double)counts[r] : 0.0;
            swg_hit *inc = (swg_hit *)calloc((size_t)maxincluded, sizeof *inc);
            unsigned char *was = (unsigned char *)calloc(db.n ? db.n : 1, 1); /* the entries the previous iteration included */
            iter_pssm = (int8_t *)malloc(lq * 32);
            if (!inc || !was || !iter_pssm) return leave(EXIT_FAILURE);
            if (rc == SWG_OK && psiblocks) rc = swg_set_option(ctx, "pssm_blocks", 1);
            if (rc == SWG_OK && purge) rc = swg_set_option(ctx, "pssm_purge", purge);
            if (rc == SWG_OK && compstats) rc = swg_set_option(ctx, "comp_scale", compstats);
            for (long it = 1; rc == SWG_OK && it < iterations; it++) {
                swg_evalue_params p;
                size_t n_inc = 0, n_new = 0;
                uint64_t n_at = 0;
                rc = swg_calibrate(ctx, compfromdb ? freq : NULL, 0, &p);
                if (rc != SWG_OK) break;
                const int32_t least = swg_evalue_min_score(&p, swg_db_residues(sdb), inclusion);
                if (least < 1) {
                    fprintf(stderr, "Error: iteration %ld: the query could not be calibrated (fit status %d): no least score for --inclusion %g\n", it,
                            p.status, inclusion);
                    return leave(EXIT_FAILURE);
                }
                rc = swg_search_above(ctx, sdb, least, inc, (size_t)maxincluded, &n_inc, &n_at, NULL);
                if (rc != SWG_OK) break;
                if (compstats && n_inc) { /* an entry stays only if the E-value of its ADJUSTED score is within --inclusion */
                    swg_comp_result *cr = (swg_comp_result *)malloc(n_inc * sizeof *cr);
                    if (!cr) return leave(EXIT_FAILURE);
                    rc = swg_comp_adjust(ctx, sdb, inc, n_inc, compfromdb ? freq : NULL, cr, NULL);
                    size_t kept = 0;
                    for (size_t h = 0; rc == SWG_OK && h < n_inc; h++) {
                        const double e = swg_evalue(&p, swg_db_residues(sdb), cr[h].adj_score);
                        if (e <= inclusion) {
                            inc[kept++] = inc[h];
                            continue;
                        }
                        fprintf(stderr, "iteration %ld: entry %u leaves by its composition: score %d adjusted to %d (ratio %.4f), E-value %g\n", it,
                                inc[h].index, inc[h].score, cr[h].adj_score, cr[h].ratio16 / 65536.0, e);
                    }
                    free(cr);
                    if (rc != SWG_OK) break;
                    fprintf(stderr, "iteration %ld: %lu of %lu entries stay after the composition-based adjustment\n", it, (unsigned long)kept,
                            (unsigned long)n_inc);
                    n_inc = kept;
                }
                for (size_t h = 0; h < n_inc; h++) n_new += !was[inc[h].index];
                fprintf(stderr, "iteration %ld: %lu entries at or above score %d (E-value %g), %lu included, %lu of them new\n", it,
                        (unsigned long)n_at, least, inclusion, (unsigned long)n_inc, (unsigned long)n_new);
                if (it > 1 && n_new == 0) {
                    fprintf(stderr, "iteration %ld includes no entry beyond iteration %ld's: the iterations end here\n", it, it - 1);
                    break;
                }
                memset(was, 0, db.n ? db.n : 1);
                for (size_t h = 0; h < n_inc; h++) was[inc[h].index] = 1;
                /* the context's query is the record itself (no residues to name) or a PSSM (--pssm, or the iteration before) */
                rc = swg_pssm_build(ctx, sdb, inc, n_inc, pssm0 ? qidx : NULL, compfromdb ? freq : NULL, SWG_PSSM_PSEUDOCOUNT_DEFAULT,
                                    iter_pssm, NULL, NULL);
                if (rc == SWG_OK) rc = swg_set_query_pssm(ctx, iter_pssm, lq);
                if (rc == SWG_OK) pssm0 = iter_pssm;
            }
            free(inc);
            free(was);
            if (rc == SWG_OK && out_pssm) { /* (iteration 1 always builds one) */
                if (swg_pssm_save(out_pssm, iter_pssm, qidx, lq) != SWG_OK) {
                    fprintf(stderr, "Error: %s\n", swg_global_error());
                    return leave(EXIT_FAILURE);
                }
            }
            phase("iterations (calibrate, include, build the PSSM)");
        }
        if (rc == SWG_OK && have_evalue) { /* the least score of the query, or of every record, from its calibration */
            uint64_t counts[32];
            if (compfromdb) rc = swg_db_composition(ctx, sdb, counts);
            if (rc == SWG_OK && allq && !plist) { /* every record as table indices, record i from q.seq_off[i] on */
                ev_qx = (int8_t *)malloc((size_t)q.seq_off[q.n] + 1);
                if (!ev_qx) return leave(EXIT_FAILURE);
                for (size_t r = 0; r < q.n; r++) {
                    for (uint64_t c = q.seq_off[r]; c < q.seq_off[r + 1]; c++) {
                        const int ix = swg_letter_index((unsigned char)q.seq[c]);
                        if (ix < 0) die_illegal(q.seq[c]);
                        ev_qx[c] = (int8_t)ix;
                    }
                    swg_query_sanitize(&sc, ev_qx + q.seq_off[r], (size_t)(q.seq_off[r + 1] - q.seq_off[r]));
                    if (maskquery && mask_query(ev_qx + q.seq_off[r], (size_t)(q.seq_off[r + 1] - q.seq_off[r]), &mp) != SWG_OK) return leave(EXIT_FAILURE);
                }
            }
            if (rc == SWG_OK) {
                int32_t one = 0;
                /* --translatedb: tblastn's convention, the nucleotides / 3 (= the six frames / 6, up to rounding) */
                ev_residues = translatedb ? swg_db_residues(ntdb) / 3 : swg_db_residues(sdb);
                if (!evalue_scores(ctx, &q, allq ? q.n : 1, ev_qx, allq ? plist : NULL, gapless, compfromdb ? counts : NULL, ev_residues, evalue, ev,
                                   allq ? mslist : &one))
                    return leave(EXIT_FAILURE);
                minscore = allq ? mslist[0] : one;
            }
            phase("calibrate (E-value to least score)");
        }
        if (rc == SWG_OK && prefilter) { /* the first record's candidates: its gapless top-N */
            memset(listed, 0, db.n ? db.n : 1); /* (--seqidlist's marks: no Entry lines here, the marks count the candidates) */
            pf_hits = (swg_hit *)calloc(pf_n ? pf_n : 1, sizeof *pf_hits);
            size_t got = 0;
            if (!pf_hits) return leave(EXIT_FAILURE);
            rc = swg_search_gapless(ctx, gdb, NULL, pf_hits, pf_n, &got, NULL);
            for (size_t i = 0; rc == SWG_OK && i < got; i++) cands[i] = pf_hits[i].index;
            c_off[1] = got;
            free(pf_hits);
            pf_hits = NULL;
            phase("prefilter (gapless top-N)");
        }
        if (rc == SWG_OK && cands) { /* the first record against its own entries */
            const uint64_t off01[2] = {0, lq};
            rc = pssm0 ? swg_search_lists_pssm(ctx, sdb, pssm0, off01, 1, cands, c_off, lsc, hits, (size_t)topk, &n_hits, &st)
                       : swg_search_lists(ctx, sdb, qidx, off01, 1, cands, c_off, lsc, hits, (size_t)topk, &n_hits, &st);
        } else if (rc == SWG_OK && minscore) {
            rc = gapless ? swg_search_gapless_above(ctx, sdb, (int32_t)minscore, hits, hit_cap, &n_hits, &n_above, &st)
                         : swg_search_above(ctx, sdb, (int32_t)minscore, hits, hit_cap, &n_hits, &n_above, &st);
        } else if (rc == SWG_OK) {
            rc = gapless ? swg_search_gapless(ctx, sdb, scores, hits, (size_t)topk, &n_hits, &st)
                         : swg_search(ctx, sdb, scores, hits, (size_t)topk, &n_hits, &st);
        }
        phase("search (first of this database)");
        if (rc != SWG_OK) {
            fprintf(stderr, "Error: %s\n", swg_last_error(ctx));
            return leave(EXIT_FAILURE);
        }
        total_ms = st.total_ms;
        if (compstats) { /* the first record's hits, against the context's query */
            uint64_t counts[32];
            if (!adj) return leave(EXIT_FAILURE);
            if (compfromdb && swg_db_composition(ctx, sdb, counts) != SWG_OK) {
                fprintf(stderr, "Error: %s\n", swg_last_error(ctx));
                return leave(EXIT_FAILURE);
            }
            for (int r = 0; r < 32; r++) comp_freq[r] = compfromdb ? (double)counts[r] : 0.0;
            if (comp_rerank(ctx, sdb, compstats, NULL, 0, NULL, 1, hits, hit_cap ? hit_cap : 1, &n_hits, compfromdb ? comp_freq : NULL, adj,
                            have_evalue ? ev : NULL, ev_residues, evalue) != SWG_OK) {
                fprintf(stderr, "Error: %s\n", swg_last_error(ctx));
                return leave(EXIT_FAILURE);
            }
            phase("composition-based adjustment (first record)");
        }
    }

    /* reference src/tools/sw_cmdline.c:38-75: per 16 records the query lines, then per record */
    const char *qname = q.names + q.name_off[0];
    size_t qi = 0;
    /* --allqueries --align: the alignments of queries [al_first, al_first + al_n) of the current chunk, hit j of query
     * al_first + i at mq_al[i*topk + j] and mq_ops + (i*topk + j)*al_stride */
    swg_alignment *mq_al = NULL;
    char *mq_ops = NULL;
    size_t al_first = 0, al_n = 0, al_stride = 0, al_records = 0, al_calls = 0;
    double al_ms = 0.0;
    /* after a failed call: one record per call, and the error of the record that fails is reported where its
     * alignments would print, after its own search results (as when each record was aligned on its own) */
    int al_one_by_one = 0, al_failed = 0;
    char al_err[512] = "";
    /* --allqueries --bounds: the coordinates of queries [bd_first, bd_first + bd_n) of the current chunk, hit j of query
     * bd_first + i at mq_bd[i*topk + j] */
    swg_alignment *mq_bd = NULL;
    swg_align_counts *mq_ct = NULL; /* --tabular: the counts beside them */
    size_t bd_first = 0, bd_n = 0;
    struct hsps hs = {NULL, NULL, NULL, NULL, 1, 0}; /* --maxhsps: the current record's alignments (a later record's come with its results, below) */
next_query:
    if (cands) { /* this record's entries: marks for the printing, scores by entry */
        if (qi > 0)
            for (uint64_t e = c_off[qi - 1]; e < c_off[qi]; e++) listed[cands[e]] = 0;
        n_listed = 0;
        for (uint64_t e = c_off[qi]; e < c_off[qi + 1]; e++) {
            if (!listed[cands[e]]) listed[cands[e]] = 1, n_listed++;
            scores[cands[e]] = lsc[e];
        }
    }
    if (allq) printf("Query #%lu: %s\n", (unsigned long)qi, qname);
    for (size_t i = 0, shown = 0; i < db.n && !prefilter && !minscore && !translatedb; i++) {
        if (listed && !listed[i]) continue;
        if (shown++ % 16 == 0) {
            if (print_fasta) {
                fputs(qname, stdout);
                putc('\n', stdout);
            }
            if (print_seq) {
                fwrite(q.seq + q.seq_off[qi], 1, (size_t)(q.seq_off[qi + 1] - q.seq_off[qi]), stdout);
                putc('\n', stdout);
            }
        }
        printf("Entry #%lu:\n", (unsigned long)i);
        if (print_fasta) {
            fputs(db.names + db.name_off[i], stdout);
            putc('\n', stdout);
        }
        if (print_seq) {
            fwrite(db.seq + db.seq_off[i], 1, (size_t)(db.seq_off[i + 1] - db.seq_off[i]), stdout);
            putc('\n', stdout);
        }
        printf("score: %i\n\n", scores[i]);
    }
    /* reference src/alignment_cmdline.c:529-530; the time is the device time of the fill */
    printf("Total Time: %f\n", total_ms * 1e-3);
    printf("Total Entries: %lu\n", (unsigned long)(listed ? n_listed : n_entries));
    if (have_evalue)
        printf("E-value %g: lambda %.4f, K %.4f, least score %ld over %llu residues\n", evalue, ev[qi].lambda, ev[qi].K, minscore,
               (unsigned long long)ev_residues);
    if (minscore) printf("Entries at or above %ld: %llu\n", minscore, (unsigned long long)n_above);
    if (topk > 0 || minscore) {
        if (compstats) { /* ranked by adjusted score; both scores */
            printf("Top %lu hits (adjusted score, score, entry, name):\n", (unsigned long)n_hits);
            for (size_t i = 0; i < n_hits; i++)
                printf("%d\t%d\t%u\t%s\n", adj[i], hits[i].score, hits[i].index, packed ? "" : db.names + db.name_off[hits[i].index]);
        } else if (translatedb) { /* the nucleotide record and the frame of it */
            printf("Top %lu hits (score, entry, frame, name):\n", (unsigned long)n_hits);
            for (size_t i = 0; i < n_hits; i++) {
                uint32_t rec;
                int fr;
                swg_translate_hit(hits[i].index, &rec, &fr);
                printf("%d\t%u\t%s\t%s\n", hits[i].score, rec, frame_names[fr], packed ? "" : db.names + db.name_off[rec]);
            }
        } else {
            printf("Top %lu hits (score, entry, name):\n", (unsigned long)n_hits);
            for (size_t i = 0; i < n_hits; i++)
                printf("%d\t%u\t%s\n", hits[i].score, hits[i].index, packed ? "" : db.names + db.name_off[hits[i].index]);
        }
    }
    if (align && n_hits > 0) {
        /* the first record against the context's query; the others were aligned with their chunk (below) */
        size_t stride = al_stride;
        swg_alignment *al = NULL;
        char *ops = NULL;
        if (qi > 0 && al_failed) {
            fprintf(stderr, "Error: %s\n", al_err);
            return leave(EXIT_FAILURE);
        }
        if (maxhsps) { /* (the first record's against the context's query) */
            if (qi == 0 && hsps_run(&hs, ctx, sdb, NULL, 0, NULL, hits, n_hits, maxhsps, hspscore ? hspscore : minscore ? minscore : 1) != SWG_OK)
                return leave(EXIT_FAILURE);
            stride = hs.stride;
        } else if (sh_n) { /* --minscore --gpus N: every hit is aligned on the GPU that holds its shard */
            stride = 1;
            for (size_t g = 0; g < sh_n; g++) {
                const size_t b = swg_align_ops_bound(sh_ctx[g], sh_sdb[g]);
                if (b > stride) stride = b;
            }
            al = (swg_alignment *)calloc(n_hits, sizeof *al);
            ops = (char *)malloc(n_hits * stride);
            swg_hit *part = (swg_hit *)calloc(n_hits, sizeof *part);
            swg_alignment *part_al = (swg_alignment *)calloc(n_hits, sizeof *part_al);
            char *part_ops = (char *)malloc(n_hits * stride);
            if (!al || !ops || !part || !part_al || !part_ops) return leave(EXIT_FAILURE);
            for (size_t g = 0; g < sh_n; g++) {
                size_t m = 0;
                for (size_t i = 0; i < n_hits; i++)
                    if (sh_of[i] == g) part[m++] = hits[i];
                if (m == 0) continue;
                if (swg_align_hits(sh_ctx[g], sh_sdb[g], part, m, part_al, part_ops, stride) != SWG_OK) {
                    fprintf(stderr, "Error: %s\n", swg_last_error(sh_ctx[g]));
                    return leave(EXIT_FAILURE);
                }
                m = 0;
                for (size_t i = 0; i < n_hits; i++)
                    if (sh_of[i] == g) {
                        al[i] = part_al[m];
                        memcpy(ops + i * stride, part_ops + m * stride, stride);
                        m++;
                    }
            }
            free(part);
            free(part_al);
            free(part_ops);
        } else if (qi == 0) {
            stride = grp ? swg_group_align_ops_bound(grp) : swg_align_ops_bound(ctx, sdb);
            al = (swg_alignment *)calloc(n_hits, sizeof *al);
            ops = (char *)malloc(n_hits * stride);
            if (!al || !ops) return leave(EXIT_FAILURE);
            if ((grp ? swg_group_align_hits(grp, hits, n_hits, al, ops, stride)
                     : swg_align_hits(ctx, sdb, hits, n_hits, al, ops, stride)) != SWG_OK) {
                fprintf(stderr, "Error: %s\n", grp ? swg_group_last_error(grp) : swg_last_error(ctx));
                return leave(EXIT_FAILURE);
            }
        }
        const swg_alignment *al_q = maxhsps ? hs.al : al ? al : mq_al + (qi - al_first) * (size_t)topk;
        const char *ops_q = maxhsps ? hs.ops : ops ? ops : mq_ops + (qi - al_first) * (size_t)topk * stride;
        char *line = (char *)malloc(stride);
        if (!line) return leave(EXIT_FAILURE);
        /* one block per hit; with --maxhsps hit i's hs.n[i] blocks one after another, all under the hit's number */
        for (size_t e = 0; e < n_hits * hs.per; e++) {
            const size_t i = e / hs.per;
            if (maxhsps && e % hs.per >= hs.n[i]) continue;
            const swg_alignment *a = &al_q[e];
            const char *o = ops_q + e * stride;
            uint32_t rec = a->index;
            int fr = 0;
            if (translatedb) { /* the frame's protein alignment under the record and the frame; the coordinates are the frame's residues */
                swg_translate_hit(a->index, &rec, &fr);
                printf("Alignment #%lu: entry %u frame %s score %d query %u..%u frame residues %u..%u\n", (unsigned long)i, rec, frame_names[fr],
                       a->score, a->q_begin, a->q_end, a->d_begin, a->d_end);
            } else {
                printf("Alignment #%lu: entry %u score %d query %u..%u entry %u..%u\n", (unsigned long)i, a->index,
                       a->score, a->q_begin, a->q_end, a->d_begin, a->d_end);
            }
            if (packed) { /* no letters in a packed database: the path itself */
                printf("%s\n\n", o);
                continue;
            }
            char *fl = NULL;
            if (translatedb && !(fl = frame_letters(didx + db.seq_off[rec], (size_t)(db.seq_off[rec + 1] - db.seq_off[rec]), fr, &tp)))
                return leave(EXIT_FAILURE);
            const char *qs = q.seq + q.seq_off[qi] + a->q_begin, *ds = (fl ? fl : db.seq + db.seq_off[a->index]) + a->d_begin;
            size_t c = 0;
            for (uint32_t k = 0; k < a->n_ops; k++) line[k] = o[k] == 'I' ? '-' : qs[c++];
            line[a->n_ops] = 0;
            printf("%s\n", line);
            c = 0;
            for (uint32_t k = 0; k < a->n_ops; k++) line[k] = o[k] == 'D' ? '-' : ds[c++];
            printf("%s\n\n", line);
            free(fl);
        }
        free(al);
        free(ops);
        free(line);
    }
    if ((bounds || tabular) && n_hits > 0) {
        /* the first record against the context's query; the others came with their chunk (below) */
        swg_alignment *bd = NULL;
        swg_align_counts *ct = NULL;
        if (maxhsps) { /* (--maxhsps --align is refused with either: this is the record's one call) */
            if (qi == 0 && hsps_run(&hs, ctx, sdb, NULL, 0, NULL, hits, n_hits, maxhsps, hspscore ? hspscore : minscore ? minscore : 1) != SWG_OK)
                return leave(EXIT_FAILURE);
        } else if (qi == 0) {
            bd = (swg_alignment *)calloc(n_hits, sizeof *bd);
            ct = (swg_align_counts *)calloc(n_hits, sizeof *ct);
            if (!bd || !ct) return leave(EXIT_FAILURE);
            if ((tabular ? swg_align_stats(ctx, sdb, hits, n_hits, bd, ct) : swg_align_bounds(ctx, sdb, hits, n_hits, bd)) != SWG_OK) {
                fprintf(stderr, "Error: %s\n", swg_last_error(ctx));
                return leave(EXIT_FAILURE);
            }
        }
        const swg_alignment *bd_q = maxhsps ? hs.al : bd ? bd : mq_bd + (qi - bd_first) * (size_t)topk;
        const swg_align_counts *ct_q = maxhsps ? hs.ct : bd ? ct : mq_ct + (qi - bd_first) * (size_t)topk;
        /* one line per hit; with --maxhsps hit e / hs.per's hs.n[] lines one after another (hs.per is 1 without it) */
        for (size_t e = 0; e < n_hits * hs.per && bounds; e++) {
            if (maxhsps && e % hs.per >= hs.n[e / hs.per]) continue;
            if (translatedb) { /* the subject in nucleotides of the record, 1-based and inclusive */
                uint32_t rec, s1, e1;
                int fr;
                swg_translate_hit(bd_q[e].index, &rec, &fr);
                nt_span(fr, nt_length(ntdb, &db, packed, rec), &bd_q[e], &s1, &e1);
                printf("Bounds #%lu: entry %u frame %s score %d query %u..%u entry %u..%u length %u\n", (unsigned long)e, rec, frame_names[fr],
                       bd_q[e].score, bd_q[e].q_begin, bd_q[e].q_end, s1, e1, bd_q[e].n_ops);
                continue;
            }
            printf("Bounds #%lu: entry %u score %d query %u..%u entry %u..%u length %u\n", (unsigned long)(e / hs.per), bd_q[e].index,
                   bd_q[e].score, bd_q[e].q_begin, bd_q[e].q_end, bd_q[e].d_begin, bd_q[e].d_end, bd_q[e].n_ops);
        }
        if (tabular && have_evalue)
            printf("# Fields: query, entry, pident, length, mismatch, gapopen, qstart, qend, sstart, send, evalue, bitscore, score%s\n",
                   translatedb ? ", sframe" : "");
        else if (tabular)
            printf("# Fields: query, entry, pident, length, mismatch, gapopen, qstart, qend, sstart, send, score%s\n", translatedb ? ", sframe" : "");
        for (size_t i = 0; i < n_hits * hs.per && tabular; i++) {
            if (maxhsps && i % hs.per >= hs.n[i / hs.per]) continue;
            const swg_alignment *a = &bd_q[i];
            if (a->score <= 0) continue; /* no alignment: no line */
            /* --compstats: the score columns are the adjusted ones (line i is hit i: --maxhsps is refused beside it); the
             * coordinates and counts stay those of the unadjusted alignment */
            const int32_t shown = compstats ? adj[i] : a->score;
            if (translatedb) { /* the nucleotide record, its coordinates (1-based, inclusive, start above end on a minus frame), the frame last */
                uint32_t rec, s1, e1;
                int fr;
                swg_translate_hit(a->index, &rec, &fr);
                nt_span(fr, nt_length(ntdb, &db, packed, rec), a, &s1, &e1);
                printf("%s\t%s\t%.2f\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t", qname, packed ? "" : db.names + db.name_off[rec],
                       100.0 * ct_q[i].n_ident / a->n_ops, a->n_ops, ct_q[i].n_match - ct_q[i].n_ident, ct_q[i].n_gap_open, a->q_begin + 1,
                       a->q_end, s1, e1);
                if (have_evalue) printf("%.3g\t%.1f\t", swg_evalue(&ev[qi], ev_residues, shown), swg_bitscore(&ev[qi], shown));
                printf("%d\t%s\n", shown, frame_names[fr]);
                continue;
            }
            if (have_evalue) { /* BLAST's twelve columns, then the raw score */
                printf("%s\t%s\t%.2f\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%.3g\t%.1f\t%d\n", qname, packed ? "" : db.names + db.name_off[a->index],
                       100.0 * ct_q[i].n_ident / a->n_ops, a->n_ops, ct_q[i].n_match - ct_q[i].n_ident, ct_q[i].n_gap_open, a->q_begin + 1,
                       a->q_end, a->d_begin + 1, a->d_end, swg_evalue(&ev[qi], ev_residues, shown), swg_bitscore(&ev[qi], shown), shown);
                continue;
            }
            printf("%s\t%s\t%.2f\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%d\n", qname, packed ? "" : db.names + db.name_off[a->index],
                   100.0 * ct_q[i].n_ident / a->n_ops, a->n_ops, ct_q[i].n_match - ct_q[i].n_ident, ct_q[i].n_gap_open,
                   a->q_begin + 1, a->q_end, a->d_begin + 1, a->d_end, shown);
        }
        free(bd);
        free(ct);
    }
    if (allq && ++qi < q.n) {
        /* The database stays resident; the remaining queries go through swg_search_multi in chunks (one
         * launch per class for a whole chunk: a small database is filled with many queries at once),
         * results are kept per query and printed in order.  With --pssmlist the chunk's PSSMs go through
         * swg_search_multi_pssm instead. */
        static int32_t *mq_scores = NULL;
        static swg_hit *mq_hits = NULL;
        static size_t *mq_nhits = NULL;
        static int32_t *mq_adj = NULL; /* --compstats: the adjusted scores beside mq_hits */
        static uint64_t *mq_above = NULL; /* --minscorelist: every record's entries at or above its score */
        static size_t chunk_first = 0, chunk_n = 0;
        static double chunk_ms = 0.0;
        static int8_t *qx = NULL;     /* the chunk's queries as table indices */
        static uint64_t *qoff = NULL;
        if (qi >= chunk_first + chunk_n) {
            size_t budget = cands ? 1024 : ((size_t)256 << 20) / (sizeof(int32_t) * (n_entries ? n_entries : 1));
            if (budget < 1) budget = 1;
            if (budget > 1024) budget = 1024;
            chunk_first = qi;
            chunk_n = q.n - qi < budget ? q.n - qi : budget;
            const size_t nres = (size_t)(q.seq_off[chunk_first + chunk_n] - q.seq_off[chunk_first]);
            free(qx);
            free(qoff);
            qx = (int8_t *)malloc(nres ? nres : 1);
            qoff = (uint64_t *)malloc((chunk_n + 1) * sizeof(uint64_t));
            free(mq_scores);
            free(mq_hits);
            free(mq_nhits);
            free(mq_above);
            mq_above = (uint64_t *)calloc(chunk_n, sizeof(uint64_t));
            mq_scores = (int32_t *)calloc(cands || mslist ? 1 : chunk_n * (n_entries ? n_entries : 1), sizeof(int32_t)); /* (--candidates: lsc) */
            mq_hits = (swg_hit *)calloc(chunk_n * (topk ? (size_t)topk : 1), sizeof(swg_hit));
            mq_nhits = (size_t *)calloc(chunk_n, sizeof(size_t));
            free(mq_adj);
            mq_adj = (int32_t *)calloc(chunk_n * (topk ? (size_t)topk : 1), sizeof(int32_t));
            if (!mq_adj) return leave(EXIT_FAILURE);
            if (!qx || !qoff || !mq_scores || !mq_hits || !mq_nhits || !mq_above) return leave(EXIT_FAILURE);
            for (size_t i = 0; i <= chunk_n; i++) qoff[i] = q.seq_off[chunk_first + i] - q.seq_off[chunk_first];
            for (size_t i = 0; i < chunk_n; i++) {
                const size_t lqi = (size_t)(qoff[i + 1] - qoff[i]);
                if (lqi == 0) {
                    fprintf(stderr, "Error: query #%lu is empty\n", (unsigned long)(chunk_first + i));
                    return leave(EXIT_FAILURE);
                }
                for (size_t c = 0; c < lqi; c++) {
                    const char ch = q.seq[q.seq_off[chunk_first + i] + c];
                    const int v = swg_letter_index((unsigned char)ch);
                    if (v < 0) die_illegal(ch);
                    qx[qoff[i] + c] = (int8_t)v;
                }
                swg_query_sanitize(&sc, qx + qoff[i], lqi);
                if (maskquery && mask_query(qx + qoff[i], lqi, &mp) != SWG_OK) return leave(EXIT_FAILURE);
            }
            swg_stats st;
            memset(&st, 0, sizeof st);
            int rc;
            if (prefilter) { /* the chunk's candidate lists: each record's gapless top-N, appended behind the lists so far */
                const double t0 = now_ms();
                free(pf_hits);
                free(pf_nhits);
                pf_hits = (swg_hit *)calloc(chunk_n * (pf_n ? pf_n : 1), sizeof *pf_hits);
                pf_nhits = (size_t *)calloc(chunk_n, sizeof *pf_nhits);
                if (!pf_hits || !pf_nhits) return leave(EXIT_FAILURE);
                rc = plist ? swg_search_gapless_multi_pssm(ctx, gdb, plist + (size_t)q.seq_off[chunk_first] * 32, qoff, chunk_n, NULL,
                                                           pf_hits, pf_n, pf_nhits, NULL)
                           : swg_search_gapless_multi(ctx, gdb, qx, qoff, chunk_n, NULL, pf_hits, pf_n, pf_nhits, NULL);
                if (rc != SWG_OK) {
                    fprintf(stderr, "Error: %s\n", swg_last_error(ctx));
                    return leave(EXIT_FAILURE);
                }
                for (size_t i = 0; i < chunk_n; i++) {
                    const uint64_t at0 = c_off[chunk_first + i];
                    for (size_t j = 0; j < pf_nhits[i]; j++) cands[at0 + j] = pf_hits[i * pf_n + j].index;
                    c_off[chunk_first + i + 1] = at0 + pf_nhits[i];
                }
                if (timing)
                    fprintf(stderr, "[timing] prefilter (gapless top-N) of %lu queries: %.3f ms\n", (unsigned long)chunk_n, now_ms() - t0);
            }
            if (cands) /* every record of the chunk against its own entries, in one pass */
                rc = plist ? swg_search_lists_pssm(ctx, sdb, plist + (size_t)q.seq_off[chunk_first] * 32, qoff, chunk_n, cands,
                                                   c_off + chunk_first, lsc, mq_hits, (size_t)topk, mq_nhits, &st)
                           : swg_search_lists(ctx, sdb, qx, qoff, chunk_n, cands, c_off + chunk_first, lsc, mq_hits, (size_t)topk,
                                              mq_nhits, &st);
            else if (mslist) { /* every record of the chunk at its own least score: no score array, K hits of room each */
                const int8_t *pl = plist ? plist + (size_t)q.seq_off[chunk_first] * 32 : NULL;
                const int32_t *ms = mslist + chunk_first;
                if (gapless)
                    rc = plist ? swg_search_gapless_above_multi_pssm(ctx, sdb, pl, qoff, chunk_n, ms, mq_hits, (size_t)topk, mq_nhits, mq_above, &st)
                               : swg_search_gapless_above_multi(ctx, sdb, qx, qoff, chunk_n, ms, mq_hits, (size_t)topk, mq_nhits, mq_above, &st);
                else
                    rc = plist ? swg_search_above_multi_pssm(ctx, sdb, pl, qoff, chunk_n, ms, mq_hits, (size_t)topk, mq_nhits, mq_above, &st)
                               : swg_search_above_multi(ctx, sdb, qx, qoff, chunk_n, ms, mq_hits, (size_t)topk, mq_nhits, mq_above, &st);
            } else if (gapless)
                rc = plist ? swg_search_gapless_multi_pssm(ctx, sdb, plist + (size_t)q.seq_off[chunk_first] * 32, qoff, chunk_n, mq_scores,
                                                           mq_hits, (size_t)topk, mq_nhits, &st)
                           : swg_search_gapless_multi(ctx, sdb, qx, qoff, chunk_n, mq_scores, mq_hits, (size_t)topk, mq_nhits, &st);
            else
                rc = plist ? swg_search_multi_pssm(ctx, sdb, plist + (size_t)q.seq_off[chunk_first] * 32, qoff, chunk_n, mq_scores,
                                                   mq_hits, (size_t)topk, mq_nhits, &st)
                           : swg_search_multi(ctx, sdb, qx, qoff, chunk_n, mq_scores, mq_hits, (size_t)topk, mq_nhits, &st);
            if (rc != SWG_OK) {
                fprintf(stderr, "Error: %s\n", swg_last_error(ctx));
                return leave(EXIT_FAILURE);
            }
            if (compstats && comp_rerank(ctx, sdb, compstats, plist ? plist + (size_t)q.seq_off[chunk_first] * 32 : qx, plist != NULL, qoff, chunk_n,
                                         mq_hits, topk ? (size_t)topk : 1, mq_nhits, compfromdb ? comp_freq : NULL, mq_adj,
                                         have_evalue ? ev + chunk_first : NULL, ev_residues, evalue) != SWG_OK) {
                fprintf(stderr, "Error: %s\n", swg_last_error(ctx));
                return leave(EXIT_FAILURE);
            }
            chunk_ms = st.total_ms / (double)chunk_n; /* the chunk's device time, shared out over its queries */
            if (timing)
                fprintf(stderr, "[timing] %lu queries in one pass: %.3f ms of fill, %.1f GCUPS\n", (unsigned long)chunk_n,
                        st.fill_ms, st.fill_ms > 0 ? (double)st.cells / (st.fill_ms * 1e-3) / 1e9 : 0.0);
        }
        const size_t at = qi - chunk_first;
        if (!cands && !mslist) memcpy(scores, mq_scores + at * (n_entries ? n_entries : 1), n_entries * sizeof(int32_t));
        if (mslist) minscore = mslist[qi], n_above = mq_above[at];
        n_hits = mq_nhits[at];
        memcpy(hits, mq_hits + at * (topk ? (size_t)topk : 1), n_hits * sizeof(swg_hit));
        if (compstats) memcpy(adj, mq_adj + at * (topk ? (size_t)topk : 1), n_hits * sizeof(int32_t));
        if (maxhsps && n_hits > 0) { /* this record's alignments, against its own query or PSSM */
            const double t0 = now_ms();
            if (hsps_run(&hs, ctx, sdb, plist ? plist + (size_t)q.seq_off[chunk_first] * 32 : qx, plist != NULL, qoff + at, hits, n_hits, maxhsps,
                         hspscore ? hspscore : minscore ? minscore : 1) != SWG_OK)
                return leave(EXIT_FAILURE);
            al_ms += now_ms() - t0, ++al_calls, ++al_records;
        }
        if (align && !maxhsps && qi >= al_first + al_n) {
            /* The alignments of the chunk's hits from this query on, in one swg_align_hits_multi call (with --pssmlist
             * swg_align_hits_multi_pssm: each record against its own PSSM).  A call takes at most 2^20 hits, and its
             * paths are kept to about 256 MB, so a chunk past either is aligned in several calls. */
            const size_t left = chunk_first + chunk_n - qi, kk = (size_t)topk;
            al_first = qi;
            al_stride = swg_align_ops_bound_multi(sdb, qoff + at, left);
            size_t per = ((size_t)256 << 20) / (kk * al_stride);
            if (per > ((size_t)1 << 20) / kk) per = ((size_t)1 << 20) / kk;
            if (per < 1 || al_one_by_one) per = 1;
            al_n = left < per ? left : per;
            free(mq_al);
            free(mq_ops);
            mq_al = (swg_alignment *)calloc(al_n * kk, sizeof *mq_al);
            mq_ops = (char *)malloc(al_n * kk * al_stride);
            if (!mq_al || !mq_ops) {
                fprintf(stderr, "Error: out of memory\n");
                return leave(EXIT_FAILURE);
            }
            for (;;) {
                const double t0 = now_ms();
                const int rc = plist ? swg_align_hits_multi_pssm(ctx, sdb, plist + (size_t)q.seq_off[chunk_first] * 32, qoff + at,
                                                                 al_n, mq_hits + at * kk, kk, mq_nhits + at, mq_al, mq_ops, al_stride)
                                     : swg_align_hits_multi(ctx, sdb, qx, qoff + at, al_n, mq_hits + at * kk, kk, mq_nhits + at,
                                                            mq_al, mq_ops, al_stride);
                al_ms += now_ms() - t0, ++al_calls;
                if (rc == SWG_OK) break;
                if (al_n == 1) {
                    snprintf(al_err, sizeof al_err, "%s", swg_last_error(ctx));
                    al_failed = 1;
                    break;
                }
                /* a record of this call cannot be aligned: the records before it still print first */
                al_one_by_one = 1, al_n = 1;
            }
            al_records += al_n;
        }
        if ((bounds || tabular) && !maxhsps && qi >= bd_first + bd_n) {
            /* the coordinates of the chunk's hits from this query on, in one swg_align_bounds_multi call (with --pssmlist
             * swg_align_bounds_multi_pssm); a call takes at most 2^20 hits */
            const size_t left = chunk_first + chunk_n - qi, kk = (size_t)topk;
            size_t per = ((size_t)1 << 20) / kk;
            if (per < 1) per = 1;
            bd_first = qi;
            bd_n = left < per ? left : per;
            free(mq_bd);
            free(mq_ct);
            mq_bd = (swg_alignment *)calloc(bd_n * kk, sizeof *mq_bd);
            mq_ct = (swg_align_counts *)calloc(bd_n * kk, sizeof *mq_ct);
            if (!mq_bd || !mq_ct) {
                fprintf(stderr, "Error: out of memory\n");
                return leave(EXIT_FAILURE);
            }
            const double t0 = now_ms();
            const int8_t *pl = plist ? plist + (size_t)q.seq_off[chunk_first] * 32 : NULL;
            const int rc = tabular ? (plist ? swg_align_stats_multi_pssm(ctx, sdb, pl, qoff + at, bd_n, mq_hits + at * kk, kk,
                                                                         mq_nhits + at, mq_bd, mq_ct)
                                            : swg_align_stats_multi(ctx, sdb, qx, qoff + at, bd_n, mq_hits + at * kk, kk,
                                                                    mq_nhits + at, mq_bd, mq_ct))
                           : plist ? swg_align_bounds_multi_pssm(ctx, sdb, pl, qoff + at, bd_n, mq_hits + at * kk, kk, mq_nhits + at, mq_bd)
                                   : swg_align_bounds_multi(ctx, sdb, qx, qoff + at, bd_n, mq_hits + at * kk, kk, mq_nhits + at, mq_bd);
            if (rc != SWG_OK) {
                fprintf(stderr, "Error: %s\n", swg_last_error(ctx));
                return leave(EXIT_FAILURE);
            }
            if (timing) fprintf(stderr, "[timing] bounds of %lu records in one call: %.3f ms\n", (unsigned long)bd_n, now_ms() - t0);
        }
        total_ms = chunk_ms;
        qname = q.names + q.name_off[qi];
        goto next_query;
    }
    if (timing && al_calls)
        fprintf(stderr, "[timing] %lu records aligned in %lu calls: %.3f ms\n", (unsigned long)al_records,
                (unsigned long)al_calls, al_ms);
    fflush(stdout);
    phase("print");
    /* The run is over and its output is out: the process ends here, without walking the runtime's teardown (streams,
     * device buffers, the runtime's own exit handlers: 25-40 ms of a 200 ms run) -- the kernel driver releases a dead
     * process's device resources anyway.  SWG_CLI_RELEASE=1 takes the long way (leak checkers want it). */
    if (!getenv("SWG_CLI_RELEASE")) {
        fflush(stderr);
        _exit(leave(EXIT_SUCCESS));
    }
    if (gdb != sdb && gdb != mdb) swg_db_free(gdb);
    swg_db_free(mdb);
    if (sdb != pdb) swg_db_free(sdb);
    swg_db_free(pdb);
    swg_db_free(ntdb);
    swg_destroy(ctx);
    swg_group_destroy(grp);
    for (size_t g = 0; g < sh_n; g++) {
        if (sh_sdb[g] != sh_db[g]) swg_db_free(sh_sdb[g]);
        swg_db_free(sh_db[g]);
        swg_destroy(sh_ctx[g]);
    }
    free(sh_ctx);
    free(sh_db);
    free(sh_sdb);
    free(sh_of);
    swg_seqs_free(&q);
    swg_seqs_free(&db);
    free(qidx);
    swg_pssm_free(pssm, NULL);
    free(plist);
    free(didx);
    free(ids);
    free(listed);
    free(cands);
    free(c_off);
    free(lsc);
    free(mslist);
    free(ev);
    free(ev_qx);
    free(pf_hits);
    free(pf_nhits);
    free(scores);
    free(hits);
    free(mq_al);
    free(mq_ops);
    free(mq_bd);
    free(hs.al);
    free(hs.ct);
    free(hs.n);
    free(hs.ops);
    phase("release (context, buffers)");
    return leave(EXIT_SUCCESS);
}
