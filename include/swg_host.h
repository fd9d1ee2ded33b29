/*
 * swg_host.h -- plain-C host helpers that sit beside the hot path: the pieces of
 * the reference's driver a caller needs to feed swg.h.  None of them touches a
 * GPU.  Each cites the reference code whose behaviour it mirrors; the reference's
 * own FASTA and line readers (libs/seq_file, libs/string_buffer) are un-vendored
 * submodules that are absent from the reference tree, so parsing parity is
 * pinned only by SURVEY A.5/A.6, not by reference code.
 */
#ifndef SWG_HOST_H
#define SWG_HOST_H

#include <stddef.h>
#include <stdint.h>

#include "swg.h" /* swg_alignment, swg_pssm_info */

#ifdef __cplusplus
extern "C" {
#endif

/* ---- scoring (reference src/alignment_scoring.{h,c}) ------------------- */

typedef struct swg_scoring {
    int gap_open, gap_extend; /* scoring_t.gap_open/gap_extend */
    int match, mismatch;      /* parsed by the CLI, unused by the fill */
    int8_t sub[32][32];       /* scoring_t.swap_scores, zero-initialised here (A.7-1) */
    uint32_t set[32];         /* scoring_t.swap_set: bit b of set[a] <=> (a,b) defined */
} swg_scoring;

/* Residue -> table index, reference letters_to_index (src/alignment_scoring.c:70-81):
 * a-z/A-Z -> 1..26, '*' -> 31; returns -1 where the reference calls exit(1). */
int swg_letter_index(int c);
/* Inverse, reference index_to_letters (src/alignment_scoring.c:83-92); 0 if illegal. */
int swg_index_letter(int idx);

/* Defaults of the smith_waterman tool (src/tools/sw_cmdline.c:27-35):
 * match 2, mismatch -2, gap_open -2, gap_extend -1; empty table. */
void swg_scoring_init(swg_scoring *sc);
/* reference scoring_add_mutation (src/alignment_scoring.c:60-68); returns
 * SWG_ERR_ARG instead of asserting when score is outside -127..127 or a letter
 * is illegal. */
int swg_scoring_add(swg_scoring *sc, int a, int b, int score);
/* reference align_scoring_load_matrix (src/alignment_scoring_load.c:57-215),
 * file format in SURVEY A.5; gz-transparent like the reference's gzopen
 * (src/alignment_cmdline.c:230).  On error returns SWG_ERR_IO and a message
 * in err (the reference prints and exits). */
int swg_scoring_load_matrix(swg_scoring *sc, const char *path, char *err, size_t errlen);

/* PSI-BLAST's ASCII PSSM (psiblast -out_ascii_pssm): free text, then a header line whose first 20 whitespace
 * tokens are single letters (the score columns; what follows them, such as the percentages, is ignored), then one
 * line per query position, `pos letter s1 .. s20 [anything]` with pos = 1, 2, 3, ..., up to the first blank line
 * (the Lambda/K footer after it is not read).  -> *pssm_out [lq*32] in swg_set_query_pssm's layout: the header's
 * columns from the file, every other residue code b (B, J, O, U, X, Z, '*', ...) sc->sub[query residue][b],
 * column 0 zero; *query_out [lq] the residue column as table indices.  gzip-transparent.  On a missing header,
 * a value outside -128..127, a gap in the positions, an illegal residue letter or a short line: SWG_ERR_IO and a
 * message naming the line in err.  Release both buffers with swg_pssm_free. */
int swg_pssm_load(const char *path, const swg_scoring *sc, int8_t **pssm_out, int8_t **query_out, size_t *lq_out,
                  char *err, size_t errlen);
void swg_pssm_free(int8_t *pssm, int8_t *query);

/* Query sanitisation of the reference driver (src/alignment_cmdline.c:391-396):
 * a residue whose self-pair is undefined in the table becomes 'X'. */
void swg_query_sanitize(const swg_scoring *sc, int8_t *idx, size_t n);

/* ---- sequence files (reference: libs/seq_file via src/alignment_cmdline.c:335-457) */

typedef struct swg_seqs {
    size_t n;
    char *names;        /* NUL-separated header texts (without '>'/'@') */
    uint64_t *name_off; /* [n+1] */
    char *seq;          /* concatenated residue letters, no newlines */
    uint64_t *seq_off;  /* [n+1] */
} swg_seqs;

/* FASTA (multi-line), FASTQ, or one sequence per line; gzip-transparent;
 * "-" reads stdin.  max_records 0 = all. */
int swg_seqs_read(const char *path, size_t max_records, swg_seqs *out, char *err, size_t errlen);
void swg_seqs_free(swg_seqs *s);
/* letters -> indices for the whole set; on an illegal letter returns
 * SWG_ERR_RESIDUE and stores it in *bad (reference: message + exit(1)). */
int swg_seqs_to_indices(const swg_seqs *s, int8_t *out, char *bad);

/* ---- synthetic protein data (the reference ships no data) --- */

/* splitmix64 streams; residues i.i.d. over the 20 standard amino acids with
 * Swiss-Prot-like frequencies; lengths log-normal(median, sigma_ln) clamped to
 * [min_len, max_len], emitted sorted longest first.  Buffers are malloc'ed
 * here and released with swg_synth_free. */
int swg_synth_db(uint64_t seed, size_t n, double median, double sigma_ln, uint32_t min_len,
                 uint32_t max_len, int8_t **flat_out, uint64_t **offsets_out);
void swg_synth_query(uint64_t seed, size_t lq, int8_t *out);
/* As swg_synth_db, but a seeded `fraction` of the sequences are full-length
 * copies of the query with `subst` point substitutions per residue: the
 * high-similarity set that drives int16 scores into saturation and exercises
 * the int32 re-score path. */
int swg_synth_db_similar(uint64_t seed, size_t n, double median, double sigma_ln, uint32_t min_len,
                         uint32_t max_len, const int8_t *query, size_t lq, double fraction,
                         double subst, int8_t **flat_out, uint64_t **offsets_out, size_t *n_planted);
/* A family of relatives instead of near-copies: as swg_synth_db_similar, but every planted sequence draws
 * its own substitution rate from [subst_lo, subst_hi] (identity 1 - rate: 0.3 .. 0.7 gives scores between
 * the f16 cells' ceiling and int16's for a 3000-aa query).  subst_hi == subst_lo is swg_synth_db_similar. */
int swg_synth_db_family(uint64_t seed, size_t n, double median, double sigma_ln, uint32_t min_len,
                        uint32_t max_len, const int8_t *query, size_t lq, double fraction,
                        double subst_lo, double subst_hi, int8_t **flat_out, uint64_t **offsets_out,
                        size_t *n_planted);
/* One shard of the same database without generating the rest: the sequences of the global bins
 * (128 consecutive sorted ranks) b with b % shard_count == shard_rank -- exactly the bins
 * swg_db_pack(..., shard_rank, shard_count) keeps of the whole database.  offsets_out[n_local+1]
 * are over the shard alone; index_out[n_local] are the sequences' global indices (a sequence is
 * seeded by its global sorted rank, so the union of all shards is byte for byte the database of
 * swg_synth_db / swg_synth_db_similar with the same arguments); residues_total = sum of lengths
 * of the WHOLE database.  fraction == 0: no planted copies (query may be NULL).  Feed the result
 * to swg_db_pack_shard. */
int swg_synth_db_shard(uint64_t seed, size_t n, double median, double sigma_ln, uint32_t min_len,
                       uint32_t max_len, const int8_t *query, size_t lq, double fraction, double subst,
                       int shard_rank, int shard_count, int8_t **flat_out, uint64_t **offsets_out,
                       uint32_t **index_out, size_t *n_local, uint64_t *residues_total, size_t *n_planted);
void swg_synth_free(void *p);
/* The random database a calibration scores against (swg_calibrate): n sequences of exactly len residues each, i.i.d.
 * from freq, in the order generated (offsets_out[i] = i * len).  freq[r] is the weight of residue index r (1..26 for
 * A..Z, 31 for '*'); NULL is the built-in table of swg_synth_db.  The weights must be finite and non-negative, freq[0]
 * (the padding residue) must be 0 and the sum positive; the library normalises.  Anything else, n or len of 0 or NULL
 * outputs: SWG_ERR_ARG.  Residue j of sequence i depends only on (seed, i, j): a longer or larger database with the same
 * seed begins with the same residues.  Release both buffers with swg_synth_free. */
int swg_synth_db_iid(uint64_t seed, size_t n, uint32_t len, const double freq[32], int8_t **flat_out, uint64_t **offsets_out);

/* ---- score statistics (HMMER / SSEARCH style calibration) -------------- */

/* Maximum-likelihood fit of a Gumbel distribution P(S >= x) = 1 - exp(-exp(-lambda (x - mu))) to a histogram of integer
 * scores: hist[s] = how many samples scored s, for s < n_bins.  All in double, bins in ascending order.  With n the
 * number of samples, x0 the lowest populated bin, xbar the mean and var the (population) variance:
 *     lambda_0 = pi / sqrt(6 var);   e_s = hist[s] exp(-lambda (s - x0)),  A = sum e_s,  B = sum s e_s,  D = sum s^2 e_s;
 *     Newton on f = 1/lambda - xbar + B/A with f' = (B/A)^2 - D/A - 1/lambda^2; a step that would make lambda <= 0 halves
 *     lambda instead; it stops once |step| <= 1e-12 lambda, or after 100 steps;   mu = x0 - ln(A/n) / lambda.
 * *n_iter = the steps taken.  Returns 0 for a fit, 1 when fewer than two distinct scores are populated (no fit:
 * *lambda = *mu = 0, *n_iter = 0), 2 when it did not converge (lambda and mu where it stopped), SWG_ERR_ARG for NULL
 * arguments.  The device's fit of swg_calibrate is this one, bin for bin. */
int swg_gumbel_fit_hist(const uint32_t *hist, size_t n_bins, double *lambda, double *mu, int *n_iter);

/* ---- a PSSM from alignments (the model of swg_pssm_build, include/swg.h) -- */

/* The scale of a substitution matrix under a background: the unique lambda > 0 with
 *     sum over a, b in A of P_a P_b exp(lambda sub[a][b]) = 1,
 * P = freq normalised (NULL: the built-in table), A = {a in 1..31 : P_a > 0}; solved in double by bracketing and Newton
 * steps kept inside the bracket until the residual is at most 1e-12.  It exists only if the expected score over A is
 * negative and some sub[a][b] over A is positive: otherwise, and for a malformed freq or a NULL argument, SWG_ERR_ARG
 * with a message in swg_global_error().  BLOSUM62 with the built-in table: 0.3172837580. */
int swg_matrix_lambda(const int8_t sub[32][32], const double *freq, double *lambda);
/* The host twin of swg_pssm_build: the same model, fed by exactly what swg_align_hits* returns -- al[n_hits] with
 * al[i].index an index into flat / offsets (sequence j is flat[offsets[j] .. offsets[j+1]), table indices), the paths
 * at ops + i*ops_stride -- for the query[lq] (table indices 1..31).  Rows and columns are summed in ascending order.
 * pssm_out [lq*32]; values_out NULL or double[lq*32]: the unrounded v, 0 where there is none; info NULL or one record.
 * A path that leaves its pair (a step past the query or the sequence, more steps than n_ops), NULL arguments, a bad
 * freq, a pseudocount that is not finite and positive, a matrix without a lambda: SWG_ERR_ARG with a message in
 * swg_global_error(). */
int swg_pssm_from_paths(const int8_t sub[32][32], const double *freq, double pseudocount, const int8_t *query, size_t lq,
                        const int8_t *flat, const uint64_t *offsets, const swg_alignment *al, const char *ops,
                        size_t ops_stride, size_t n_hits, int8_t *pssm_out, double *values_out, swg_pssm_info *info);
/* The same with the two options of swg_pssm_build (include/swg.h, "per-column blocks" and "purge"): blocks 0 or 1 as
 * option "pssm_blocks", purge 0 or 50..100 as option "pssm_purge"; any other value is SWG_ERR_ARG.  swg_pssm_from_paths
 * is this routine called with 0, 0.  Under blocks = 1 the segments (runs of columns between two consecutive extent
 * boundaries) are taken in ascending order, a block's columns and its member rows likewise. */
int swg_pssm_from_paths_ex(const int8_t sub[32][32], const double *freq, double pseudocount, const int8_t *query, size_t lq,
                           const int8_t *flat, const uint64_t *offsets, const swg_alignment *al, const char *ops,
                           size_t ops_stride, size_t n_hits, int blocks, int purge, int8_t *pssm_out, double *values_out,
                           swg_pssm_info *info);
/* Writes the ASCII layout swg_pssm_load reads: a header of the 20 standard amino acids (A R N D C Q E G H I L K M F P S
 * T W Y V), then `pos letter s1 .. s20` per query position and a blank line.  The other residue codes are not written:
 * swg_pssm_load rebuilds them from the matrix, as swg_pssm_build filled them, so loading the file with the same
 * scoring returns the same bytes.  SWG_ERR_ARG for NULL arguments, lq of 0 or a query residue without a letter;
 * SWG_ERR_IO when the file cannot be written. */
int swg_pssm_save(const char *path, const int8_t *pssm, const int8_t *query, size_t lq);

/* swg_seg_mask (include/swg.h) over a whole database laid end to end, in place and on every core: sequence i is
 * flat[offsets[i] .. offsets[i+1]); masked positions take p->replace (p NULL: the defaults).  What a caller does in
 * front of swg_db_pack where swg_db_mask cannot be used.  totals NULL, or {positions masked, sequences with any,
 * kept runs}. */
int swg_seg_mask_flat(int8_t *flat, const uint64_t *offsets, size_t n, const swg_mask_params *p, uint64_t totals[3]);

/* Threads the host helpers' parallel loops use: the smallest of OpenMP's maximum (OMP_NUM_THREADS),
 * the CPUs this process may run on, and its cgroup CPU quota.  (The reference sizes its loop by
 * omp_get_max_threads() alone, src/alignment_cmdline.c:341-347.) */
int swg_host_threads(void);

#ifdef __cplusplus
}
#endif
#endif /* SWG_HOST_H */
