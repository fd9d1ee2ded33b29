/*
 * swg_scoring.c -- residue map, scoring table and substitution-matrix reader.
 * Host-only C; behaviour mirrors reference src/alignment_scoring.c and
 * src/alignment_scoring_load.c (file format: SURVEY A.5) but returns error
 * codes where the reference prints and exits.
 */
#include "../../include/swg.h"
#include "../../include/swg_host.h"

#include <ctype.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>

int swg_letter_index(int c)
{
    /* reference src/alignment_scoring.c:70-81 */
    if (c >= 'a' && c <= 'z') return c - 'a' + 1;
    if (c >= 'A' && c <= 'Z') return c - 'A' + 1;
    if (c == '*') return 31;
    return -1;
}

int swg_index_letter(int idx)
{
    /* reference src/alignment_scoring.c:83-92 */
    if (idx >= 1 && idx <= 26) return 'A' + idx - 1;
    if (idx == 31) return '*';
    return 0;
}

void swg_scoring_init(swg_scoring *sc)
{
    /* reference src/tools/sw_cmdline.c:27-35; unlike the reference the table
     * starts zeroed (the reference leaves swap_scores uninitialised, A.7-1) */
    memset(sc, 0, sizeof *sc);
    sc->match = 2;
    sc->mismatch = -2;
    sc->gap_open = -2;
    sc->gap_extend = -1;
}

int swg_scoring_add(swg_scoring *sc, int a, int b, int score)
{
    /* reference src/alignment_scoring.c:60-68 */
    const int ia = swg_letter_index(a), ib = swg_letter_index(b);
    if (ia < 0 || ib < 0 || score <= -128 || score >= 128) return SWG_ERR_ARG;
    sc->sub[ia][ib] = (int8_t)score;
    sc->set[ia] |= 1u << ib;
    return SWG_OK;
}

void swg_query_sanitize(const swg_scoring *sc, int8_t *idx, size_t n)
{
    /* reference src/alignment_cmdline.c:391-396 */
    const int8_t x = (int8_t)swg_letter_index('X');
    for (size_t i = 0; i < n; i++) {
        const int a = idx[i];
        if (a < 0 || a > 31 || !((sc->set[a] >> a) & 1u)) idx[i] = x;
    }
}

/* ---- line reader over zlib (plain files pass through gzread unchanged) ---- */
typedef struct {
    gzFile f;
    char *buf;
    size_t cap, len;
} linebuf;

static int lb_next(linebuf *lb)
{
    lb->len = 0;
    for (;;) {
        if (lb->cap - lb->len < 256) {
            size_t ncap = lb->cap ? lb->cap * 2 : 1024;
            char *nb = (char *)realloc(lb->buf, ncap);
            if (!nb) return -1;
            lb->buf = nb;
            lb->cap = ncap;
        }
        if (!gzgets(lb->f, lb->buf + lb->len, (int)(lb->cap - lb->len))) {
            if (lb->len == 0) return 0;
            break;
        }
        lb->len += strlen(lb->buf + lb->len);
        if (lb->len && lb->buf[lb->len - 1] == '\n') break;
    }
    while (lb->len && (lb->buf[lb->len - 1] == '\n' || lb->buf[lb->len - 1] == '\r'))
        lb->buf[--lb->len] = '\0';
    return 1;
}

static int all_space(const char *s)
{
    for (; *s; s++)
        if (!isspace((unsigned char)*s)) return 0;
    return 1;
}

static int fail(char *err, size_t errlen, const char *path, long line, const char *msg)
{
    if (err && errlen) {
        if (line >= 0)
            snprintf(err, errlen, "substitution matrix : %s (file %s, line %ld)", msg, path, line);
        else
            snprintf(err, errlen, "substitution matrix : %s (file %s)", msg, path);
    }
    return SWG_ERR_IO;
}

int swg_scoring_load_matrix(swg_scoring *sc, const char *path, char *err, size_t errlen)
{
    if (!sc || !path) return SWG_ERR_ARG;
    linebuf lb = {0};
    lb.f = gzopen(path, "r");
    if (!lb.f) return fail(err, errlen, path, -1, "couldn't read file");
    int rc = SWG_OK;
    long line = 0;
    int got;
    /* header: first line that is neither empty, all-space nor a '#' comment
     * (src/alignment_scoring_load.c:64-80) */
    while ((got = lb_next(&lb)) > 0) {
        line++;
        if (lb.len > 0 && lb.buf[0] != '#' && !all_space(lb.buf)) break;
    }
    if (got <= 0) {
        rc = fail(err, errlen, path, -1, "empty file");
        goto done;
    }
    if (lb.len < 2) {
        rc = fail(err, errlen, path, line, "too few column headings");
        goto done;
    }
    {
        /* the header's first character is the separator (:88-93) */
        const char sep = lb.buf[0];
        if ((sep >= '0' && sep <= '9') || sep == '-') {
            rc = fail(err, errlen, path, line, "numbers (0-9) and dashes (-) do not make good separators");
            goto done;
        }
        char cols[256];
        int ncols = 0;
        if (isspace((unsigned char)sep)) {
            /* whitespace mode (:98-151) */
            for (const char *p = lb.buf; *p; p++) {
                if (isspace((unsigned char)*p)) continue;
                if (ncols >= 255) {
                    rc = fail(err, errlen, path, line, "too many column headings");
                    goto done;
                }
                cols[ncols++] = *p;
                if (p[1] && !isspace((unsigned char)p[1])) {
                    rc = fail(err, errlen, path, line, "column headings must be single characters");
                    goto done;
                }
            }
            while ((got = lb_next(&lb)) > 0) {
                line++;
                const char *p = lb.buf;
                while (*p && isspace((unsigned char)*p)) p++;
                if (*p == '\0' || lb.buf[0] == '#') continue;
                const char from = *p++;
                for (int i = 0; i < ncols; i++) {
                    if (!isspace((unsigned char)*p)) {
                        rc = fail(err, errlen, path, line,
                                  *p ? "expected whitespace between elements" : "missing number value on line");
                        goto done;
                    }
                    while (*p && isspace((unsigned char)*p)) p++;
                    char *end = NULL;
                    const long v = strtol(p, &end, 10);
                    if (end == p) {
                        rc = fail(err, errlen, path, line, "missing number value on line");
                        goto done;
                    }
                    if (swg_scoring_add(sc, from, cols[i], (int)v) != SWG_OK) {
                        rc = fail(err, errlen, path, line, "illegal residue letter or score outside -127..127");
                        goto done;
                    }
                    p = end;
                }
                if (*p != '\0' && !all_space(p)) {
                    rc = fail(err, errlen, path, line, "too many columns on row");
                    goto done;
                }
            }
        } else {
            /* single-character separator mode (:152-211): "<sep>A<sep>B..." */
            for (size_t i = 0; i < lb.len; i += 2) {
                if (lb.buf[i] != sep || lb.buf[i + 1] == '\0' || ncols >= 255) {
                    rc = fail(err, errlen, path, line, "separator missing from line");
                    goto done;
                }
                cols[ncols++] = lb.buf[i + 1];
            }
            while ((got = lb_next(&lb)) > 0) {
                line++;
                if (lb.buf[0] == '#' || all_space(lb.buf)) continue;
                const char from = lb.buf[0];
                const char *p = lb.buf + 1;
                int i = 0;
                while (*p != '\0') {
                    if (*p != sep) {
                        rc = fail(err, errlen, path, line, "separator missing from line");
                        goto done;
                    }
                    p++;
                    char *end = NULL;
                    const long v = strtol(p, &end, 10);
                    if (end == p) {
                        rc = fail(err, errlen, path, line, "missing number value on line");
                        goto done;
                    }
                    if (i >= ncols) {
                        rc = fail(err, errlen, path, line, "too many columns on row");
                        goto done;
                    }
                    if (swg_scoring_add(sc, from, cols[i++], (int)v) != SWG_OK) {
                        rc = fail(err, errlen, path, line, "illegal residue letter or score outside -127..127");
                        goto done;
                    }
                    p = end;
                }
            }
        }
        if (got < 0) rc = fail(err, errlen, path, line, "out of memory");
    }
done:
    gzclose(lb.f);
    free(lb.buf);
    return rc;
}

/* ---- PSI-BLAST ASCII PSSM (psiblast -out_ascii_pssm) ---------------------- */
static int pssm_fail(char *err, size_t errlen, const char *path, long line, const char *msg)
{
    if (err && errlen) {
        if (line >= 0)
            snprintf(err, errlen, "PSSM : %s (file %s, line %ld)", msg, path, line);
        else
            snprintf(err, errlen, "PSSM : %s (file %s)", msg, path);
    }
    return SWG_ERR_IO;
}

/* splits s in place into at most max whitespace-separated tokens; returns how many */
static int split_ws(char *s, char **tok, int max)
{
    int n = 0;
    while (*s && n < max) {
        while (*s && isspace((unsigned char)*s)) s++;
        if (!*s) break;
        tok[n++] = s;
        while (*s && !isspace((unsigned char)*s)) s++;
        if (*s) *s++ = '\0';
    }
    return n;
}

/* a whole token as a decimal integer */
static int token_long(const char *t, long *v)
{
    char *end = NULL;
    *v = strtol(t, &end, 10);
    return end != t && *end == '\0';
}

int swg_pssm_load(const char *path, const swg_scoring *sc, int8_t **pssm_out, int8_t **query_out, size_t *lq_out,
                  char *err, size_t errlen)
{
    if (!path || !sc || !pssm_out || !query_out || !lq_out) return SWG_ERR_ARG;
    *pssm_out = NULL;
    *query_out = NULL;
    *lq_out = 0;
    linebuf lb = {0};
    lb.f = gzopen(path, "r");
    if (!lb.f) return pssm_fail(err, errlen, path, -1, "couldn't read file");
    int rc = SWG_OK, got;
    long line = 0;
    int cols[20]; /* residue code of each score column */
    int have_header = 0;
    int8_t *pssm = NULL, *query = NULL;
    size_t lq = 0, cap = 0;
    char *tok[22];
    /* header: the first line whose first 20 tokens are single residue letters (the free text before it is skipped) */
    while (!have_header && (got = lb_next(&lb)) > 0) {
        line++;
        const int n = split_ws(lb.buf, tok, 20);
        if (n < 20) continue;
        int ok = 1;
        for (int c = 0; c < 20 && ok; c++) {
            ok = tok[c][1] == '\0' && isalpha((unsigned char)tok[c][0]);
            if (ok) cols[c] = swg_letter_index(tok[c][0]);
        }
        have_header = ok;
    }
    if (!have_header) {
        rc = pssm_fail(err, errlen, path, -1, "no header line (20 single-letter column headings)");
        goto done;
    }
    /* one line per position up to the first blank line: pos letter s1 .. s20 [anything] */
    while ((got = lb_next(&lb)) > 0) {
        line++;
        if (all_space(lb.buf)) break;
        const int n = split_ws(lb.buf, tok, 22);
        long v;
        if (n < 22) {
            rc = pssm_fail(err, errlen, path, line, "expected a position, a residue letter and 20 scores");
            goto done;
        }
        if (!token_long(tok[0], &v) || v != (long)lq + 1) {
            rc = pssm_fail(err, errlen, path, line, "positions must be 1, 2, 3, ... without a gap");
            goto done;
        }
        const int q = tok[1][1] == '\0' ? swg_letter_index(tok[1][0]) : -1;
        if (q < 0) {
            rc = pssm_fail(err, errlen, path, line, "illegal residue letter");
            goto done;
        }
        if (lq == cap) {
            const size_t ncap = cap ? cap * 2 : 256;
            int8_t *np = (int8_t *)realloc(pssm, ncap * 32), *nq;
            if (np) pssm = np;
            nq = np ? (int8_t *)realloc(query, ncap) : NULL;
            if (!np || !nq) {
                rc = pssm_fail(err, errlen, path, line, "out of memory");
                goto done;
            }
            query = nq;
            cap = ncap;
        }
        int8_t *row = pssm + lq * 32;
        /* residues the file has no column for score as the matrix scores them against this position's residue */
        row[0] = 0;
        for (int b = 1; b < 32; b++) row[b] = sc->sub[q][b];
        for (int c = 0; c < 20; c++) {
            if (!token_long(tok[2 + c], &v)) {
                rc = pssm_fail(err, errlen, path, line, "missing or malformed score");
                goto done;
            }
            if (v < -128 || v > 127) {
                rc = pssm_fail(err, errlen, path, line, "score outside -128..127");
                goto done;
            }
            row[cols[c]] = (int8_t)v;
        }
        query[lq++] = (int8_t)q;
    }
    if (got < 0) {
        rc = pssm_fail(err, errlen, path, line, "out of memory");
        goto done;
    }
    if (lq == 0) {
        rc = pssm_fail(err, errlen, path, line, "no positions after the header");
        goto done;
    }
    *pssm_out = pssm;
    *query_out = query;
    *lq_out = lq;
    pssm = query = NULL;
done:
    free(pssm);
    free(query);
    gzclose(lb.f);
    free(lb.buf);
    return rc;
}

void swg_pssm_free(int8_t *pssm, int8_t *query)
{
    free(pssm);
    free(query);
}
