// swg_hsps.hip -- several non-overlapping alignments per hit (swg_align_hsps*): Waterman and Eggert's
// declumping, which upstream seq-align's smith_waterman has and the reference's fork removed with its traceback.
//
// A sibling of swg_trace.hip, by whose launch rule it runs (swg_host_internal.h): one workgroup of 256 lanes per pair
// sweeps the anti-diagonals of the pair's matrix in int32 with one predecessor byte per cell, finds the best match cell
// and one lane walks back -- and then the workgroup goes round again with the residue pairs of the walk's M steps marked
// "used": bit 6 of the cell's predecessor byte, which the next round's fill reads before it overwrites the three 2-bit
// codes of bits 0-5, and keeps.  The H state of a used cell is SWG_HSPS_USED, which neither wins a maximum against 0 nor
// overflows under a gap score of either sign; its A and B states are computed as ever, so a later alignment may cross
// an earlier one through a gap and may not share an aligned residue pair with it.  The rounds of a pair stop at the
// first alignment below min_score or after max_hsps of them.  The traceback's own kernel (swg_trace_kernel) is not
// touched: this one is a unit of its own.
#include "swg_host_internal.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <stdexcept>

struct SwgHspsParams {
    const int8_t *query; // table indices of the batch's queries, back to back (PSSM kernel: unread)
    const int8_t *sub;   // [32][32], row = query residue (PSSM kernel: unread)
    const int8_t *pssm;  // PSSM kernel: the batch's PSSM rows [positions][32]
    const uint8_t *ident; // what identity is counted against, per position: the query's residues, or a PSSM's consensus
    const int8_t *res;   // database residue indices of the jobs' sequences
    const SwgTraceJob *jobs;
    int32_t *diag;       // three rotating anti-diagonals of H, A and B per job (kernels without LDS)
    uint8_t *dir;        // predecessor bytes per job, diagonal-major; bit 6 = the cell is used
    char *ops;           // max_hsps paths per job
    SwgTraceOut *out;    // max_hsps records per job; pad[0] = identical columns, pad[1] = gap runs of the path
    uint32_t *n_out;     // alignments written per job
    int go, ge;
    uint32_t max_hsps;
    int32_t min_score;
};

#define SWG_HSPS_USED (-(1 << 29))
#define SWG_HSPS_MARK 0x40u

// predecessor code of one state: 0 = the alignment starts here, 1/2/3 = came from H/A/B (as swg_trace.hip)
__device__ __forceinline__ uint32_t hsps_pick(int32_t m, int32_t x, int32_t y)
{
    return m == 0 ? 0u : x == m ? 1u : y == m ? 2u : 3u;
}

// IN_LDS, PSSM: as swg_trace_kernel.  Round 0 is a writing round (no byte is read before it was written); a later
// round reads a byte's mark, then writes the codes with the mark kept.
template <bool IN_LDS, bool PSSM>
__global__ __launch_bounds__(SWG_TRACE_THREADS) void swg_hsps_kernel(SwgHspsParams p)
{
    extern __shared__ int32_t s_diag[];
    __shared__ int8_t s_sub[1024];
    __shared__ int s_best;
    __shared__ unsigned long long s_pos;
    __shared__ uint32_t s_n;
    const SwgTraceJob job = p.jobs[blockIdx.x];
    const uint32_t lq = job.lq, len = job.len, tid = threadIdx.x, w = lq + 1;
    const int8_t *query = PSSM ? nullptr : p.query + job.q_off, *pssm = PSSM ? p.pssm + job.q_off * 32 : nullptr;
    const uint8_t *ident = p.ident + job.q_off;
    if (!PSSM)
        for (uint32_t k = tid; k < 1024; k += SWG_TRACE_THREADS) s_sub[k] = p.sub[k];
    int32_t *X;
    if (IN_LDS) X = s_diag;
    else X = p.diag + job.diag_off;
    const int8_t *d = p.res + job.res_off;
    uint8_t *dir = p.dir + job.dir_off;
    const int go = p.go, ge = p.ge;
    const size_t slot_bytes = (size_t)lq + len + 1;
    SwgTraceOut *out = p.out + (size_t)blockIdx.x * p.max_hsps;

    uint32_t r = 0;
    for (; r < p.max_hsps; ++r) {
        // (the lanes read s_best of the round before between its two barriers behind the fill, the walking lane s_pos
        // in front of the barrier behind the walk: both are free again here)
        if (tid == 0) s_best = 0, s_pos = ~0ull;
        __syncthreads();

        // cell (j, i): database row j, query column i, both from 1; anti-diagonal dg = i + j.  The buffers are indexed
        // by i: (j-1, i) and (j, i-1) lie on dg-1 at i and i-1, (j-1, i-1) on dg-2 at i-1.  Every cell read was
        // written in this round.
        int32_t best = 0;
        uint32_t bj = 0, bi = 0;
        for (uint32_t dg = 2; dg <= lq + len; ++dg) {
            const uint32_t c0 = dg % 3, c1 = (dg + 2) % 3, c2 = (dg + 1) % 3;
            int32_t *H0 = X + c0 * w, *A0 = X + (3 + c0) * w, *B0 = X + (6 + c0) * w;
            const int32_t *H1 = X + c1 * w, *A1 = X + (3 + c1) * w, *B1 = X + (6 + c1) * w;
            const int32_t *H2 = X + c2 * w, *A2 = X + (3 + c2) * w, *B2 = X + (6 + c2) * w;
            const uint32_t ilo = dg > len ? dg - len : 1u, ihi = min(lq, dg - 1);
            uint8_t *drow = dir + (size_t)(dg - 2) * lq;
            for (uint32_t i = ilo + tid; i <= ihi; i += SWG_TRACE_THREADS) {
                const uint32_t j = dg - i;
                int32_t hd = 0, ad = 0, bd = 0, hu = 0, au = 0, bu = 0, hl = 0, al = 0, bl = 0;
                if (j > 1) {
                    hu = H1[i], au = A1[i], bu = B1[i];
                    if (i > 1) hd = H2[i - 1], ad = A2[i - 1], bd = B2[i - 1];
                }
                if (i > 1) hl = H1[i - 1], al = A1[i - 1], bl = B1[i - 1];
                const uint32_t mark = r > 0 ? drow[i - 1] & SWG_HSPS_MARK : 0u;
                const int32_t s = PSSM ? (int32_t)pssm[(size_t)(i - 1) * 32 + (int)d[j - 1]]
                                       : (int32_t)s_sub[(int)query[i - 1] * 32 + (int)d[j - 1]];
                const int32_t mh = max(max(hd, ad), max(bd, 0));
                const int32_t xa = hu + go, ya = au + ge, za = bu + go;
                const int32_t ma = max(max(xa, ya), max(za, 0));
                const int32_t xb = hl + go, yb = al + go, zb = bl + ge;
                const int32_t mb = max(max(xb, yb), max(zb, 0));
                drow[i - 1] = (uint8_t)(hsps_pick(mh, hd, ad) | hsps_pick(ma, xa, ya) << 2 | hsps_pick(mb, xb, yb) << 4 | mark);
                const int32_t h = mark ? SWG_HSPS_USED : mh + s;
                H0[i] = h, A0[i] = ma, B0[i] = mb;
                if (h > best || (h == best && h > 0 && (j < bj || (j == bj && i < bi)))) best = h, bj = j, bi = i;
            }
            __syncthreads();
        }

        // best match cell: highest score, then smallest database position, then smallest query position
        atomicMax(&s_best, best);
        __syncthreads();
        const int32_t top = s_best; // the same word for every lane: the stop below is uniform
        if (best == top && best > 0) atomicMin(&s_pos, (unsigned long long)bj << 32 | bi);
        __syncthreads();
        if (top < p.min_score) break;

        char *ops = p.ops + job.ops_off + r * slot_bytes; // alignment r's own slot
        if (tid == 0) {
            SwgTraceOut o = {};
            uint32_t n = 0, same = 0, runs = 0;
            uint32_t j = (uint32_t)(s_pos >> 32), i = (uint32_t)s_pos;
            o.score = top, o.q_end = i, o.d_end = j;
            uint32_t state = 1;
            char later = 0; // the step walked before this one, which follows it in the path
            while (j > 0 && i > 0 && n < lq + len) {
                uint8_t *cell = dir + (size_t)(i + j - 2) * lq + (i - 1);
                const uint32_t c = *cell;
                uint32_t from;
                char op;
                if (state == 1) {
                    *cell = (uint8_t)(c | SWG_HSPS_MARK);
                    same += ident[i - 1] == (uint8_t)d[j - 1];
                    op = 'M', from = c & 3, --j, --i;
                } else if (state == 2) op = 'I', from = (c >> 2) & 3, --j;
                else op = 'D', from = (c >> 4) & 3, --i;
                runs += op != 'M' && op != later;
                ops[n++] = later = op;
                if (from == 0) break;
                state = from;
            }
            o.q_begin = i, o.d_begin = j;
            o.n_ops = n, o.pad[0] = same, o.pad[1] = runs;
            ops[n] = 0;
            out[r] = o;
            s_n = n;
        }
        // the marks and the path were written by one lane to global memory; every lane reads them from here on
        __threadfence();
        __syncthreads();
        const uint32_t n = s_n; // written last to first: turn it round
        for (uint32_t k = tid; k < n / 2; k += SWG_TRACE_THREADS) {
            const char a = ops[k], b = ops[n - 1 - k];
            ops[k] = b, ops[n - 1 - k] = a;
        }
    }
    if (tid == 0) p.n_out[blockIdx.x] = r;
}

#define HSPS_TRY(ctx, expr)                                                                             \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) {                                                                         \
            rc = swg_set_ctx_error(ctx, e_ == hipErrorOutOfMemory ? SWG_ERR_NOMEM : SWG_ERR_HIP,        \
                                   "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            goto done;                                                                                  \
        }                                                                                               \
    } while (0)

// What a call writes to (swg.h): slot s of the hits owns out / counts / ops [s*max_hsps + r] and n_hsps[s].
struct HspsDest {
    uint32_t max_hsps;
    int32_t min_score;
    swg_alignment *out;
    uint32_t *n_hsps;
    swg_align_counts *counts;
    char *ops;
    size_t ops_stride;
};

// Every hit of a checked batch (total > 0 hits), by the traceback's launch plan with max_hsps path slots a job.  Nothing
// is written before a launch has come back, so a refusal of the plan leaves the outputs as they were.
static int hsps_batch(swg_ctx *ctx, const swg_db *db, const SwgTraceBatch &tb, size_t total, const HspsDest &o)
{
    const char *fn = tb.fn;
    SwgTracePlan pl;
    const int prc = swg_trace_plan_batch(ctx, db, tb, total, o.max_hsps, &pl);
    if (prc != SWG_OK) return prc;
    const size_t n = pl.jobs.size(), H = o.max_hsps;
    const size_t positions = (size_t)(tb.q_offsets[tb.n_queries] - tb.q_offsets[0]);
    const size_t q_bytes = positions * (tb.pssm ? 32 : 1);
    std::vector<uint8_t> h_cons; // a PSSM batch's consensus residues (swg.h, swg_align_stats), position by position
    if (tb.pssm) {
        h_cons.resize(positions);
        const int8_t *rows = tb.src + tb.q_offsets[0] * 32;
        for (size_t r = 0; r < positions; ++r) {
            int at = 1;
            for (int b = 2; b < 32; ++b)
                if (rows[r * 32 + b] > rows[r * 32 + at]) at = b;
            h_cons[r] = (uint8_t)at;
        }
    }
    std::vector<SwgTraceOut> h_out(n * H);
    std::vector<uint32_t> h_n(n);
    std::vector<char> h_ops(o.ops ? pl.max_ops : 0);

    int rc = SWG_OK;
    int8_t *d_query = nullptr, *d_sub = nullptr, *d_res = nullptr;
    uint8_t *d_cons = nullptr;
    SwgTraceJob *d_jobs = nullptr;
    int32_t *d_diag = nullptr;
    uint8_t *d_dir = nullptr;
    char *d_ops = nullptr;
    SwgTraceOut *d_out = nullptr;
    uint32_t *d_n = nullptr;
    HSPS_TRY(ctx, hipSetDevice(ctx->device));
    HSPS_TRY(ctx, hipMalloc(&d_query, q_bytes));
    HSPS_TRY(ctx, hipMalloc(&d_sub, 1024));
    HSPS_TRY(ctx, hipMalloc(&d_cons, std::max<size_t>(h_cons.size(), 4)));
    HSPS_TRY(ctx, hipMalloc(&d_res, std::max<size_t>(pl.res.size(), 4)));
    HSPS_TRY(ctx, hipMalloc(&d_jobs, n * sizeof(SwgTraceJob)));
    HSPS_TRY(ctx, hipMalloc(&d_diag, pl.max_diag * sizeof(int32_t)));
    HSPS_TRY(ctx, hipMalloc(&d_dir, pl.max_dir));
    HSPS_TRY(ctx, hipMalloc(&d_ops, pl.max_ops));
    HSPS_TRY(ctx, hipMalloc(&d_out, n * H * sizeof(SwgTraceOut)));
    HSPS_TRY(ctx, hipMalloc(&d_n, n * sizeof(uint32_t)));
    HSPS_TRY(ctx, hipMemcpyAsync(d_query, tb.src + tb.q_offsets[0] * (tb.pssm ? 32 : 1), q_bytes, hipMemcpyHostToDevice, ctx->stream));
    if (!tb.pssm) HSPS_TRY(ctx, hipMemcpyAsync(d_sub, &ctx->sub[0][0], 1024, hipMemcpyHostToDevice, ctx->stream));
    else HSPS_TRY(ctx, hipMemcpyAsync(d_cons, h_cons.data(), h_cons.size(), hipMemcpyHostToDevice, ctx->stream));
    HSPS_TRY(ctx, hipMemcpyAsync(d_res, pl.res.data(), pl.res.size(), hipMemcpyHostToDevice, ctx->stream));
    HSPS_TRY(ctx, hipMemcpyAsync(d_jobs, pl.jobs.data(), n * sizeof(SwgTraceJob), hipMemcpyHostToDevice, ctx->stream));
    for (const SwgTraceLaunch &L : pl.launches) {
        const size_t nb = L.e - L.b;
        SwgHspsParams p;
        p.query = d_query, p.sub = d_sub, p.pssm = d_query, p.res = d_res, p.jobs = d_jobs + L.b, p.diag = d_diag, p.dir = d_dir;
        p.ident = tb.pssm ? d_cons : reinterpret_cast<const uint8_t *>(d_query);
        p.ops = d_ops, p.out = d_out + L.b * H, p.n_out = d_n + L.b;
        p.go = ctx->gap_open + ctx->gap_extend, p.ge = ctx->gap_extend; // src/alignment.c:58-59
        p.max_hsps = o.max_hsps, p.min_score = o.min_score;
        const bool in_lds = L.lq_max <= SWG_TRACE_LDS_COLS;
        const size_t lds = in_lds ? 9 * ((size_t)L.lq_max + 1) * sizeof(int32_t) : 0;
        if (in_lds && !tb.pssm)
            hipLaunchKernelGGL((swg_hsps_kernel<true, false>), dim3((unsigned)nb), dim3(SWG_TRACE_THREADS), lds, ctx->stream, p);
        else if (!tb.pssm)
            hipLaunchKernelGGL((swg_hsps_kernel<false, false>), dim3((unsigned)nb), dim3(SWG_TRACE_THREADS), 0, ctx->stream, p);
        else if (in_lds)
            hipLaunchKernelGGL((swg_hsps_kernel<true, true>), dim3((unsigned)nb), dim3(SWG_TRACE_THREADS), lds, ctx->stream, p);
        else
            hipLaunchKernelGGL((swg_hsps_kernel<false, true>), dim3((unsigned)nb), dim3(SWG_TRACE_THREADS), 0, ctx->stream, p);
        HSPS_TRY(ctx, hipGetLastError());
        HSPS_TRY(ctx, hipMemcpyAsync(h_n.data() + L.b, d_n + L.b, nb * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        HSPS_TRY(ctx, hipMemcpyAsync(h_out.data() + L.b * H, d_out + L.b * H, nb * H * sizeof(SwgTraceOut), hipMemcpyDeviceToHost,
                                     ctx->stream));
        if (o.ops) HSPS_TRY(ctx, hipMemcpyAsync(h_ops.data(), d_ops, L.ops, hipMemcpyDeviceToHost, ctx->stream));
        HSPS_TRY(ctx, hipStreamSynchronize(ctx->stream));
        for (size_t h = L.b; h < L.e; ++h) {
            const size_t slot = pl.dest[h], path_bytes = (size_t)pl.jobs[h].lq + pl.jobs[h].len + 1;
            o.n_hsps[slot] = h_n[h];
            for (size_t r = 0; r < h_n[h]; ++r) {
                const SwgTraceOut &t = h_out[h * H + r];
                swg_alignment &a = o.out[slot * H + r];
                a.score = t.score, a.index = tb.hits[slot].index;
                a.q_begin = t.q_begin, a.q_end = t.q_end, a.d_begin = t.d_begin, a.d_end = t.d_end;
                a.n_ops = t.n_ops, a.reserved = 0;
                if (o.counts) {
                    swg_align_counts &c = o.counts[slot * H + r];
                    c.n_ident = t.pad[0], c.n_gap_open = t.pad[1];
                    c.n_match = (a.q_end - a.q_begin) + (a.d_end - a.d_begin) - a.n_ops; // (every M takes a column and a residue)
                    c.n_gap = a.n_ops - c.n_match;
                }
                if (!o.ops) continue;
                if ((size_t)t.n_ops + 1 > o.ops_stride) {
                    rc = swg_set_ctx_error(ctx, SWG_ERR_ARG, "%s: ops_stride %zu too small for a path of %u steps "
                                           "(swg_align_ops_bound() / swg_align_ops_bound_multi() is always enough)", fn, o.ops_stride, t.n_ops);
                    goto done;
                }
                memcpy(o.ops + (slot * H + r) * o.ops_stride, h_ops.data() + pl.jobs[h].ops_off + r * path_bytes, (size_t)t.n_ops + 1);
            }
        }
    }
done:
    (void)hipFree(d_query), (void)hipFree(d_sub), (void)hipFree(d_cons), (void)hipFree(d_res), (void)hipFree(d_jobs);
    (void)hipFree(d_diag), (void)hipFree(d_dir), (void)hipFree(d_ops), (void)hipFree(d_out), (void)hipFree(d_n);
    return rc;
}

// try/catch: no C++ exception crosses the ABI (the host vectors are sized by the batch)
static int hsps_guarded(swg_ctx *ctx, const swg_db *db, const SwgTraceBatch &tb, size_t total, const HspsDest &o)
{
    try {
        return hsps_batch(ctx, db, tb, total, o);
    } catch (const std::bad_alloc &) {
        return swg_set_ctx_error(ctx, SWG_ERR_NOMEM, "%s: out of host memory", tb.fn);
    } catch (const std::exception &e) {
        return swg_set_ctx_error(ctx, SWG_ERR_NOMEM, "%s: %s", tb.fn, e.what());
    }
}

// The two arguments of their own, refused in front of everything but a NULL context.
static int hsps_check_limits(swg_ctx *ctx, const char *fn, uint32_t max_hsps, int32_t min_score)
{
    if (max_hsps < 1 || max_hsps > SWG_MAX_HSPS)
        return swg_set_ctx_error(ctx, SWG_ERR_ARG, "%s: max_hsps %u outside 1..%d", fn, max_hsps, SWG_MAX_HSPS);
    if (min_score < 1) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "%s: min_score %d below 1", fn, min_score);
    return SWG_OK;
}

extern "C" int swg_align_hsps(swg_ctx *ctx, const swg_db *db, const swg_hit *hits, size_t n_hits, uint32_t max_hsps,
                              int32_t min_score, swg_alignment *out, uint32_t *n_hsps, swg_align_counts *counts, char *ops,
                              size_t ops_stride)
{
    if (!ctx) return swg_set_global_error(SWG_ERR_ARG, "swg_align_hsps: NULL context");
    const int lim = hsps_check_limits(ctx, "swg_align_hsps", max_hsps, min_score);
    if (lim != SWG_OK) return lim;
    if (!db || (n_hits && (!hits || !out || !n_hsps)))
        return swg_set_ctx_error(ctx, SWG_ERR_ARG, "swg_align_hsps: NULL argument");
    if (!ctx->have_scoring || ctx->query_len() == 0)
        return swg_set_ctx_error(ctx, SWG_ERR_STATE, "swg_align_hsps: scoring and query must be set first");
    if (db->device != ctx->device || !db->d_codes)
        return swg_set_ctx_error(ctx, SWG_ERR_STATE, "swg_align_hsps: database is not resident on device %d", ctx->device);
    if (ops && ops_stride == 0) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "swg_align_hsps: ops_stride is 0");
    if (n_hits == 0) return SWG_OK;
    if (n_hits > (1u << 20)) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "swg_align_hsps: more than 2^20 hits");
    const uint64_t q_offsets[2] = {0, ctx->query_len()};
    const SwgTraceBatch tb = {"swg_align_hsps", ctx->query_pssm ? ctx->pssm.data() : ctx->query.data(), ctx->query_pssm,
                              q_offsets, 1, hits, n_hits, &n_hits};
    return hsps_guarded(ctx, db, tb, n_hits, HspsDest{max_hsps, min_score, out, n_hsps, counts, ops, ops_stride});
}

static int hsps_multi(swg_ctx *ctx, const swg_db *db, const SwgTraceBatch &tb, const HspsDest &o)
{
    if (!ctx) return swg_set_global_error(SWG_ERR_ARG, "%s: NULL context", tb.fn);
    const int lim = hsps_check_limits(ctx, tb.fn, o.max_hsps, o.min_score);
    if (lim != SWG_OK) return lim;
    size_t total = 0;
    const int rc = swg_trace_check_batch(ctx, db, tb, o.out, o.ops && o.ops_stride == 0, &total);
    if (rc != SWG_OK || total == 0) return rc;
    if (!o.n_hsps) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "%s: NULL argument", tb.fn);
    return hsps_guarded(ctx, db, tb, total, o);
}

extern "C" int swg_align_hsps_multi(swg_ctx *ctx, const swg_db *db, const int8_t *queries, const uint64_t *q_offsets,
                                    size_t n_queries, const swg_hit *hits, size_t k, const size_t *n_hits, uint32_t max_hsps,
                                    int32_t min_score, swg_alignment *out, uint32_t *n_hsps, swg_align_counts *counts, char *ops,
                                    size_t ops_stride)
{
    const SwgTraceBatch tb = {"swg_align_hsps_multi", queries, false, q_offsets, n_queries, hits, k, n_hits};
    return hsps_multi(ctx, db, tb, HspsDest{max_hsps, min_score, out, n_hsps, counts, ops, ops_stride});
}

extern "C" int swg_align_hsps_multi_pssm(swg_ctx *ctx, const swg_db *db, const int8_t *pssms, const uint64_t *q_offsets,
                                         size_t n_queries, const swg_hit *hits, size_t k, const size_t *n_hits, uint32_t max_hsps,
                                         int32_t min_score, swg_alignment *out, uint32_t *n_hsps, swg_align_counts *counts,
                                         char *ops, size_t ops_stride)
{
    const SwgTraceBatch tb = {"swg_align_hsps_multi_pssm", pssms, true, q_offsets, n_queries, hits, k, n_hits};
    return hsps_multi(ctx, db, tb, HspsDest{max_hsps, min_score, out, n_hsps, counts, ops, ops_stride});
}
