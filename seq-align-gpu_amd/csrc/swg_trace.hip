// swg_trace.hip -- alignments of reported hits ("traceback for the top-K only").
//
// The reference prints scores only: its fork removed the traceback of upstream seq-align (Final
// Report p.7, p.10; what is left is the comment at src/alignment.c:46).  A search here returns the K
// best pairs; this unit re-runs exactly those K pairs with the recurrence of src/alignment.c:124-161
// kept whole and walks back from the best match cell.  It is a cold path (K pairs, not the
// database): one workgroup per pair sweeps the anti-diagonals of the pair's matrix, 256 cells at a
// time, in int32, three rotating diagonals per state (in LDS for queries up to 1700 columns, else
// in HBM/L2), one predecessor byte per cell stored diagonal-major (coalesced), then one lane follows
// the bytes back.  A call may hold the hits of a whole batch of queries (swg_align_hits_multi): each
// pair carries its own query.  Everything runs on
// the GPU; like the rest of the library there is no CPU path.
#include "swg_host_internal.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <stdexcept>
#include <cstring>
#include <unordered_map>

// (SwgTraceJob, one pair, and SwgTraceOut, what the kernel leaves for it: swg_host_internal.h)
struct SwgTraceParams {
    const int8_t *query; // table indices of the batch's queries, back to back (PSSM kernel: unread)
    const int8_t *sub;   // [32][32], row = query residue (PSSM kernel: unread)
    const int8_t *pssm;  // PSSM kernel: the batch's PSSM rows [positions][32], row = query position
    const int8_t *res;   // database residue indices of the jobs' sequences
    const SwgTraceJob *jobs;
    int32_t *diag;       // three rotating anti-diagonals of H, A and B per job (kernels without LDS)
    uint8_t *dir;        // predecessor bytes per job, diagonal-major
    char *ops;           // path per job
    SwgTraceOut *out;
    int go, ge;
};

// (SWG_TRACE_THREADS, SWG_TRACE_LDS_COLS: swg_host_internal.h, shared with swg_hsps.hip)

// predecessor code of one state: 0 = the alignment starts here, 1/2/3 = came from H/A/B
__device__ __forceinline__ uint32_t trace_pick(int32_t m, int32_t x, int32_t y)
{
    return m == 0 ? 0u : x == m ? 1u : y == m ? 2u : 3u;
}

// IN_LDS: the nine rotating anti-diagonals live in the workgroup's LDS (queries up to
// SWG_TRACE_LDS_COLS columns; one dependent sweep then waits for LDS, not for L2), sized by the longest query of
// the launch.
// PSSM: a position-specific query; a cell's score is read from row i-1 of the PSSM in global memory (32 * lq bytes,
// more than LDS holds for a long query; a sweep reads consecutive rows, which stay in cache) instead of the table.
template <bool IN_LDS, bool PSSM>
__global__ __launch_bounds__(SWG_TRACE_THREADS) void swg_trace_kernel(SwgTraceParams p)
{
    extern __shared__ int32_t s_diag[];
    __shared__ int8_t s_sub[1024];
    __shared__ int s_best;
    __shared__ unsigned long long s_pos;
    __shared__ uint32_t s_n;
    const SwgTraceJob job = p.jobs[blockIdx.x];
    const uint32_t lq = job.lq, len = job.len, tid = threadIdx.x, w = lq + 1;
    const int8_t *query = PSSM ? nullptr : p.query + job.q_off, *pssm = PSSM ? p.pssm + job.q_off * 32 : nullptr;
    if (!PSSM)
        for (uint32_t k = tid; k < 1024; k += SWG_TRACE_THREADS) s_sub[k] = p.sub[k];
    if (tid == 0) {
        s_best = 0;
        s_pos = ~0ull;
        s_n = 0;
    }
    int32_t *X;
    if (IN_LDS) X = s_diag;
    else X = p.diag + job.diag_off;
    const int8_t *d = p.res + job.res_off;
    uint8_t *dir = p.dir + job.dir_off;
    const int go = p.go, ge = p.ge;
    __syncthreads();

    // cell (j, i): database row j, query column i, both from 1; anti-diagonal dg = i + j.  The
    // buffers are indexed by i: (j-1, i) and (j, i-1) lie on dg-1 at i and i-1, (j-1, i-1) on dg-2 at i-1.
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
            const int32_t s = PSSM ? (int32_t)pssm[(size_t)(i - 1) * 32 + (int)d[j - 1]]
                                   : (int32_t)s_sub[(int)query[i - 1] * 32 + (int)d[j - 1]];
            const int32_t mh = max(max(hd, ad), max(bd, 0));
            const int32_t xa = hu + go, ya = au + ge, za = bu + go;
            const int32_t ma = max(max(xa, ya), max(za, 0));
            const int32_t xb = hl + go, yb = al + go, zb = bl + ge;
            const int32_t mb = max(max(xb, yb), max(zb, 0));
            drow[i - 1] = (uint8_t)(trace_pick(mh, hd, ad) | trace_pick(ma, xa, ya) << 2 | trace_pick(mb, xb, yb) << 4);
            const int32_t h = mh + s;
            H0[i] = h, A0[i] = ma, B0[i] = mb;
            if (h > best || (h == best && h > 0 && (j < bj || (j == bj && i < bi)))) best = h, bj = j, bi = i;
        }
        __syncthreads();
    }

    // best match cell: highest score, then smallest database position, then smallest query position
    atomicMax(&s_best, best);
    __syncthreads();
    if (best == s_best && best > 0) atomicMin(&s_pos, (unsigned long long)bj << 32 | bi);
    __syncthreads();

    char *ops = p.ops + job.ops_off;
    if (tid == 0) {
        SwgTraceOut o = {};
        uint32_t n = 0;
        if (s_best > 0) {
            uint32_t j = (uint32_t)(s_pos >> 32), i = (uint32_t)s_pos;
            o.score = s_best, o.q_end = i, o.d_end = j;
            uint32_t state = 1;
            while (j > 0 && i > 0 && n < lq + len) {
                const uint32_t c = dir[(size_t)(i + j - 2) * lq + (i - 1)];
                uint32_t from;
                if (state == 1) ops[n++] = 'M', from = c & 3, --j, --i;
                else if (state == 2) ops[n++] = 'I', from = (c >> 2) & 3, --j;
                else ops[n++] = 'D', from = (c >> 4) & 3, --i;
                if (from == 0) break;
                state = from;
            }
            o.q_begin = i, o.d_begin = j;
        }
        o.n_ops = n;
        ops[n] = 0;
        p.out[blockIdx.x] = o;
        s_n = n;
    }
    __syncthreads();
    const uint32_t n = s_n; // written last to first: turn it round
    for (uint32_t k = tid; k < n / 2; k += SWG_TRACE_THREADS) {
        const char a = ops[k], b = ops[n - 1 - k];
        ops[k] = b, ops[n - 1 - k] = a;
    }
}

#define TRACE_TRY(ctx, expr)                                                                            \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) {                                                                         \
            rc = swg_set_ctx_error(ctx, e_ == hipErrorOutOfMemory ? SWG_ERR_NOMEM : SWG_ERR_HIP,        \
                                   "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            goto done;                                                                                  \
        }                                                                                               \
    } while (0)

static size_t longest_sequence(const swg_db *db)
{
    uint32_t longest = 0;
    for (uint32_t l : db->lens) longest = std::max(longest, l);
    return longest;
}

extern "C" size_t swg_align_ops_bound(const swg_ctx *ctx, const swg_db *db)
{
    if (!ctx || !db) return 0;
    return ctx->query_len() + longest_sequence(db) + 1;
}

extern "C" size_t swg_align_ops_bound_multi(const swg_db *db, const uint64_t *q_offsets, size_t n_queries)
{
    if (!db || !q_offsets) return 0;
    uint64_t lq_max = 0;
    for (size_t i = 0; i < n_queries; ++i)
        if (q_offsets[i + 1] > q_offsets[i]) lq_max = std::max<uint64_t>(lq_max, q_offsets[i + 1] - q_offsets[i]);
    return (size_t)lq_max + longest_sequence(db) + 1;
}

using TraceBatch = SwgTraceBatch; // (swg_host_internal.h: the bounds calls hand their fallback pairs over as one)

// The launches of a checked batch (total > 0 hits), and its refusals by the database: jobs are ordered by query length and
// cut into launches by class (swg_trace_class) and by the 2 GiB budget of predecessor bytes.  paths: the path slots of lq + len + 1 bytes a
// job owns (1: the traceback's one); paths_in_budget: they count against the launch's bytes as well (swg_align_hsps*).
static int plan_batch(swg_ctx *ctx, const swg_db *db, const TraceBatch &tb, size_t total, uint32_t paths, bool paths_in_budget,
                      SwgTracePlan &pl)
{
    const char *fn = tb.fn;
    // original index -> slot of the sorted order, for the wanted sequences only
    std::unordered_map<uint32_t, size_t> slot_of;
    slot_of.reserve(total * 2);
    for (size_t i = 0; i < tb.n_queries; ++i)
        for (size_t j = 0; j < tb.n_hits[i]; ++j) slot_of[tb.hits[i * tb.k + j].index] = SIZE_MAX;
    for (size_t s = 0; s < db->order.size(); ++s) {
        if (db->order[s] == ~0u) continue;
        auto it = slot_of.find(db->order[s]);
        if (it != slot_of.end()) it->second = s;
    }
    std::vector<SwgTraceJob> in_order;
    std::vector<size_t> dest_in_order; // out[] index of each job
    in_order.reserve(total), dest_in_order.reserve(total);
    std::unordered_map<size_t, uint64_t> res_of; // slot -> its residues in `res` (a sequence is gathered once)
    std::vector<int8_t> &res = pl.res;
    for (size_t i = 0; i < tb.n_queries; ++i) {
        const size_t lq = (size_t)(tb.q_offsets[i + 1] - tb.q_offsets[i]);
        for (size_t j = 0; j < tb.n_hits[i]; ++j) {
            const uint32_t index = tb.hits[i * tb.k + j].index;
            const size_t s = slot_of[index];
            if (s == SIZE_MAX)
                return swg_set_ctx_error(ctx, SWG_ERR_ARG, "%s: sequence %u is not in this database shard", fn, index);
            const size_t len = db->lens[s];
            const uint64_t cells = (uint64_t)(lq + len) * lq;
            if (len == 0 || cells > (16ull << 30))
                return swg_set_ctx_error(ctx, SWG_ERR_ARG, "%s: pair %u (%zu x %zu) is outside what a traceback holds", fn,
                                         index, lq, len);
            const auto r = res_of.emplace(s, (uint64_t)res.size());
            if (r.second) {
                const uint8_t *c = swg_db_codes(db) + db->code_off[s];
                for (size_t x = 0; x < len; ++x) res.push_back((int8_t)(c[x] >> 3)); // codes are index << 3
            }
            SwgTraceJob jb = {};
            jb.q_off = tb.q_offsets[i] - tb.q_offsets[0];
            jb.res_off = r.first->second;
            jb.lq = (uint32_t)lq, jb.len = (uint32_t)len;
            in_order.push_back(jb), dest_in_order.push_back(i * tb.k + j);
        }
    }
    // launch order: by query length (stable), then cut where the class changes or the predecessor bytes would pass
    // 2 GiB (a single larger pair goes alone)
    const size_t n = in_order.size();
    std::vector<size_t> perm(n);
    for (size_t h = 0; h < n; ++h) perm[h] = h;
    std::stable_sort(perm.begin(), perm.end(), [&](size_t a, size_t b) { return in_order[a].lq < in_order[b].lq; });
    std::vector<SwgTraceJob> &jobs = pl.jobs;
    std::vector<size_t> &dest = pl.dest;
    jobs.resize(n), dest.resize(n);
    for (size_t h = 0; h < n; ++h) jobs[h] = in_order[perm[h]], dest[h] = dest_in_order[perm[h]];
    std::vector<SwgTraceLaunch> &launches = pl.launches;
    uint64_t &max_dir = pl.max_dir, &max_diag = pl.max_diag, &max_ops = pl.max_ops;
    for (size_t b = 0; b < n;) {
        const uint64_t budget = 2ull << 30;
        SwgTraceLaunch L = {b, b, 0, 0, 0, 0};
        for (; L.e < n; ++L.e) {
            SwgTraceJob &jb = jobs[L.e];
            const uint64_t path_bytes = ((uint64_t)jb.lq + jb.len + 1) * paths;
            const uint64_t need = (uint64_t)(jb.lq + jb.len - 1) * jb.lq, held = paths_in_budget ? L.ops + path_bytes : 0;
            if (L.e > b && (L.dir + need + held > budget || swg_trace_class(jb.lq) != swg_trace_class(jobs[b].lq))) break;
            jb.dir_off = L.dir, jb.diag_off = L.diag, jb.ops_off = L.ops;
            L.dir += need, L.diag += 9ull * (jb.lq + 1), L.ops += path_bytes;
            L.lq_max = std::max(L.lq_max, jb.lq);
        }
        max_dir = std::max(max_dir, L.dir), max_ops = std::max(max_ops, L.ops);
        if (L.lq_max > SWG_TRACE_LDS_COLS) max_diag = std::max(max_diag, L.diag);
        launches.push_back(L);
        b = L.e;
    }
    return SWG_OK;
}

int swg_trace_plan_batch(swg_ctx *ctx, const swg_db *db, const SwgTraceBatch &tb, size_t total, uint32_t paths, SwgTracePlan *plan)
{
    return plan_batch(ctx, db, tb, total, paths, true, *plan);
}

// Every hit of a checked batch (total > 0 hits): the shared body of all three entry points.  Device buffers are
// allocated once per call; each launch of the plan ends in one stream synchronisation, then its results are copied out.
static int align_batch(swg_ctx *ctx, const swg_db *db, const TraceBatch &tb, size_t total, swg_alignment *out, char *ops,
                       size_t ops_stride, const SwgTraceSink *sink)
{
    const char *fn = tb.fn;
    SwgTracePlan pl;
    const int prc = plan_batch(ctx, db, tb, total, 1, false, pl);
    if (prc != SWG_OK) return prc;
    const std::vector<SwgTraceJob> &jobs = pl.jobs;
    const std::vector<size_t> &dest = pl.dest;
    const std::vector<SwgTraceLaunch> &launches = pl.launches;
    const std::vector<int8_t> &res = pl.res;
    const uint64_t max_dir = pl.max_dir, max_diag = pl.max_diag, max_ops = pl.max_ops;
    const size_t n = jobs.size();
    const size_t row_bytes = tb.pssm ? 32 : 1;
    const size_t q_bytes = (size_t)(tb.q_offsets[tb.n_queries] - tb.q_offsets[0]) * row_bytes;
    std::vector<SwgTraceOut> h_out(n);
    std::vector<char> h_ops(ops ? max_ops : 0);

    int rc = SWG_OK;
    int8_t *d_query = nullptr, *d_sub = nullptr, *d_res = nullptr;
    SwgTraceJob *d_jobs = nullptr;
    int32_t *d_diag = nullptr;
    uint8_t *d_dir = nullptr;
    char *d_ops = nullptr;
    SwgTraceOut *d_out = nullptr;
    TRACE_TRY(ctx, hipSetDevice(ctx->device));
    // the queries' scores: index queries + table, or the PSSM rows (then the table is not read)
    TRACE_TRY(ctx, hipMalloc(&d_query, q_bytes));
    TRACE_TRY(ctx, hipMalloc(&d_sub, 1024));
    TRACE_TRY(ctx, hipMalloc(&d_res, std::max<size_t>(res.size(), 4)));
    TRACE_TRY(ctx, hipMalloc(&d_jobs, n * sizeof(SwgTraceJob)));
    TRACE_TRY(ctx, hipMalloc(&d_diag, max_diag * sizeof(int32_t)));
    TRACE_TRY(ctx, hipMalloc(&d_dir, max_dir));
    TRACE_TRY(ctx, hipMalloc(&d_ops, max_ops));
    TRACE_TRY(ctx, hipMalloc(&d_out, n * sizeof(SwgTraceOut)));
    TRACE_TRY(ctx, hipMemcpyAsync(d_query, tb.src + tb.q_offsets[0] * row_bytes, q_bytes, hipMemcpyHostToDevice, ctx->stream));
    if (!tb.pssm) TRACE_TRY(ctx, hipMemcpyAsync(d_sub, &ctx->sub[0][0], 1024, hipMemcpyHostToDevice, ctx->stream));
    TRACE_TRY(ctx, hipMemcpyAsync(d_res, res.data(), res.size(), hipMemcpyHostToDevice, ctx->stream));
    TRACE_TRY(ctx, hipMemcpyAsync(d_jobs, jobs.data(), n * sizeof(SwgTraceJob), hipMemcpyHostToDevice, ctx->stream));
    for (const SwgTraceLaunch &L : launches) {
        const size_t nb = L.e - L.b;
        SwgTraceParams p;
        p.query = d_query, p.sub = d_sub, p.pssm = d_query, p.res = d_res, p.jobs = d_jobs + L.b, p.diag = d_diag, p.dir = d_dir;
        p.ops = d_ops, p.out = d_out + L.b;
        p.go = ctx->gap_open + ctx->gap_extend, p.ge = ctx->gap_extend; // src/alignment.c:58-59
        const bool in_lds = L.lq_max <= SWG_TRACE_LDS_COLS;
        const size_t lds = in_lds ? 9 * ((size_t)L.lq_max + 1) * sizeof(int32_t) : 0;
        if (in_lds && !tb.pssm)
            hipLaunchKernelGGL((swg_trace_kernel<true, false>), dim3((unsigned)nb), dim3(SWG_TRACE_THREADS), lds, ctx->stream, p);
        else if (!tb.pssm)
            hipLaunchKernelGGL((swg_trace_kernel<false, false>), dim3((unsigned)nb), dim3(SWG_TRACE_THREADS), 0, ctx->stream, p);
        else if (in_lds)
            hipLaunchKernelGGL((swg_trace_kernel<true, true>), dim3((unsigned)nb), dim3(SWG_TRACE_THREADS), lds, ctx->stream, p);
        else
            hipLaunchKernelGGL((swg_trace_kernel<false, true>), dim3((unsigned)nb), dim3(SWG_TRACE_THREADS), 0, ctx->stream, p);
        TRACE_TRY(ctx, hipGetLastError());
        if (sink) { // (the launch's buffers are valid until the synchronisation below)
            const SwgTraceLaunchView v = {d_jobs + L.b, d_out + L.b, d_ops, d_res, dest.data() + L.b, nb};
            TRACE_TRY(ctx, sink->run(sink->user, v, ctx->stream));
        }
        TRACE_TRY(ctx, hipMemcpyAsync(h_out.data() + L.b, d_out + L.b, nb * sizeof(SwgTraceOut), hipMemcpyDeviceToHost,
                                      ctx->stream));
        if (ops) TRACE_TRY(ctx, hipMemcpyAsync(h_ops.data(), d_ops, L.ops, hipMemcpyDeviceToHost, ctx->stream));
        TRACE_TRY(ctx, hipStreamSynchronize(ctx->stream));
        for (size_t h = L.b; h < L.e; ++h) {
            const SwgTraceOut &o = h_out[h];
            swg_alignment &a = out[dest[h]];
            a.score = o.score, a.index = tb.hits[dest[h]].index;
            a.q_begin = o.q_begin, a.q_end = o.q_end, a.d_begin = o.d_begin, a.d_end = o.d_end;
            a.n_ops = o.n_ops, a.reserved = 0;
            if (!ops) continue;
            if ((size_t)o.n_ops + 1 > ops_stride) {
                rc = swg_set_ctx_error(ctx, SWG_ERR_ARG, "%s: ops_stride %zu too small for a path of %u steps "
                                       "(swg_align_ops_bound() / swg_align_ops_bound_multi() is always enough)", fn, ops_stride, o.n_ops);
                goto done;
            }
            memcpy(ops + dest[h] * ops_stride, h_ops.data() + jobs[h].ops_off, (size_t)o.n_ops + 1);
        }
    }
done:
    (void)hipFree(d_query), (void)hipFree(d_sub), (void)hipFree(d_res), (void)hipFree(d_jobs);
    (void)hipFree(d_diag), (void)hipFree(d_dir), (void)hipFree(d_ops), (void)hipFree(d_out);
    return rc;
}

// align_batch's refusals by the database, without the rest of it (same order, same messages)
static int check_pairs(swg_ctx *ctx, const swg_db *db, const TraceBatch &tb)
{
    const char *fn = tb.fn;
    std::unordered_map<uint32_t, size_t> slot_of;
    for (size_t i = 0; i < tb.n_queries; ++i)
        for (size_t j = 0; j < tb.n_hits[i]; ++j) slot_of[tb.hits[i * tb.k + j].index] = SIZE_MAX;
    for (size_t s = 0; s < db->order.size(); ++s) {
        if (db->order[s] == ~0u) continue;
        auto it = slot_of.find(db->order[s]);
        if (it != slot_of.end()) it->second = s;
    }
    for (size_t i = 0; i < tb.n_queries; ++i) {
        const size_t lq = (size_t)(tb.q_offsets[i + 1] - tb.q_offsets[i]);
        for (size_t j = 0; j < tb.n_hits[i]; ++j) {
            const uint32_t index = tb.hits[i * tb.k + j].index;
            const size_t s = slot_of[index];
            if (s == SIZE_MAX)
                return swg_set_ctx_error(ctx, SWG_ERR_ARG, "%s: sequence %u is not in this database shard", fn, index);
            const size_t len = db->lens[s];
            if (len == 0 || (uint64_t)(lq + len) * lq > (16ull << 30))
                return swg_set_ctx_error(ctx, SWG_ERR_ARG, "%s: pair %u (%zu x %zu) is outside what a traceback holds", fn,
                                         index, lq, len);
        }
    }
    return SWG_OK;
}

int swg_trace_check_pairs(swg_ctx *ctx, const swg_db *db, const SwgTraceBatch &tb)
{
    try {
        return check_pairs(ctx, db, tb);
    } catch (const std::exception &) {
        return swg_set_ctx_error(ctx, SWG_ERR_NOMEM, "%s: out of host memory", tb.fn);
    }
}

// try/catch: no C++ exception crosses the ABI (the host vectors are sized by the batch)
int swg_trace_align_batch(swg_ctx *ctx, const swg_db *db, const SwgTraceBatch &tb, size_t total, swg_alignment *out, char *ops,
                          size_t ops_stride, const SwgTraceSink *sink)
{
    try {
        return align_batch(ctx, db, tb, total, out, ops, ops_stride, sink);
    } catch (const std::bad_alloc &) {
        return swg_set_ctx_error(ctx, SWG_ERR_NOMEM, "%s: out of host memory", tb.fn);
    } catch (const std::exception &e) {
        return swg_set_ctx_error(ctx, SWG_ERR_NOMEM, "%s: %s", tb.fn, e.what());
    }
}

extern "C" int swg_align_hits(swg_ctx *ctx, const swg_db *db, const swg_hit *hits, size_t n_hits,
                              swg_alignment *out, char *ops, size_t ops_stride)
{
    if (!ctx) return swg_set_global_error(SWG_ERR_ARG, "swg_align_hits: NULL context");
    if (!db || (n_hits && (!hits || !out)))
        return swg_set_ctx_error(ctx, SWG_ERR_ARG, "swg_align_hits: NULL argument");
    if (!ctx->have_scoring || ctx->query_len() == 0)
        return swg_set_ctx_error(ctx, SWG_ERR_STATE, "swg_align_hits: scoring and query must be set first");
    if (ops && ops_stride == 0) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "swg_align_hits: ops_stride is 0");
    if (n_hits == 0) return SWG_OK;
    if (n_hits > (1u << 20)) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "swg_align_hits: more than 2^20 hits");
    const uint64_t q_offsets[2] = {0, ctx->query_len()};
    const TraceBatch tb = {"swg_align_hits", ctx->query_pssm ? ctx->pssm.data() : ctx->query.data(), ctx->query_pssm,
                           q_offsets, 1, hits, n_hits, &n_hits};
    return swg_trace_align_batch(ctx, db, tb, n_hits, out, ops, ops_stride);
}

// The batch entry points: the queries are checked as search_multi_impl checks them, the rows of hits against k.
int swg_trace_check_batch(swg_ctx *ctx, const swg_db *db, const SwgTraceBatch &tb, const swg_alignment *out, bool stride0,
                          size_t *total_out)
{
    const char *fn = tb.fn;
    *total_out = 0;
    if (!ctx) return swg_set_global_error(SWG_ERR_ARG, "%s: NULL context", fn);
    if (!db || (tb.n_queries && (!tb.src || !tb.q_offsets || !tb.n_hits)))
        return swg_set_ctx_error(ctx, SWG_ERR_ARG, "%s: NULL argument", fn);
    if (!ctx->have_scoring) return swg_set_ctx_error(ctx, SWG_ERR_STATE, "%s: no scoring set", fn);
    if (db->device != ctx->device || !db->d_codes)
        return swg_set_ctx_error(ctx, SWG_ERR_STATE, "%s: database is not resident on device %d", fn, ctx->device);
    if (stride0) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "%s: ops_stride is 0", fn);
    size_t total = 0;
    for (size_t i = 0; i < tb.n_queries; ++i) {
        if (tb.q_offsets[i + 1] <= tb.q_offsets[i])
            return swg_set_ctx_error(ctx, SWG_ERR_ARG, "%s: query %zu is empty or the offsets are not increasing", fn, i);
        if (tb.q_offsets[i + 1] - tb.q_offsets[i] > (1u << 24))
            return swg_set_ctx_error(ctx, SWG_ERR_ARG, "%s: query %zu too long", fn, i);
        for (uint64_t j = tb.q_offsets[i]; j < tb.q_offsets[i + 1] && !tb.pssm; ++j) // (a PSSM takes any int8)
            if (tb.src[j] < 1 || tb.src[j] > 31)
                return swg_set_ctx_error(ctx, SWG_ERR_RESIDUE, "%s: residue index %d in query %zu outside 1..31", fn,
                                         tb.src[j], i);
        if (tb.n_hits[i] > tb.k)
            return swg_set_ctx_error(ctx, SWG_ERR_ARG, "%s: row %zu holds %zu hits, more than k = %zu", fn, i, tb.n_hits[i],
                                     tb.k);
        total += tb.n_hits[i];
    }
    if (total == 0) return SWG_OK;
    if (!tb.hits || !out) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "%s: NULL argument", fn);
    if (total > (1u << 20)) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "%s: more than 2^20 hits", fn);
    *total_out = total;
    return SWG_OK;
}

static int align_hits_multi(swg_ctx *ctx, const swg_db *db, const TraceBatch &tb, swg_alignment *out, char *ops,
                            size_t ops_stride)
{
    size_t total = 0;
    const int rc = swg_trace_check_batch(ctx, db, tb, out, ops && ops_stride == 0, &total);
    if (rc != SWG_OK || total == 0) return rc;
    return swg_trace_align_batch(ctx, db, tb, total, out, ops, ops_stride);
}

extern "C" int swg_align_hits_multi(swg_ctx *ctx, const swg_db *db, const int8_t *queries, const uint64_t *q_offsets,
                                    size_t n_queries, const swg_hit *hits, size_t k, const size_t *n_hits,
                                    swg_alignment *out, char *ops, size_t ops_stride)
{
    const TraceBatch tb = {"swg_align_hits_multi", queries, false, q_offsets, n_queries, hits, k, n_hits};
    return align_hits_multi(ctx, db, tb, out, ops, ops_stride);
}

extern "C" int swg_align_hits_multi_pssm(swg_ctx *ctx, const swg_db *db, const int8_t *pssms, const uint64_t *q_offsets,
                                         size_t n_queries, const swg_hit *hits, size_t k, const size_t *n_hits,
                                         swg_alignment *out, char *ops, size_t ops_stride)
{
    const TraceBatch tb = {"swg_align_hits_multi_pssm", pssms, true, q_offsets, n_queries, hits, k, n_hits};
    return align_hits_multi(ctx, db, tb, out, ops, ops_stride);
}
