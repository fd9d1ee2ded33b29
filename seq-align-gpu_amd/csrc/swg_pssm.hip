// swg_pssm.hip -- the device half of swg_pssm_build* (include/swg.h "a PSSM from a query's hits"): the paths
// the traceback's kernel leaves on the device become the rows of a query-anchored alignment, the rows are counted,
// weighted (Henikoff) and, with PSI-BLAST's pseudocounts, scored -- so that 32 bytes per query column come back and no
// path crosses PCIe.  The model on the host, which the tests hold this unit against, is swg_pssm_from_paths
// (swg_pssm_host.cpp).  No floating-point atomics and no fused multiply-add; every floating sum has a fixed order.
#include "swg_host_internal.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <new>
#include <stdexcept>
#include <vector>

// One query of a chunk: its rows (row 0 the query itself, row 1 + j its hit j) are rows x lq bytes from msa_off -- 0
// empty, 1..31 a residue, 32 a gap --, its columns are positions pos_off .. pos_off + lq of the chunk's per-column
// arrays, its rows' weights are w[row0 .. row0 + rows).
struct SwgPssmQuery {
    uint64_t msa_off, pos_off, row0;
    uint32_t lq, rows;
};

#define SWG_PSSM_TILE 256       /* columns of a workgroup of the rows', row-0 and count kernels */
#define SWG_PSSM_SCORE_TILE 128 /* of the score kernel: [32][128] doubles of LDS */

__device__ __forceinline__ bool pssm_in_A(uint32_t x, uint32_t mask) { return x >= 1u && x <= 31u && (mask >> x & 1u); }

// Row 0 of every query: its residues.  Grid (column tiles, queries).
__global__ __launch_bounds__(SWG_PSSM_TILE) void swg_pssm_row0_kernel(const SwgPssmQuery *qs, const int8_t *qres, uint8_t *msa)
{
    const SwgPssmQuery q = qs[blockIdx.y];
    const uint32_t p = blockIdx.x * SWG_PSSM_TILE + threadIdx.x;
    if (p < q.lq) msa[q.msa_off + p] = (uint8_t)qres[q.pos_off + p];
}

// One workgroup per job of a traceback launch: the job's path, 256 steps at a time, the (query, database) position carried
// through a block scan of the steps that consume a query column (low half of the word) and a residue (high half); an 'M'
// step stores the residue into its column of the job's row, a 'D' step a gap, 'I' steps nothing.  Every store is guarded
// by the pair's own lengths: a path that were wrong would leave cells empty, never write outside the row.
__global__ __launch_bounds__(256) void swg_pssm_rows_kernel(const SwgTraceJob *jobs, const SwgTraceOut *out, const char *ops, const int8_t *res,
                                                            const uint64_t *row_off, uint8_t *msa)
{
    __shared__ uint32_t wave_tot[4];
    const SwgTraceJob job = jobs[blockIdx.x];
    const SwgTraceOut o = out[blockIdx.x];
    if (o.score <= 0) return; // (the whole workgroup: a hit of score 0 contributes nothing)
    const uint32_t lq = job.lq, len = job.len, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t n = o.n_ops < lq + len ? o.n_ops : lq + len;
    const char *path = ops + job.ops_off;
    const int8_t *d = res + job.res_off;
    uint8_t *row = msa + row_off[blockIdx.x];
    uint32_t cq = o.q_begin, cd = o.d_begin;
    for (uint32_t base = 0; base < n; base += 256u) {
        const uint32_t s = base + tid;
        const char op = s < n ? path[s] : (char)0;
        const uint32_t v = (op == 'M' || op == 'D' ? 1u : 0u) | (op == 'M' || op == 'I' ? 0x10000u : 0u);
        uint32_t incl = v;
#pragma unroll
        for (uint32_t k = 1; k < 64u; k <<= 1) {
            const uint32_t t = __shfl_up(incl, k, 64);
            if (lane >= k) incl += t;
        }
        if (lane == 63u) wave_tot[wave] = incl;
        __syncthreads();
        uint32_t before = 0, tot = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            const uint32_t t = wave_tot[k];
            before += k < wave ? t : 0u;
            tot += t;
        }
        const uint32_t excl = before + incl - v;
        const uint32_t qpos = cq + (excl & 0xFFFFu), dpos = cd + (excl >> 16);
        if (op == 'M') {
            if (qpos < lq && dpos < len) row[qpos] = (uint8_t)d[dpos] & 31u;
        } else if (op == 'D') {
            if (qpos < lq) row[qpos] = 32u;
        }
        cq += tot & 0xFFFFu, cd += tot >> 16;
        __syncthreads(); // (wave_tot is written again in the next round)
    }
}

// Grid (column tiles of 256, queries), one thread per column: it walks the rows in order (a row's bytes of a tile are
// consecutive), counting in its own column of the LDS table [32][256], so no atomics; then n[a][column], k_p and m_p go
// out, and sum k_p, the columns with m_p >= 1 and the columns some hit shows a residue in go to the query's integers
// stat[0..2], one integer atomic per wavefront each.
__global__ __launch_bounds__(SWG_PSSM_TILE) void swg_pssm_count_kernel(const SwgPssmQuery *qs, const uint8_t *msa, uint32_t mask, uint64_t pos_total,
                                                                       uint32_t *n_out, uint32_t *k_out, uint32_t *m_out, uint32_t *stat)
{
    __shared__ uint32_t cnt[32][SWG_PSSM_TILE];
    const SwgPssmQuery q = qs[blockIdx.y];
    if (blockIdx.x * SWG_PSSM_TILE >= q.lq) return;
    const uint32_t tid = threadIdx.x, p = blockIdx.x * SWG_PSSM_TILE + tid;
    const bool active = p < q.lq;
    uint32_t k = 0, m = 0, m_hits = 0;
    if (active) {
        for (uint32_t a = 0; a < 32u; ++a) cnt[a][tid] = 0u;
        const uint8_t *col = msa + q.msa_off + p;
        for (uint32_t r = 0; r < q.rows; ++r) {
            const uint32_t x = col[(uint64_t)r * q.lq];
            if (!pssm_in_A(x, mask)) continue;
            cnt[x][tid] += 1u;
            m_hits += r > 0u ? 1u : 0u;
        }
        const uint64_t pos = q.pos_off + p;
        for (uint32_t a = 1; a < 32u; ++a) {
            const uint32_t c = cnt[a][tid];
            n_out[a * pos_total + pos] = c;
            k += c > 0u ? 1u : 0u, m += c;
        }
        k_out[pos] = k, m_out[pos] = m;
    }
    uint32_t s[3] = {m >= 1u ? k : 0u, m >= 1u ? 1u : 0u, m_hits > 0u ? 1u : 0u};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
#pragma unroll
        for (int dl = 32; dl >= 1; dl >>= 1) s[j] += __shfl_xor(s[j], dl, 64);
    }
    if ((tid & 63u) == 0u)
        for (int j = 0; j < 3; ++j)
            if (s[j]) atomicAdd(&stat[blockIdx.y * 4u + j], s[j]);
}

// One wavefront per row, its lanes over the row's columns (lane, lane + 64, ...: each lane's partial sum in ascending
// order), one butterfly: w_r = sum over the columns where the row shows a residue x of 1 / (k_p n[p][x]).
__global__ __launch_bounds__(256) void swg_pssm_weight_kernel(const SwgPssmQuery *qs, const uint32_t *row_q, uint64_t rows_total, const uint8_t *msa,
                                                              uint32_t mask, uint64_t pos_total, const uint32_t *n_in, const uint32_t *k_in, double *w)
{
#pragma clang fp contract(off)
    const uint64_t row = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (row >= rows_total) return; // (whole wavefronts)
    const uint32_t lane = threadIdx.x & 63u;
    const SwgPssmQuery q = qs[row_q[row]];
    const uint8_t *mr = msa + q.msa_off + (row - q.row0) * q.lq;
    double s = 0.0;
    for (uint32_t p = lane; p < q.lq; p += 64u) {
        const uint32_t x = mr[p];
        if (!pssm_in_A(x, mask)) continue;
        const uint64_t pos = q.pos_off + p;
        s += 1.0 / ((double)k_in[pos] * (double)n_in[x * pos_total + pos]);
    }
#pragma unroll
    for (int dl = 32; dl >= 1; dl >>= 1) s += __shfl_xor(s, dl, 64);
    if (lane == 0u) w[row] = s;
}

struct SwgPssmModel {
    const double *E;   // [32][32] exp(lambda sub[b][a]), b in the query's role
    const double *P;   // [32] the background
    const int8_t *sub; // [32][32]
    double lambda, beta;
    uint32_t mask;
};

// Grid (column tiles of 128, queries), one thread per column: the rows' weights are added in row order into the
// thread's column of the LDS accumulators [a][tid] (LDS, not a dynamically indexed register array: no scratch), then
// f, g, alpha, Q, v and the rounding as include/swg.h states them; clamped entries are counted into stat[3].
__global__ __launch_bounds__(SWG_PSSM_SCORE_TILE) void swg_pssm_score_kernel(const SwgPssmQuery *qs, const uint8_t *msa, const double *w, const uint32_t *m_in,
                                                                             const uint32_t *stat_in, SwgPssmModel md, int8_t *pssm, double *values,
                                                                             uint32_t *stat)
{
#pragma clang fp contract(off)
    __shared__ double acc[32][SWG_PSSM_SCORE_TILE];
    __shared__ double sE[1024];
    __shared__ double sP[32];
    __shared__ int8_t ssub[1024];
    const SwgPssmQuery q = qs[blockIdx.y];
    if (blockIdx.x * SWG_PSSM_SCORE_TILE >= q.lq) return;
    const uint32_t tid = threadIdx.x, p = blockIdx.x * SWG_PSSM_SCORE_TILE + tid, mask = md.mask;
    for (uint32_t i = tid; i < 1024u; i += SWG_PSSM_SCORE_TILE) sE[i] = md.E[i], ssub[i] = md.sub[i];
    if (tid < 32u) sP[tid] = md.P[tid];
    __syncthreads();
    uint32_t clamped = 0;
    if (p < q.lq) {
        for (uint32_t a = 0; a < 32u; ++a) acc[a][tid] = 0.0;
        const uint8_t *col = msa + q.msa_off + p;
        double W = 0.0;
        for (uint32_t r = 0; r < q.rows; ++r) {
            const uint32_t x = col[(uint64_t)r * q.lq];
            if (!pssm_in_A(x, mask)) continue;
            const double wr = w[q.row0 + r];
            acc[x][tid] += wr;
            W += wr;
        }
        const uint64_t pos = q.pos_off + p;
        const uint32_t m = m_in[pos], qr = col[0] & 31u;
        double alpha = 0.0;
        if (m > 0u) {
            const double nbar = (double)stat_in[blockIdx.y * 4u] / (double)stat_in[blockIdx.y * 4u + 1u];
            alpha = fmin(nbar, (double)m) - 1.0;
            for (uint32_t a = 0; a < 32u; ++a) acc[a][tid] = acc[a][tid] / W; // f
        }
        for (uint32_t a = 0; a < 32u; ++a) {
            int8_t sc = a == 0u ? (int8_t)0 : ssub[qr * 32u + a];
            double v = 0.0;
            if (m > 0u && pssm_in_A(a, mask)) {
                double g = 0.0;
                for (uint32_t b = 1; b < 32u; ++b)
                    if (mask >> b & 1u) g += acc[b][tid] * sE[b * 32u + a];
                g *= sP[a];
                const double Q = (alpha * acc[a][tid] + md.beta * g) / (alpha + md.beta);
                v = log(Q / sP[a]) / md.lambda;
                const double r = v < 0.0 ? -floor(-v + 0.5) : floor(v + 0.5); // half away from zero
                if (!(r >= -128.0 && r <= 127.0)) ++clamped;
                sc = (int8_t)(r < -128.0 ? -128.0 : r > 127.0 ? 127.0 : r);
            }
            pssm[pos * 32u + a] = sc;
            if (values) values[pos * 32u + a] = v;
        }
    }
#pragma unroll
    for (int dl = 32; dl >= 1; dl >>= 1) clamped += __shfl_xor(clamped, dl, 64);
    if ((tid & 63u) == 0u && clamped) atomicAdd(&stat[blockIdx.y * 4u + 3u], clamped);
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
#define PSSM_TRY(ctx, expr)                                                                             \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) {                                                                         \
            rc = swg_set_ctx_error(ctx, e_ == hipErrorOutOfMemory ? SWG_ERR_NOMEM : SWG_ERR_HIP,        \
                                   "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            goto done;                                                                                  \
        }                                                                                               \
    } while (0)

// What the traceback's sink needs of the chunk it runs for: where the rows of the chunk's queries lie, and the
// device words its jobs' row offsets go to.
struct PssmSink {
    const std::vector<SwgPssmQuery> *qs;
    size_t k;
    std::vector<uint64_t> h_row_off; // [hits of the chunk], launch after launch
    uint64_t *d_row_off;
    size_t used;
    uint8_t *d_msa;
};

static hipError_t pssm_sink_run(void *user, const SwgTraceLaunchView &v, hipStream_t stream)
{
    PssmSink &s = *(PssmSink *)user;
    if (s.used + v.n_jobs > s.h_row_off.size()) return hipErrorInvalidValue;
    uint64_t *h = s.h_row_off.data() + s.used;
    for (size_t j = 0; j < v.n_jobs; ++j) {
        const size_t i = v.dest[j] / s.k, hit = v.dest[j] % s.k;
        const SwgPssmQuery &q = (*s.qs)[i];
        if (hit + 1 >= q.rows) return hipErrorInvalidValue;
        h[j] = q.msa_off + (uint64_t)(1 + hit) * q.lq;
    }
    uint64_t *d = s.d_row_off + s.used;
    s.used += v.n_jobs;
    const hipError_t e = hipMemcpyAsync(d, h, v.n_jobs * sizeof(uint64_t), hipMemcpyHostToDevice, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(swg_pssm_rows_kernel, dim3((unsigned)v.n_jobs), dim3(256), 0, stream, v.d_jobs, v.d_out, v.d_ops, v.d_res, d, s.d_msa);
    return hipGetLastError();
}

// A chunk: queries [b, e) of the batch and what its device arrays hold.
struct PssmChunk {
    size_t b, e;
    uint64_t msa, pos, rows, hits;
};

#define SWG_PSSM_CHUNK_QUERIES 32768u /* (a grid's second dimension holds 65535) */

// The shared body: tb is the batch as the traceback takes it (index queries, or PSSMs), residues the queries' residues
// by the same offsets.
static int pssm_build_batch(swg_ctx *ctx, const swg_db *db, const SwgTraceBatch &tb, const int8_t *residues, const double *freq,
                            double beta, int8_t *pssms_out, double *values_out, swg_pssm_info *info)
{
    const char *fn = tb.fn;
    size_t total = 0;
    swg_alignment none; // (the check wants to see an output where there are hits; the alignments stay in here)
    int rc = swg_trace_check_batch(ctx, db, tb, &none, false, &total);
    if (rc != SWG_OK) return rc;
    if (tb.n_queries && !residues) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "%s: NULL argument", fn);
    for (uint64_t j = tb.n_queries ? tb.q_offsets[0] : 0; tb.n_queries && j < tb.q_offsets[tb.n_queries]; ++j)
        if (residues[j] < 1 || residues[j] > 31)
            return swg_set_ctx_error(ctx, SWG_ERR_RESIDUE, "%s: residue index %d in a query outside 1..31", fn, residues[j]);
    double P[32], lambda, E[1024];
    uint32_t mask;
    if (swg_pssm_check_model(fn, ctx->sub, freq, beta, P, &mask, &lambda) != SWG_OK)
        return swg_set_ctx_error(ctx, SWG_ERR_ARG, "%s", swg_global_error());
    if (tb.n_queries == 0) return SWG_OK;
    if (!pssms_out) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "%s: pssms_out is NULL", fn);
    for (int b = 0; b < 32; ++b)
        for (int a = 0; a < 32; ++a) E[b * 32 + a] = std::exp(lambda * (double)ctx->sub[b][a]);

    // chunks of queries whose rows stay within the bound (a single query over it goes alone)
    const uint64_t bound = (uint64_t)ctx->opt_pssm_msa_mb << 20;
    std::vector<PssmChunk> chunks;
    PssmChunk big = {0, 0, 1, 1, 1, 1};
    for (size_t i = 0; i < tb.n_queries;) {
        PssmChunk c = {i, i, 0, 0, 0, 0};
        for (; c.e < tb.n_queries && c.e - c.b < SWG_PSSM_CHUNK_QUERIES; ++c.e) {
            const uint64_t lq = tb.q_offsets[c.e + 1] - tb.q_offsets[c.e], rows = 1 + tb.n_hits[c.e];
            if (c.e > c.b && c.msa + rows * lq > bound) break;
            c.msa += rows * lq, c.pos += lq, c.rows += rows, c.hits += tb.n_hits[c.e];
        }
        big.msa = std::max(big.msa, c.msa), big.pos = std::max(big.pos, c.pos), big.rows = std::max(big.rows, c.rows);
        big.hits = std::max(big.hits, c.hits);
        chunks.push_back(c);
        i = c.e;
    }
    if (total > 0) { // every refusal before any launch: what the traceback would refuse by the database, for all chunks
        rc = swg_trace_check_pairs(ctx, db, tb);
        if (rc != SWG_OK) return rc;
    }

    uint8_t *d_msa = nullptr;
    int8_t *d_qres = nullptr, *d_pssm = nullptr, *d_sub = nullptr;
    SwgPssmQuery *d_qs = nullptr;
    uint32_t *d_row_q = nullptr, *d_n = nullptr, *d_k = nullptr, *d_m = nullptr, *d_stat = nullptr;
    uint64_t *d_row_off = nullptr;
    double *d_w = nullptr, *d_values = nullptr, *d_E = nullptr, *d_P = nullptr;
    size_t most_q = 0;
    for (const PssmChunk &c : chunks) most_q = std::max(most_q, c.e - c.b);
    std::vector<SwgPssmQuery> qs;
    std::vector<uint32_t> row_q, stat;
    std::vector<swg_alignment> al;
    PssmSink sink_state = {&qs, std::max<size_t>(tb.k, 1), {}, nullptr, 0, nullptr};
    sink_state.h_row_off.resize(big.hits);
    const SwgTraceSink sink = {&sink_state, pssm_sink_run};
    SwgPssmModel md;
    PSSM_TRY(ctx, hipSetDevice(ctx->device));
    PSSM_TRY(ctx, hipMalloc(&d_msa, big.msa));
    PSSM_TRY(ctx, hipMalloc(&d_qres, big.pos));
    PSSM_TRY(ctx, hipMalloc(&d_pssm, big.pos * 32));
    PSSM_TRY(ctx, hipMalloc(&d_sub, 1024));
    PSSM_TRY(ctx, hipMalloc(&d_qs, most_q * sizeof(SwgPssmQuery)));
    PSSM_TRY(ctx, hipMalloc(&d_row_q, big.rows * sizeof(uint32_t)));
    PSSM_TRY(ctx, hipMalloc(&d_n, big.pos * 32 * sizeof(uint32_t)));
    PSSM_TRY(ctx, hipMalloc(&d_k, big.pos * sizeof(uint32_t)));
    PSSM_TRY(ctx, hipMalloc(&d_m, big.pos * sizeof(uint32_t)));
    PSSM_TRY(ctx, hipMalloc(&d_stat, most_q * 4 * sizeof(uint32_t)));
    PSSM_TRY(ctx, hipMalloc(&d_row_off, big.hits * sizeof(uint64_t)));
    PSSM_TRY(ctx, hipMalloc(&d_w, big.rows * sizeof(double)));
    if (values_out) PSSM_TRY(ctx, hipMalloc(&d_values, big.pos * 32 * sizeof(double)));
    PSSM_TRY(ctx, hipMalloc(&d_E, sizeof E));
    PSSM_TRY(ctx, hipMalloc(&d_P, sizeof P));
    PSSM_TRY(ctx, hipMemcpyAsync(d_sub, &ctx->sub[0][0], 1024, hipMemcpyHostToDevice, ctx->stream));
    PSSM_TRY(ctx, hipMemcpyAsync(d_E, E, sizeof E, hipMemcpyHostToDevice, ctx->stream));
    PSSM_TRY(ctx, hipMemcpyAsync(d_P, P, sizeof P, hipMemcpyHostToDevice, ctx->stream));
    md.E = d_E, md.P = d_P, md.sub = d_sub, md.lambda = lambda, md.beta = beta, md.mask = mask;
    sink_state.d_row_off = d_row_off, sink_state.d_msa = d_msa;

    for (const PssmChunk &c : chunks) {
        const size_t nq = c.e - c.b;
        const uint64_t pos0 = tb.q_offsets[c.b];
        qs.assign(nq, SwgPssmQuery{});
        row_q.assign(c.rows, 0u);
        uint64_t msa = 0, row = 0;
        uint32_t lq_max = 0;
        for (size_t i = 0; i < nq; ++i) {
            SwgPssmQuery &q = qs[i];
            q.lq = (uint32_t)(tb.q_offsets[c.b + i + 1] - tb.q_offsets[c.b + i]), q.rows = (uint32_t)(1 + tb.n_hits[c.b + i]);
            q.msa_off = msa, q.pos_off = tb.q_offsets[c.b + i] - pos0, q.row0 = row;
            for (uint32_t r = 0; r < q.rows; ++r) row_q[row + r] = (uint32_t)i;
            msa += (uint64_t)q.rows * q.lq, row += q.rows;
            lq_max = std::max(lq_max, q.lq);
        }
        PSSM_TRY(ctx, hipMemcpyAsync(d_qs, qs.data(), nq * sizeof(SwgPssmQuery), hipMemcpyHostToDevice, ctx->stream));
        PSSM_TRY(ctx, hipMemcpyAsync(d_row_q, row_q.data(), c.rows * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        PSSM_TRY(ctx, hipMemcpyAsync(d_qres, residues + pos0, c.pos, hipMemcpyHostToDevice, ctx->stream));
        PSSM_TRY(ctx, hipMemsetAsync(d_msa, 0, c.msa, ctx->stream));
        PSSM_TRY(ctx, hipMemsetAsync(d_stat, 0, nq * 4 * sizeof(uint32_t), ctx->stream));
        const dim3 tiles((lq_max + SWG_PSSM_TILE - 1) / SWG_PSSM_TILE, (unsigned)nq);
        hipLaunchKernelGGL(swg_pssm_row0_kernel, tiles, dim3(SWG_PSSM_TILE), 0, ctx->stream, d_qs, d_qres, d_msa);
        PSSM_TRY(ctx, hipGetLastError());
        al.assign(c.hits ? nq * tb.k : 0, swg_alignment{});
        if (c.hits) { // the traceback of the chunk's hits; after every launch the sink turns its paths into rows
            SwgTraceBatch sub_tb = tb;
            sub_tb.q_offsets = tb.q_offsets + c.b, sub_tb.n_queries = nq, sub_tb.hits = tb.hits + c.b * tb.k, sub_tb.n_hits = tb.n_hits + c.b;
            sink_state.used = 0;
            rc = swg_trace_align_batch(ctx, db, sub_tb, c.hits, al.data(), nullptr, 0, &sink);
            if (rc != SWG_OK) goto done;
        }
        hipLaunchKernelGGL(swg_pssm_count_kernel, tiles, dim3(SWG_PSSM_TILE), 0, ctx->stream, d_qs, d_msa, mask, c.pos, d_n, d_k, d_m, d_stat);
        PSSM_TRY(ctx, hipGetLastError());
        hipLaunchKernelGGL(swg_pssm_weight_kernel, dim3((unsigned)((c.rows + 3) / 4)), dim3(256), 0, ctx->stream, d_qs, d_row_q, c.rows, d_msa, mask,
                           c.pos, d_n, d_k, d_w);
        PSSM_TRY(ctx, hipGetLastError());
        hipLaunchKernelGGL(swg_pssm_score_kernel, dim3((lq_max + SWG_PSSM_SCORE_TILE - 1) / SWG_PSSM_SCORE_TILE, (unsigned)nq),
                           dim3(SWG_PSSM_SCORE_TILE), 0, ctx->stream, d_qs, d_msa, d_w, d_m, d_stat, md, d_pssm, d_values, d_stat);
        PSSM_TRY(ctx, hipGetLastError());
        stat.assign(nq * 4, 0u);
        PSSM_TRY(ctx, hipMemcpyAsync(pssms_out + pos0 * 32, d_pssm, c.pos * 32, hipMemcpyDeviceToHost, ctx->stream));
        if (values_out)
            PSSM_TRY(ctx, hipMemcpyAsync(values_out + pos0 * 32, d_values, c.pos * 32 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        PSSM_TRY(ctx, hipMemcpyAsync(stat.data(), d_stat, nq * 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        PSSM_TRY(ctx, hipStreamSynchronize(ctx->stream));
        for (size_t i = 0; i < nq && info; ++i) {
            swg_pssm_info &f = info[c.b + i];
            f.lambda = lambda;
            f.n_distinct = stat[i * 4 + 1] ? (double)stat[i * 4] / (double)stat[i * 4 + 1] : 0.0;
            f.n_rows = 1;
            for (size_t j = 0; j < tb.n_hits[c.b + i]; ++j) f.n_rows += al[i * tb.k + j].score > 0;
            f.n_observed = stat[i * 4 + 2], f.n_clamped = stat[i * 4 + 3], f.reserved = 0;
        }
    }
done:
    (void)hipFree(d_msa), (void)hipFree(d_qres), (void)hipFree(d_pssm), (void)hipFree(d_sub), (void)hipFree(d_qs), (void)hipFree(d_row_q);
    (void)hipFree(d_n), (void)hipFree(d_k), (void)hipFree(d_m), (void)hipFree(d_stat), (void)hipFree(d_row_off), (void)hipFree(d_w);
    (void)hipFree(d_values), (void)hipFree(d_E), (void)hipFree(d_P);
    return rc;
}

static int pssm_build_guarded(swg_ctx *ctx, const swg_db *db, const SwgTraceBatch &tb, const int8_t *residues, const double *freq,
                              double beta, int8_t *pssms_out, double *values_out, swg_pssm_info *info)
{
    try {
        return pssm_build_batch(ctx, db, tb, residues, freq, beta, pssms_out, values_out, info);
    } catch (const std::bad_alloc &) {
        return swg_set_ctx_error(ctx, SWG_ERR_NOMEM, "%s: out of host memory", tb.fn);
    } catch (const std::exception &e) {
        return swg_set_ctx_error(ctx, SWG_ERR_NOMEM, "%s: %s", tb.fn, e.what());
    }
}

extern "C" int swg_pssm_build(swg_ctx *ctx, const swg_db *db, const swg_hit *hits, size_t n_hits, const int8_t *query_residues,
                              const double *freq, double pseudocount, int8_t *pssm_out, double *values_out, swg_pssm_info *info)
{
    const char *fn = "swg_pssm_build";
    if (!ctx) return swg_set_global_error(SWG_ERR_ARG, "%s: NULL context", fn);
    if (!db || (n_hits && !hits)) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "%s: NULL argument", fn);
    if (!ctx->have_scoring || ctx->query_len() == 0)
        return swg_set_ctx_error(ctx, SWG_ERR_STATE, "%s: scoring and query must be set first", fn);
    if (ctx->query_pssm && !query_residues)
        return swg_set_ctx_error(ctx, SWG_ERR_ARG, "%s: the context's query is a PSSM: query_residues (its %zu residues) is required", fn,
                                 ctx->query_len());
    if (!ctx->query_pssm && query_residues)
        return swg_set_ctx_error(ctx, SWG_ERR_ARG, "%s: query_residues must be NULL for an index query", fn);
    const uint64_t q_offsets[2] = {0, ctx->query_len()};
    const SwgTraceBatch tb = {fn, ctx->query_pssm ? ctx->pssm.data() : ctx->query.data(), ctx->query_pssm, q_offsets, 1, hits, n_hits, &n_hits};
    return pssm_build_guarded(ctx, db, tb, ctx->query_pssm ? query_residues : ctx->query.data(), freq, pseudocount, pssm_out, values_out, info);
}

extern "C" int swg_pssm_build_multi(swg_ctx *ctx, const swg_db *db, const int8_t *queries, const uint64_t *q_offsets, size_t n_queries,
                                    const swg_hit *hits, size_t k, const size_t *n_hits, const double *freq, double pseudocount,
                                    int8_t *pssms_out, double *values_out, swg_pssm_info *info)
{
    const SwgTraceBatch tb = {"swg_pssm_build_multi", queries, false, q_offsets, n_queries, hits, k, n_hits};
    return pssm_build_guarded(ctx, db, tb, queries, freq, pseudocount, pssms_out, values_out, info);
}

extern "C" int swg_pssm_build_multi_pssm(swg_ctx *ctx, const swg_db *db, const int8_t *pssms, const int8_t *queries,
                                         const uint64_t *q_offsets, size_t n_queries, const swg_hit *hits, size_t k, const size_t *n_hits,
                                         const double *freq, double pseudocount, int8_t *pssms_out, double *values_out,
                                         swg_pssm_info *info)
{
    const SwgTraceBatch tb = {"swg_pssm_build_multi_pssm", pssms, true, q_offsets, n_queries, hits, k, n_hits};
    return pssm_build_guarded(ctx, db, tb, queries, freq, pseudocount, pssms_out, values_out, info);
}
