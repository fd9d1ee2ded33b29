// swg_pssm.hip -- the device half of swg_pssm_build* (include/swg.h "a PSSM from a query's hits"): the paths
// the traceback's kernel leaves on the device become the rows of a query-anchored alignment, the rows are counted,
// weighted (Henikoff) and, with PSI-BLAST's pseudocounts, scored -- so that 32 bytes per query column come back and no
// path crosses PCIe.  The model on the host, which the tests hold this unit against, is swg_pssm_from_paths
// (swg_pssm_host.cpp).  No floating-point atomics and no fused multiply-add; every floating sum has a fixed order.
// Options "pssm_purge" and "pssm_blocks" add the rows' extents, the purge of near-identical rows (a kernel for the pairs,
// one for the greedy order) and per-column blocks (a kernel that lists a query's segments, one workgroup per segment
// that counts, weights and scores): the second half of the device code; their twin is swg_pssm_from_paths_ex.
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

// One column's scores from its accumulators (the thread's column `tid` of acc: the weights of the rows showing a, W their
// total), m_p, the diversity figure nbar of the column's block and the query's residue qr: f, alpha, g, Q, v and the
// rounding as include/swg.h states them, b ascending in g.  Returns the entries that were clamped.  Shared by the score
// kernel (one nbar per query) and the blocks kernel (one per segment).
template <uint32_t TILE>
__device__ __forceinline__ uint32_t pssm_score_column(double (*acc)[TILE], uint32_t tid, double W, uint32_t m, double nbar, uint32_t qr,
                                                      const SwgPssmModel &md, const double *sE, const double *sP, const int8_t *ssub,
                                                      int8_t *pssm_row, double *values_row)
{
#pragma clang fp contract(off)
    const uint32_t mask = md.mask;
    uint32_t clamped = 0;
    double alpha = 0.0;
    if (m > 0u) {
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
        pssm_row[a] = sc;
        if (values_row) values_row[a] = v;
    }
    return clamped;
}

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
        const double nbar = m > 0u ? (double)stat_in[blockIdx.y * 4u] / (double)stat_in[blockIdx.y * 4u + 1u] : 0.0;
        clamped = pssm_score_column<SWG_PSSM_SCORE_TILE>(acc, tid, W, m, nbar, qr, md, sE, sP, ssub, pssm + pos * 32u,
                                                         values ? values + pos * 32u : nullptr);
    }
#pragma unroll
    for (int dl = 32; dl >= 1; dl >>= 1) clamped += __shfl_xor(clamped, dl, 64);
    if ((tid & 63u) == 0u && clamped) atomicAdd(&stat[blockIdx.y * 4u + 3u], clamped);
}

// ---------------------------------------------------------------------------
// options "pssm_purge" and "pssm_blocks": the rows' extents, the purge of near-identical rows, per-column blocks
// ---------------------------------------------------------------------------
#define SWG_PSSM_NEAR_WORD 64u    /* rows s of one word of a row's "near" bits: one wavefront's share of a pair launch */
#define SWG_PSSM_NEAR_WAVES 4u    /* wavefronts of a near workgroup: 256 rows s per round */
#define SWG_PSSM_ROWS_LDS 1024u   /* rows whose weights a blocks workgroup keeps in LDS; the rows beyond take global memory */

// The extent [b, e) of the rows of one traceback launch, one thread per job: the path's [q_begin, q_end), clamped to the
// query as the rows kernel's stores are; empty for a hit of score 0.
__global__ __launch_bounds__(256) void swg_pssm_extent_kernel(const SwgTraceJob *jobs, const SwgTraceOut *out, const uint64_t *row_idx, uint32_t n_jobs,
                                                              uint2 *ext)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n_jobs) return;
    const SwgTraceOut o = out[j];
    const uint32_t lq = jobs[j].lq, e = o.q_end < lq ? o.q_end : lq, b = o.q_begin < e ? o.q_begin : e;
    ext[row_idx[j]] = o.score > 0 ? make_uint2(b, e) : make_uint2(0u, 0u);
}

// Row 0 of every query spans it.
__global__ __launch_bounds__(256) void swg_pssm_extent0_kernel(const SwgPssmQuery *qs, uint32_t n_queries, uint2 *ext)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n_queries) ext[qs[i].row0] = make_uint2(0u, qs[i].lq);
}

// The pairs of the purge.  Grid (rows - 1, queries): workgroup (r - 1, query) compares row r with every row s < r, one
// wavefront per word of 64 rows s (words wave, wave + 4, ...), its lanes over the columns; c(r, s) and i(r, s) are sums
// of ballots' population counts, so integers and the same on every lane.  Bit s of word s / 64 of row r's bits is set if
// the pair is "near": s = 0 (the query) identical in every shared column, s >= 1 with 100 i >= T c; both need c >= 1.
// A query's bits are rows x words uint64 from near_off; the words at and beyond r / 64 + 1 of row r are not written and
// not read.
__global__ __launch_bounds__(256) void swg_pssm_near_kernel(const SwgPssmQuery *qs, const uint64_t *near_off, const uint8_t *msa, uint32_t T,
                                                            unsigned long long *near)
{
    const SwgPssmQuery q = qs[blockIdx.y];
    const uint32_t r = blockIdx.x + 1u;
    if (r >= q.rows) return;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t words = (q.rows + SWG_PSSM_NEAR_WORD - 1u) / SWG_PSSM_NEAR_WORD, nw = (r + SWG_PSSM_NEAR_WORD - 1u) / SWG_PSSM_NEAR_WORD;
    const uint8_t *xr = msa + q.msa_off + (uint64_t)r * q.lq;
    unsigned long long *bits = near + near_off[blockIdx.y] + (uint64_t)r * words;
    for (uint32_t w = wave; w < nw; w += SWG_PSSM_NEAR_WAVES) {
        unsigned long long word = 0;
        const uint32_t s_end = r < (w + 1u) * SWG_PSSM_NEAR_WORD ? r : (w + 1u) * SWG_PSSM_NEAR_WORD;
        for (uint32_t s = w * SWG_PSSM_NEAR_WORD; s < s_end; ++s) {
            const uint8_t *xs = msa + q.msa_off + (uint64_t)s * q.lq;
            uint32_t c = 0, i = 0;
            for (uint32_t base = 0; base < q.lq; base += 64u) {
                const uint32_t p = base + lane;
                const uint32_t x = p < q.lq ? xr[p] : 0u, y = p < q.lq ? xs[p] : 0u;
                const bool both = x >= 1u && x <= 31u && y >= 1u && y <= 31u;
                c += (uint32_t)__popcll(__ballot(both));
                i += (uint32_t)__popcll(__ballot(both && x == y));
            }
            const bool is_near = c >= 1u && (s == 0u ? i == c : (uint64_t)100u * i >= (uint64_t)T * c);
            if (is_near) word |= 1ull << (s & 63u);
        }
        if (lane == 0u) bits[w] = word;
    }
}

// The greedy order of the purge, one wavefront per query: rows r = 1, 2, ... in turn; row r is purged if one of its near
// bits meets a kept row's bit (bit 0, the query, is always kept).  The kept bits are `words` uint64 behind the query's
// near bits; they are written and read with agent-scope accesses, a release between a row's store and the next row's
// loads, so no lane reads a stale word.  A purged row's bytes and extent are zeroed: it is a hit of score 0 from here on.
__global__ __launch_bounds__(64) void swg_pssm_purge_kernel(const SwgPssmQuery *qs, const uint64_t *near_off, unsigned long long *near, uint8_t *msa,
                                                            uint2 *ext, uint32_t *n_purged)
{
    const SwgPssmQuery q = qs[blockIdx.x];
    const uint32_t lane = threadIdx.x, words = (q.rows + SWG_PSSM_NEAR_WORD - 1u) / SWG_PSSM_NEAR_WORD;
    const unsigned long long *bits = near + near_off[blockIdx.x];
    unsigned long long *kept = near + near_off[blockIdx.x] + (uint64_t)q.rows * words;
    for (uint32_t w = lane; w < words; w += 64u) __hip_atomic_store(&kept[w], w == 0u ? 1ull : 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    uint32_t purged = 0;
    for (uint32_t r = 1; r < q.rows; ++r) {
        const uint32_t nw = (r + SWG_PSSM_NEAR_WORD - 1u) / SWG_PSSM_NEAR_WORD;
        bool hit = false;
        for (uint32_t w = lane; w < nw; w += 64u)
            hit = hit || (bits[(uint64_t)r * words + w] & __hip_atomic_load(&kept[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != 0ull;
        if (__ballot(hit) != 0ull) {
            uint8_t *row = msa + q.msa_off + (uint64_t)r * q.lq;
            for (uint32_t p = lane; p < q.lq; p += 64u) row[p] = 0u;
            if (lane == 0u) ext[q.row0 + r] = make_uint2(0u, 0u);
            ++purged;
        } else {
            if (lane == 0u) {
                const unsigned long long k = __hip_atomic_load(&kept[r >> 6], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&kept[r >> 6], k | 1ull << (r & 63u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        }
    }
    if (lane == 0u) n_purged[blockIdx.x] = purged;
}

// The segments of a query, one workgroup per query: the rows' extent boundaries are marked in cut (zeroed by the host),
// then the marked columns are numbered by a block scan, 256 columns a round: segment j begins at seg_start[pos_off + j]
// and ends where segment j + 1 begins (the last at lq).  Column 0 is always marked, by row 0.
__global__ __launch_bounds__(256) void swg_pssm_segments_kernel(const SwgPssmQuery *qs, const uint2 *ext, uint8_t *cut, uint32_t *seg_start,
                                                                uint32_t *n_seg)
{
    __shared__ uint32_t wave_tot[4];
    const SwgPssmQuery q = qs[blockIdx.x];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    for (uint32_t r = tid; r < q.rows; r += 256u) {
        const uint2 e = ext[q.row0 + r];
        if (e.x >= e.y) continue;
        if (e.x < q.lq) cut[q.pos_off + e.x] = 1u;
        if (e.y < q.lq) cut[q.pos_off + e.y] = 1u;
    }
    __syncthreads();
    uint32_t count = 0;
    for (uint32_t base = 0; base < q.lq; base += 256u) {
        const uint32_t p = base + tid;
        const uint32_t v = p < q.lq && cut[q.pos_off + p] ? 1u : 0u;
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
        if (v) seg_start[q.pos_off + count + before + incl - 1u] = p; // (at most one segment per column: within the query's lq words)
        count += tot;
        __syncthreads(); // (wave_tot is written again in the next round)
    }
    if (tid == 0u) n_seg[blockIdx.x] = count;
}

// Per-column blocks.  Grid (segments, queries); a workgroup beyond its query's segments leaves at once.  The columns of
// segment [p0, p1) share R = the rows whose extent contains p0, hence the block [L, U) = [max b_r, min e_r) over R.
//   1. L and U: the threads over the rows, a butterfly and the four wavefronts' results.
//   2. The block's columns in tiles of 256, ascending: one thread per column counts the rows of R in its column of
//      cnt[32][256] (slot 0 then takes k_c); then one wavefront per row of R (rows wave, wave + 4, ...: a row always has
//      the same wavefront) adds the tile's share of the row's weight -- lanes over the tile's columns lane, lane + 64,
//      ..., each lane's partial sum in ascending order, one butterfly, added to the row's weight tile after tile.  The
//      weights of rows below SWG_PSSM_ROWS_LDS are in LDS, the others in the workgroup's own stretch of wg.
//   3. Nbar of the block from the threads' integer sums of k_c.
//   4. The segment's own columns in tiles of 128, one thread per column: the weights of the rows of R in row order into
//      the accumulators (the count table's LDS, used again), then pssm_score_column.
// m_p and Nbar_p go out per column (the host takes info.n_distinct from them), n_observed and n_clamped to stat[2..3].
__global__ __launch_bounds__(256) void swg_pssm_blocks_kernel(const SwgPssmQuery *qs, const uint2 *ext, const uint32_t *seg_start, const uint32_t *n_seg,
                                                              const uint64_t *wg_off, const uint8_t *msa, SwgPssmModel md, double *wg, int8_t *pssm,
                                                              double *values, uint32_t *m_out, double *nbar_out, uint32_t *stat)
{
#pragma clang fp contract(off)
    __shared__ double buf[32 * SWG_PSSM_SCORE_TILE]; // uint32 cnt[32][256], then double acc[32][128]
    __shared__ double sE[1024];
    __shared__ double sP[32];
    __shared__ int8_t ssub[1024];
    __shared__ double wrow[SWG_PSSM_ROWS_LDS];
    __shared__ uint32_t red[2][4];
    static_assert(sizeof(uint32_t) * 32 * SWG_PSSM_TILE == sizeof(double) * 32 * SWG_PSSM_SCORE_TILE, "the count table and the accumulators share LDS");
    const SwgPssmQuery q = qs[blockIdx.y];
    const uint32_t j = blockIdx.x, nseg = n_seg[blockIdx.y];
    if (j >= nseg) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, mask = md.mask;
    const uint32_t p0 = seg_start[q.pos_off + j], p1 = j + 1u < nseg ? seg_start[q.pos_off + j + 1u] : q.lq;
    const uint2 *qext = ext + q.row0;
    const uint8_t *rows = msa + q.msa_off;
    double *wglob = wg + wg_off[blockIdx.y] + (uint64_t)j * (q.rows > SWG_PSSM_ROWS_LDS ? q.rows - SWG_PSSM_ROWS_LDS : 0u);
    for (uint32_t i = tid; i < 1024u; i += 256u) sE[i] = md.E[i], ssub[i] = md.sub[i];
    if (tid < 32u) sP[tid] = md.P[tid];
    // 1. the block
    uint32_t L = 0, U = q.lq;
    for (uint32_t r = tid; r < q.rows; r += 256u) {
        const uint2 e = qext[r];
        if (e.x <= p0 && p0 < e.y) L = e.x > L ? e.x : L, U = e.y < U ? e.y : U;
        if (r < SWG_PSSM_ROWS_LDS) wrow[r] = 0.0;
        else wglob[r - SWG_PSSM_ROWS_LDS] = 0.0;
    }
#pragma unroll
    for (int dl = 32; dl >= 1; dl >>= 1) {
        const uint32_t l2 = __shfl_xor(L, dl, 64), u2 = __shfl_xor(U, dl, 64);
        L = l2 > L ? l2 : L, U = u2 < U ? u2 : U;
    }
    if (lane == 0u) red[0][wave] = L, red[1][wave] = U;
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) L = red[0][k] > L ? red[0][k] : L, U = red[1][k] < U ? red[1][k] : U;
    __syncthreads(); // (red is written again below)
    // 2. counts and weights, tile after tile
    uint32_t(*cnt)[SWG_PSSM_TILE] = (uint32_t(*)[SWG_PSSM_TILE])buf;
    uint32_t sum_k = 0, n_m = 0;
    for (uint32_t c0 = L; c0 < U; c0 += SWG_PSSM_TILE) {
        const uint32_t c = c0 + tid;
        for (uint32_t a = 0; a < 32u; ++a) cnt[a][tid] = 0u;
        if (c < U) {
            for (uint32_t r = 0; r < q.rows; ++r) {
                const uint2 e = qext[r];
                if (!(e.x <= p0 && p0 < e.y)) continue;
                const uint32_t x = rows[(uint64_t)r * q.lq + c];
                if (pssm_in_A(x, mask)) cnt[x][tid] += 1u;
            }
            uint32_t k = 0, m = 0;
            for (uint32_t a = 1; a < 32u; ++a) {
                const uint32_t n = cnt[a][tid];
                k += n > 0u ? 1u : 0u, m += n;
            }
            cnt[0][tid] = k;
            if (m >= 1u) sum_k += k, n_m += 1u;
        }
        __syncthreads();
        const uint32_t width = U - c0 < SWG_PSSM_TILE ? U - c0 : SWG_PSSM_TILE;
        for (uint32_t r = wave; r < q.rows; r += 4u) {
            const uint2 e = qext[r];
            if (!(e.x <= p0 && p0 < e.y)) continue;
            const uint8_t *xr = rows + (uint64_t)r * q.lq + c0;
            double s = 0.0;
            for (uint32_t t = lane; t < width; t += 64u) {
                const uint32_t x = xr[t];
                if (pssm_in_A(x, mask)) s += 1.0 / ((double)cnt[0][t] * (double)cnt[x][t]);
            }
#pragma unroll
            for (int dl = 32; dl >= 1; dl >>= 1) s += __shfl_xor(s, dl, 64);
            if (lane == 0u) {
                if (r < SWG_PSSM_ROWS_LDS) wrow[r] += s;
                else wglob[r - SWG_PSSM_ROWS_LDS] += s;
            }
        }
        __syncthreads();
    }
    // 3. Nbar of the block
#pragma unroll
    for (int dl = 32; dl >= 1; dl >>= 1) sum_k += __shfl_xor(sum_k, dl, 64), n_m += __shfl_xor(n_m, dl, 64);
    if (lane == 0u) red[0][wave] = sum_k, red[1][wave] = n_m;
    __syncthreads();
    sum_k = red[0][0] + red[0][1] + red[0][2] + red[0][3], n_m = red[1][0] + red[1][1] + red[1][2] + red[1][3];
    const double nbar = n_m ? (double)sum_k / (double)n_m : 0.0;
    // 4. the segment's columns
    double(*acc)[SWG_PSSM_SCORE_TILE] = (double(*)[SWG_PSSM_SCORE_TILE])buf;
    uint32_t clamped = 0, observed = 0;
    for (uint32_t t0 = p0; t0 < p1; t0 += SWG_PSSM_SCORE_TILE) {
        const uint32_t p = t0 + tid;
        if (tid >= SWG_PSSM_SCORE_TILE || p >= p1) continue;
        for (uint32_t a = 0; a < 32u; ++a) acc[a][tid] = 0.0;
        double W = 0.0;
        uint32_t m = 0, m_hits = 0;
        for (uint32_t r = 0; r < q.rows; ++r) {
            const uint2 e = qext[r];
            if (!(e.x <= p0 && p0 < e.y)) continue;
            const uint32_t x = rows[(uint64_t)r * q.lq + p];
            if (!pssm_in_A(x, mask)) continue;
            const double wr = r < SWG_PSSM_ROWS_LDS ? wrow[r] : wglob[r - SWG_PSSM_ROWS_LDS];
            acc[x][tid] += wr;
            W += wr;
            m += 1u, m_hits += r > 0u ? 1u : 0u;
        }
        const uint64_t pos = q.pos_off + p;
        m_out[pos] = m, nbar_out[pos] = nbar;
        observed += m_hits > 0u ? 1u : 0u;
        clamped += pssm_score_column<SWG_PSSM_SCORE_TILE>(acc, tid, W, m, nbar, rows[p] & 31u, md, sE, sP, ssub, pssm + pos * 32u,
                                                          values ? values + pos * 32u : nullptr);
    }
#pragma unroll
    for (int dl = 32; dl >= 1; dl >>= 1) clamped += __shfl_xor(clamped, dl, 64), observed += __shfl_xor(observed, dl, 64);
    if (lane == 0u && observed) atomicAdd(&stat[blockIdx.y * 4u + 2u], observed);
    if (lane == 0u && clamped) atomicAdd(&stat[blockIdx.y * 4u + 3u], clamped);
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
    // options "pssm_blocks" / "pssm_purge": the rows' extents are collected as well (d_ext NULL: they are not)
    std::vector<uint64_t> h_row_idx; // [hits of the chunk]: the job's row among the chunk's rows
    uint64_t *d_row_idx;
    uint2 *d_ext;
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
        if (s.d_ext) s.h_row_idx[s.used + j] = q.row0 + 1 + hit;
    }
    uint64_t *d = s.d_row_off + s.used;
    s.used += v.n_jobs;
    const hipError_t e = hipMemcpyAsync(d, h, v.n_jobs * sizeof(uint64_t), hipMemcpyHostToDevice, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(swg_pssm_rows_kernel, dim3((unsigned)v.n_jobs), dim3(256), 0, stream, v.d_jobs, v.d_out, v.d_ops, v.d_res, d, s.d_msa);
    if (s.d_ext) {
        uint64_t *di = s.d_row_idx + (d - s.d_row_off);
        const hipError_t e2 = hipMemcpyAsync(di, s.h_row_idx.data() + (d - s.d_row_off), v.n_jobs * sizeof(uint64_t), hipMemcpyHostToDevice, stream);
        if (e2 != hipSuccess) return e2;
        hipLaunchKernelGGL(swg_pssm_extent_kernel, dim3((unsigned)((v.n_jobs + 255) / 256)), dim3(256), 0, stream, v.d_jobs, v.d_out, di,
                           (uint32_t)v.n_jobs, s.d_ext);
    }
    return hipGetLastError();
}

// A chunk: queries [b, e) of the batch and what its device arrays hold.
struct PssmChunk {
    size_t b, e;
    uint64_t msa, pos, rows, hits;
    uint64_t near, wg; // uint64 words of the purge's bits, doubles of the blocks' weights beyond LDS: both count against the bound
};

// What a query adds to its chunk beyond its rows' bytes: the purge's near and kept bits ((rows + 1) x ceil(rows / 64)
// words), and the blocks kernel's weights in global memory (for the rows beyond SWG_PSSM_ROWS_LDS, one stretch per
// segment; a query has at most min(lq, 2 rows) segments).
static uint64_t pssm_near_words(uint64_t rows) { return (rows + 1) * ((rows + SWG_PSSM_NEAR_WORD - 1) / SWG_PSSM_NEAR_WORD); }
static uint64_t pssm_segments_bound(uint64_t lq, uint64_t rows) { return std::min<uint64_t>(lq, 2 * rows); }
static uint64_t pssm_wg_doubles(uint64_t lq, uint64_t rows)
{
    return rows > SWG_PSSM_ROWS_LDS ? pssm_segments_bound(lq, rows) * (rows - SWG_PSSM_ROWS_LDS) : 0;
}

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
    const bool blocks = ctx->opt_pssm_blocks != 0, purge = ctx->opt_pssm_purge != 0;
    std::vector<PssmChunk> chunks;
    PssmChunk big = {0, 0, 1, 1, 1, 1, 1, 1};
    for (size_t i = 0; i < tb.n_queries;) {
        PssmChunk c = {i, i, 0, 0, 0, 0, 0, 0};
        for (; c.e < tb.n_queries && c.e - c.b < SWG_PSSM_CHUNK_QUERIES; ++c.e) {
            const uint64_t lq = tb.q_offsets[c.e + 1] - tb.q_offsets[c.e], rows = 1 + tb.n_hits[c.e];
            const uint64_t near = purge ? pssm_near_words(rows) : 0, wg = blocks ? pssm_wg_doubles(lq, rows) : 0;
            if (c.e > c.b && c.msa + rows * lq + (c.near + near + c.wg + wg) * 8 > bound) break;
            c.msa += rows * lq, c.pos += lq, c.rows += rows, c.hits += tb.n_hits[c.e], c.near += near, c.wg += wg;
        }
        big.msa = std::max(big.msa, c.msa), big.pos = std::max(big.pos, c.pos), big.rows = std::max(big.rows, c.rows);
        big.hits = std::max(big.hits, c.hits), big.near = std::max(big.near, c.near), big.wg = std::max(big.wg, c.wg);
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
    // options "pssm_blocks" / "pssm_purge"
    uint2 *d_ext = nullptr;
    uint64_t *d_row_idx = nullptr, *d_near_off = nullptr, *d_wg_off = nullptr;
    unsigned long long *d_near = nullptr;
    uint32_t *d_purged = nullptr, *d_seg_start = nullptr, *d_nseg = nullptr;
    uint8_t *d_cut = nullptr;
    double *d_wg = nullptr, *d_nbar = nullptr;
    std::vector<uint64_t> near_off, wg_off;
    std::vector<uint32_t> purged, m_host;
    std::vector<double> nbar_host;
    size_t most_q = 0;
    for (const PssmChunk &c : chunks) most_q = std::max(most_q, c.e - c.b);
    std::vector<SwgPssmQuery> qs;
    std::vector<uint32_t> row_q, stat;
    std::vector<swg_alignment> al;
    PssmSink sink_state = {&qs, std::max<size_t>(tb.k, 1), {}, nullptr, 0, nullptr, {}, nullptr, nullptr};
    sink_state.h_row_off.resize(big.hits);
    if (blocks || purge) sink_state.h_row_idx.resize(big.hits);
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
    if (blocks || purge) {
        PSSM_TRY(ctx, hipMalloc(&d_ext, big.rows * sizeof(uint2)));
        PSSM_TRY(ctx, hipMalloc(&d_row_idx, big.hits * sizeof(uint64_t)));
    }
    if (purge) {
        PSSM_TRY(ctx, hipMalloc(&d_near, big.near * sizeof(unsigned long long)));
        PSSM_TRY(ctx, hipMalloc(&d_near_off, most_q * sizeof(uint64_t)));
        PSSM_TRY(ctx, hipMalloc(&d_purged, most_q * sizeof(uint32_t)));
    }
    if (blocks) {
        PSSM_TRY(ctx, hipMalloc(&d_cut, big.pos));
        PSSM_TRY(ctx, hipMalloc(&d_seg_start, big.pos * sizeof(uint32_t)));
        PSSM_TRY(ctx, hipMalloc(&d_nseg, most_q * sizeof(uint32_t)));
        PSSM_TRY(ctx, hipMalloc(&d_wg_off, most_q * sizeof(uint64_t)));
        PSSM_TRY(ctx, hipMalloc(&d_wg, big.wg * sizeof(double)));
        PSSM_TRY(ctx, hipMalloc(&d_nbar, big.pos * sizeof(double)));
    }
    PSSM_TRY(ctx, hipMemcpyAsync(d_sub, &ctx->sub[0][0], 1024, hipMemcpyHostToDevice, ctx->stream));
    PSSM_TRY(ctx, hipMemcpyAsync(d_E, E, sizeof E, hipMemcpyHostToDevice, ctx->stream));
    PSSM_TRY(ctx, hipMemcpyAsync(d_P, P, sizeof P, hipMemcpyHostToDevice, ctx->stream));
    md.E = d_E, md.P = d_P, md.sub = d_sub, md.lambda = lambda, md.beta = beta, md.mask = mask;
    sink_state.d_row_off = d_row_off, sink_state.d_msa = d_msa, sink_state.d_row_idx = d_row_idx, sink_state.d_ext = d_ext;

    for (const PssmChunk &c : chunks) {
        const size_t nq = c.e - c.b;
        const uint64_t pos0 = tb.q_offsets[c.b];
        qs.assign(nq, SwgPssmQuery{});
        row_q.assign(c.rows, 0u);
        uint64_t msa = 0, row = 0, near = 0, wg = 0;
        uint32_t lq_max = 0, rows_max = 0, seg_max = 0;
        near_off.assign(nq, 0), wg_off.assign(nq, 0);
        for (size_t i = 0; i < nq; ++i) {
            SwgPssmQuery &q = qs[i];
            q.lq = (uint32_t)(tb.q_offsets[c.b + i + 1] - tb.q_offsets[c.b + i]), q.rows = (uint32_t)(1 + tb.n_hits[c.b + i]);
            q.msa_off = msa, q.pos_off = tb.q_offsets[c.b + i] - pos0, q.row0 = row;
            for (uint32_t r = 0; r < q.rows; ++r) row_q[row + r] = (uint32_t)i;
            msa += (uint64_t)q.rows * q.lq, row += q.rows;
            lq_max = std::max(lq_max, q.lq), rows_max = std::max(rows_max, q.rows);
            seg_max = std::max(seg_max, (uint32_t)pssm_segments_bound(q.lq, q.rows));
            near_off[i] = near, wg_off[i] = wg;
            near += purge ? pssm_near_words(q.rows) : 0, wg += blocks ? pssm_wg_doubles(q.lq, q.rows) : 0;
        }
        PSSM_TRY(ctx, hipMemcpyAsync(d_qs, qs.data(), nq * sizeof(SwgPssmQuery), hipMemcpyHostToDevice, ctx->stream));
        PSSM_TRY(ctx, hipMemcpyAsync(d_row_q, row_q.data(), c.rows * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        PSSM_TRY(ctx, hipMemcpyAsync(d_qres, residues + pos0, c.pos, hipMemcpyHostToDevice, ctx->stream));
        PSSM_TRY(ctx, hipMemsetAsync(d_msa, 0, c.msa, ctx->stream));
        PSSM_TRY(ctx, hipMemsetAsync(d_stat, 0, nq * 4 * sizeof(uint32_t), ctx->stream));
        const dim3 tiles((lq_max + SWG_PSSM_TILE - 1) / SWG_PSSM_TILE, (unsigned)nq);
        hipLaunchKernelGGL(swg_pssm_row0_kernel, tiles, dim3(SWG_PSSM_TILE), 0, ctx->stream, d_qs, d_qres, d_msa);
        PSSM_TRY(ctx, hipGetLastError());
        if (d_ext) { // row 0 spans its query; a row the traceback does not reach keeps the empty extent
            PSSM_TRY(ctx, hipMemsetAsync(d_ext, 0, c.rows * sizeof(uint2), ctx->stream));
            hipLaunchKernelGGL(swg_pssm_extent0_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, ctx->stream, d_qs, (uint32_t)nq, d_ext);
            PSSM_TRY(ctx, hipGetLastError());
        }
        al.assign(c.hits ? nq * tb.k : 0, swg_alignment{});
        if (c.hits) { // the traceback of the chunk's hits; after every launch the sink turns its paths into rows
            SwgTraceBatch sub_tb = tb;
            sub_tb.q_offsets = tb.q_offsets + c.b, sub_tb.n_queries = nq, sub_tb.hits = tb.hits + c.b * tb.k, sub_tb.n_hits = tb.n_hits + c.b;
            sink_state.used = 0;
            rc = swg_trace_align_batch(ctx, db, sub_tb, c.hits, al.data(), nullptr, 0, &sink);
            if (rc != SWG_OK) goto done;
        }
        if (purge) { // before everything else: the pairs' near bits, then the greedy order; the purged rows are zeroed
            PSSM_TRY(ctx, hipMemcpyAsync(d_near_off, near_off.data(), nq * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
            if (rows_max > 1) {
                hipLaunchKernelGGL(swg_pssm_near_kernel, dim3(rows_max - 1, (unsigned)nq), dim3(256), 0, ctx->stream, d_qs, d_near_off, d_msa,
                                   (uint32_t)ctx->opt_pssm_purge, d_near);
                PSSM_TRY(ctx, hipGetLastError());
            }
            hipLaunchKernelGGL(swg_pssm_purge_kernel, dim3((unsigned)nq), dim3(64), 0, ctx->stream, d_qs, d_near_off, d_near, d_msa, d_ext, d_purged);
            PSSM_TRY(ctx, hipGetLastError());
        }
        if (blocks) {
            PSSM_TRY(ctx, hipMemcpyAsync(d_wg_off, wg_off.data(), nq * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
            PSSM_TRY(ctx, hipMemsetAsync(d_cut, 0, c.pos, ctx->stream));
            hipLaunchKernelGGL(swg_pssm_segments_kernel, dim3((unsigned)nq), dim3(256), 0, ctx->stream, d_qs, d_ext, d_cut, d_seg_start, d_nseg);
            PSSM_TRY(ctx, hipGetLastError());
            hipLaunchKernelGGL(swg_pssm_blocks_kernel, dim3(seg_max, (unsigned)nq), dim3(256), 0, ctx->stream, d_qs, d_ext, d_seg_start, d_nseg,
                               d_wg_off, d_msa, md, d_wg, d_pssm, d_values, d_m, d_nbar, d_stat);
            PSSM_TRY(ctx, hipGetLastError());
        } else {
            hipLaunchKernelGGL(swg_pssm_count_kernel, tiles, dim3(SWG_PSSM_TILE), 0, ctx->stream, d_qs, d_msa, mask, c.pos, d_n, d_k, d_m, d_stat);
            PSSM_TRY(ctx, hipGetLastError());
            hipLaunchKernelGGL(swg_pssm_weight_kernel, dim3((unsigned)((c.rows + 3) / 4)), dim3(256), 0, ctx->stream, d_qs, d_row_q, c.rows, d_msa,
                               mask, c.pos, d_n, d_k, d_w);
            PSSM_TRY(ctx, hipGetLastError());
            hipLaunchKernelGGL(swg_pssm_score_kernel, dim3((lq_max + SWG_PSSM_SCORE_TILE - 1) / SWG_PSSM_SCORE_TILE, (unsigned)nq),
                               dim3(SWG_PSSM_SCORE_TILE), 0, ctx->stream, d_qs, d_msa, d_w, d_m, d_stat, md, d_pssm, d_values, d_stat);
            PSSM_TRY(ctx, hipGetLastError());
        }
        stat.assign(nq * 4, 0u), purged.assign(nq, 0u);
        if (purge) PSSM_TRY(ctx, hipMemcpyAsync(purged.data(), d_purged, nq * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        if (blocks && info) {
            m_host.resize(c.pos), nbar_host.resize(c.pos);
            PSSM_TRY(ctx, hipMemcpyAsync(m_host.data(), d_m, c.pos * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
            PSSM_TRY(ctx, hipMemcpyAsync(nbar_host.data(), d_nbar, c.pos * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        }
        PSSM_TRY(ctx, hipMemcpyAsync(pssms_out + pos0 * 32, d_pssm, c.pos * 32, hipMemcpyDeviceToHost, ctx->stream));
        if (values_out)
            PSSM_TRY(ctx, hipMemcpyAsync(values_out + pos0 * 32, d_values, c.pos * 32 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        PSSM_TRY(ctx, hipMemcpyAsync(stat.data(), d_stat, nq * 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        PSSM_TRY(ctx, hipStreamSynchronize(ctx->stream));
        for (size_t i = 0; i < nq && info; ++i) {
            swg_pssm_info &f = info[c.b + i];
            f.lambda = lambda;
            f.n_distinct = stat[i * 4 + 1] ? (double)stat[i * 4] / (double)stat[i * 4 + 1] : 0.0;
            if (blocks) { // the mean of Nbar_p over the columns with m_p >= 1, columns ascending
                double sum = 0.0;
                uint64_t n_m = 0;
                for (uint64_t p = qs[i].pos_off; p < qs[i].pos_off + qs[i].lq; ++p)
                    if (m_host[p] >= 1) sum += nbar_host[p], ++n_m;
                f.n_distinct = n_m ? sum / (double)n_m : 0.0;
            }
            f.n_rows = 1;
            for (size_t j = 0; j < tb.n_hits[c.b + i]; ++j) f.n_rows += al[i * tb.k + j].score > 0;
            f.n_rows -= purged[i], f.n_purged = purged[i];
            f.n_observed = stat[i * 4 + 2], f.n_clamped = stat[i * 4 + 3];
        }
    }
done:
    (void)hipFree(d_msa), (void)hipFree(d_qres), (void)hipFree(d_pssm), (void)hipFree(d_sub), (void)hipFree(d_qs), (void)hipFree(d_row_q);
    (void)hipFree(d_n), (void)hipFree(d_k), (void)hipFree(d_m), (void)hipFree(d_stat), (void)hipFree(d_row_off), (void)hipFree(d_w);
    (void)hipFree(d_values), (void)hipFree(d_E), (void)hipFree(d_P);
    (void)hipFree(d_ext), (void)hipFree(d_row_idx), (void)hipFree(d_near), (void)hipFree(d_near_off), (void)hipFree(d_purged), (void)hipFree(d_cut);
    (void)hipFree(d_seg_start), (void)hipFree(d_nseg), (void)hipFree(d_wg_off), (void)hipFree(d_wg), (void)hipFree(d_nbar);
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
