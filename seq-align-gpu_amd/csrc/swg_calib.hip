// swg_calib.hip -- the device half of swg_calibrate* and swg_db_composition (include/swg.h): the residue
// counts of a resident database, and per score row of a calibration the histogram and the Gumbel fit, so that 32 bytes
// per query cross PCIe and never a score array.
#include "swg_internal.h"

// ---------------------------------------------------------------------------
// residue counts of a resident database or view
// ---------------------------------------------------------------------------
// A wavefront takes a slot at a time (grid-stride over the slots, so a view walks its own slots over its root's bytes),
// its lanes the sequence's dwords; every byte below the sequence's length is counted in the wavefront's own 32 LDS bins.
// At the end the workgroup's four sets are added up and each populated bin goes to HBM with one atomic.
__global__ __launch_bounds__(256) void swg_db_composition_kernel(const uint32_t *codes, const uint64_t *code_off, const uint32_t *lens,
                                                                 uint32_t n_slots, unsigned long long *counts)
{
    __shared__ unsigned long long bins[4][32];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    if (threadIdx.x < 128u) (&bins[0][0])[threadIdx.x] = 0ull;
    __syncthreads();
    for (uint64_t slot = (uint64_t)blockIdx.x * 4u + wave; slot < n_slots; slot += (uint64_t)gridDim.x * 4u) {
        const uint64_t len = lens[slot], nd = (len + 3u) / 4u;
        const uint32_t *c = codes + code_off[slot];
        for (uint64_t k = lane; k < nd; k += 64u) {
            const uint32_t w = c[k];
#pragma unroll
            for (uint32_t j = 0; j < 4u; ++j)
                if (4u * k + j < len) atomicAdd(&bins[wave][(w >> (8u * j + 3u)) & 31u], 1ull);
        }
    }
    __syncthreads();
    if (threadIdx.x < 32u) {
        const unsigned long long sum = bins[0][threadIdx.x] + bins[1][threadIdx.x] + bins[2][threadIdx.x] + bins[3][threadIdx.x];
        if (sum != 0ull) atomicAdd(&counts[threadIdx.x], sum);
    }
}

hipError_t swg_launch_db_composition(const uint32_t *d_codes, const uint64_t *d_code_off, const uint32_t *d_lens, uint32_t n_slots,
                                     unsigned long long *d_counts, hipStream_t stream)
{
    if (!d_counts) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(d_counts, 0, 32 * sizeof(unsigned long long), stream);
    if (e != hipSuccess || n_slots == 0) return e;
    if (!d_codes || !d_code_off || !d_lens) return hipErrorInvalidValue;
    const uint32_t want = (n_slots + 3u) / 4u;
    hipLaunchKernelGGL(swg_db_composition_kernel, dim3(want > 2048u ? 2048u : want), dim3(256), 0, stream, d_codes, d_code_off, d_lens, n_slots,
                       d_counts);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// histogram and Gumbel fit of a score row
// ---------------------------------------------------------------------------
// Three sums over the workgroup's 256 threads at once, each in a fixed order -- its wavefront's butterfly, then the four
// wavefronts' sums left to right --, the same in every thread: the fit does not depend on which thread ran when.
// Between two calls the second one's writes wait behind the first one's reads (the barrier at its head).
template <class T> __device__ static void calib_block_sum3(T v[3], T (*part)[4])
{
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v[k] += __shfl_xor(v[k], d, 64);
    }
    __syncthreads();
    if ((threadIdx.x & 63u) == 0u)
        for (int k = 0; k < 3; ++k) part[k][threadIdx.x >> 6] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = ((part[k][0] + part[k][1]) + part[k][2]) + part[k][3];
}

// One workgroup per score row (grid (1, rows)): the row's histogram in LDS -- integer atomics, so the counts do not
// depend on their order --, then swg_gumbel_fit_hist (host/swg_evalue.c) on the bins, every thread carrying the same
// lambda through the same Newton steps: thread t sums the bins x0 + t, x0 + t + 256, ... in ascending order.  No fused
// multiply-add: the sums are then the host's up to the order of the additions and the last places of exp.
__global__ __launch_bounds__(256) void swg_calib_fit_kernel(const int32_t *scores, uint64_t row_stride, const uint32_t *order, uint32_t n,
                                                            SwgCalibFit *out)
{
#pragma clang fp contract(off)
    __shared__ uint32_t hist[SWG_CALIB_BINS];
    __shared__ double part[3][4];
    __shared__ long long part_i[3][4];
    __shared__ uint32_t lo_hi[2];
    const uint32_t y = blockIdx.y, t = threadIdx.x;
    const int32_t *row = scores + (uint64_t)y * row_stride;
    for (uint32_t s = t; s < SWG_CALIB_BINS; s += 256u) hist[s] = 0u;
    if (t == 0u) lo_hi[0] = SWG_CALIB_BINS, lo_hi[1] = 0u;
    __syncthreads();
    for (uint32_t base = 0u; base < n; base += 8u * 256u) { // (eight slots per thread and round: their loads are in flight together)
        uint32_t o[8];
        int32_t v[8];
#pragma unroll
        for (uint32_t j = 0; j < 8u; ++j) {
            const uint32_t i = base + j * 256u + t;
            o[j] = i < n ? order[i] : 0xFFFFFFFFu;
            v[j] = i < n ? row[i] : 0;
        }
#pragma unroll
        for (uint32_t j = 0; j < 8u; ++j)
            if (o[j] != 0xFFFFFFFFu) atomicAdd(&hist[v[j] < 0 ? 0u : v[j] >= (int32_t)SWG_CALIB_BINS ? SWG_CALIB_BINS - 1u : (uint32_t)v[j]], 1u);
    }
    __syncthreads();
    // the moments as exact integers, and the populated range
    long long m[3] = {0ll, 0ll, 0ll}; // the count, sum s c_s, sum s^2 c_s (4095^2 x 2^32 < 2^63)
    uint32_t lo = SWG_CALIB_BINS, hi = 0u;
    for (uint32_t s = t; s < SWG_CALIB_BINS; s += 256u) {
        const long long c = hist[s];
        if (c == 0ll) continue;
        m[0] += c, m[1] += c * s, m[2] += c * s * s;
        lo = s < lo ? s : lo, hi = s > hi ? s : hi;
    }
    if (lo < SWG_CALIB_BINS) atomicMin(&lo_hi[0], lo), atomicMax(&lo_hi[1], hi);
    calib_block_sum3(m, part_i); // (its barriers also publish lo_hi)
    const unsigned long long cnt = (unsigned long long)m[0], s1 = (unsigned long long)m[1], s2 = (unsigned long long)m[2];
    const uint32_t x0 = lo_hi[0], x1 = lo_hi[1];
    SwgCalibFit r;
    r.lambda = 0.0, r.mu = 0.0, r.n_iter = 0, r.status = 1, r.n = (uint32_t)cnt, r.reserved = 0u;
    if (cnt != 0ull && x0 != x1) { // (the same in every thread)
        const double nd = (double)cnt, xbar = (double)s1 / nd, var = (double)s2 / nd - xbar * xbar;
        double lam = 3.14159265358979323846 / sqrt(6.0 * var);
        int it = 0;
        r.status = 2;
        while (it < 100) {
            double abd[3] = {0.0, 0.0, 0.0};
            for (uint32_t s = x0 + t; s <= x1; s += 256u) {
                if (hist[s] == 0u) continue;
                const double e = (double)hist[s] * exp(-lam * (double)(s - x0));
                abd[0] += e, abd[1] += (double)s * e, abd[2] += (double)s * (double)s * e;
            }
            calib_block_sum3(abd, part);
            const double A = abd[0], B = abd[1], D = abd[2];
            const double q = B / A;
            const double f = 1.0 / lam - xbar + q;
            const double fp = q * q - D / A - 1.0 / (lam * lam);
            double next = lam - f / fp;
            if (!(next > 0.0)) next = 0.5 * lam;
            const double step = fabs(next - lam);
            ++it;
            const bool done = step <= 1e-12 * lam;
            lam = next;
            if (done) {
                r.status = 0;
                break;
            }
        }
        double last[3] = {0.0, 0.0, 0.0};
        for (uint32_t s = x0 + t; s <= x1; s += 256u)
            if (hist[s] != 0u) last[0] += (double)hist[s] * exp(-lam * (double)(s - x0));
        calib_block_sum3(last, part);
        const double A = last[0];
        r.lambda = lam;
        r.mu = (double)x0 - log(A / nd) / lam;
        r.n_iter = it;
    }
    if (t == 0u) out[y] = r;
}

hipError_t swg_launch_calib_fit(const int32_t *d_scores, uint64_t row_stride, const uint32_t *d_order, uint32_t n_slots, uint32_t n_rows,
                                SwgCalibFit *d_out, hipStream_t stream)
{
    if (n_rows == 0) return hipSuccess;
    if (n_rows > 65535u || !d_scores || !d_order || !d_out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(swg_calib_fit_kernel, dim3(1, n_rows), dim3(256), 0, stream, d_scores, row_stride, d_order, n_slots, d_out);
    return hipGetLastError();
}
