// swg_translate.hip -- swg_db_translate (include/swg.h): the six-frame translation of a resident nucleotide
// database, written on the device.
//
// One streaming kernel, no floating point, no scratch.  A wavefront takes a parent slot at a time (grid-strided in x; the
// tiles of a slot are dealt over the grid's y, so that a database of a few long contigs still fills the chip) and works in
// tiles of SWG_TRANSLATE_TILE_CODONS codons per frame = 64 output dwords per frame, one per lane:
//   stage    the tile's nucleotide bytes come in with coalesced dword loads; every byte becomes its 2-bit code, or 4 where
//            it names no base (the three bit planes of include/swg.h, indexed by byte >> 3), and the four codes of a dword
//            go to the wavefront's LDS tile in one dword store;
//   gather   a lane reads the 14 codes its three frames need (12 nucleotides of four codons, and two more for the frame
//            offsets 1 and 2) as bytes, 12 bytes = 3 dwords apart from lane to lane -- 3 is odd, so the 32 lanes of an LDS
//            lane group fall on 32 banks -- into one word of codes and one of no-base flags;
//   form     frame f's codon k is a 6-bit field of the word of codes: the residue byte comes from the 64-entry table in LDS
//            (a dword per entry: two entries to a bank), `unknown` where the flags say so, 0 past the frame's end (the fill
//            bytes of a sequence's last dword), and the lane stores its whole dword -- consecutive lanes, consecutive dwords.
// The forward pass counts tiles from the sequence's start; the reverse pass counts them from its END (position r of the
// reverse complement is the complement of nucleotide L - 1 - r), reads the tile downwards and complements the word of codes
// with one XOR.  The window of a reverse tile starts on a dword of the parent at or below its lowest nucleotide; what a
// lane reads below nucleotide 0 (only in codons past the frame's end) falls into a pad of no-base codes in front of it.
#include "swg_host_internal.h"

#include <chrono>
#include <exception>

#define SWG_TRANSLATE_TILE_CODONS 256u                              // codons of a frame per tile: a dword of output per lane
#define SWG_TRANSLATE_TILE_NT (3u * SWG_TRANSLATE_TILE_CODONS)      // nucleotides a tile advances by
#define SWG_TRANSLATE_PAD_DWORDS 4u                                 // no-base codes in front of the window (a lane reads 13 below its first)
// the window: 768 + 2 nucleotides and the last lane's two beyond them (it gathers 14), from a dword boundary up to 3 below
#define SWG_TRANSLATE_WINDOW_DWORDS ((SWG_TRANSLATE_TILE_NT + 4u + 3u + 3u) / 4u)
#define SWG_TRANSLATE_LDS_DWORDS (SWG_TRANSLATE_PAD_DWORDS + SWG_TRANSLATE_WINDOW_DWORDS + 2u)

extern "C" unsigned swg_translate_tile_codons(void) { return SWG_TRANSLATE_TILE_CODONS; }

// four residue bytes (index << 3) -> four codes: bits 0..1 the base, bit 2 set where there is none
__device__ static inline uint32_t translate_codes4(uint32_t v)
{
    uint32_t out = 0u;
#pragma unroll
    for (uint32_t j = 0; j < 4u; ++j) {
        const uint32_t i = (v >> (8u * j + 3u)) & 31u;
        const uint32_t c = ((SWG_NT_PLANE_LO >> i) & 1u) | (((SWG_NT_PLANE_HI >> i) & 1u) << 1) | (((~SWG_NT_PLANE_BASE >> i) & 1u) << 2);
        out |= c << (8u * j);
    }
    return out;
}

__global__ __launch_bounds__(256) void swg_translate_kernel(const uint32_t *p_codes, const uint64_t *p_code_off, const uint32_t *p_lens, uint32_t n_pslots,
                                                            const uint32_t *dst, const uint64_t *o_code_off, uint32_t *o_codes,
                                                            const uint32_t *tab, uint32_t unknown_byte, unsigned long long *totals)
{
    __shared__ uint32_t tile[4][SWG_TRANSLATE_LDS_DWORDS];
    __shared__ uint32_t s_tab[64]; // residue byte (index << 3) of codon c
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    if (threadIdx.x < 64u) s_tab[threadIdx.x] = tab[threadIdx.x];
    if (lane < SWG_TRANSLATE_PAD_DWORDS) tile[wave][lane] = 0x04040404u;
    __syncthreads();
    const uint8_t *tb = reinterpret_cast<const uint8_t *>(tile[wave]);
    unsigned long long n_stops = 0ull, n_unknown = 0ull;
    for (uint64_t slot = (uint64_t)blockIdx.x * 4u + wave; slot < n_pslots; slot += (uint64_t)gridDim.x * 4u) {
        const uint32_t L = p_lens[slot];
        if (L < 3u) continue; // no frame has a codon (an empty slot included)
        const uint32_t nd_in = (L + 3u) / 4u;
        const uint32_t *src = p_codes + p_code_off[slot];
        const uint32_t plen[3] = {L / 3u, L >= 4u ? (L - 1u) / 3u : 0u, L >= 5u ? (L - 2u) / 3u : 0u};
        const uint32_t n_tiles = (plen[0] + SWG_TRANSLATE_TILE_CODONS - 1u) / SWG_TRANSLATE_TILE_CODONS;
#pragma unroll
        for (uint32_t rev = 0; rev < 2u; ++rev) {
            uint64_t obase[3];
#pragma unroll
            for (uint32_t f = 0; f < 3u; ++f) obase[f] = plen[f] ? o_code_off[dst[slot * 6u + rev * 3u + f]] : 0ull;
            for (uint32_t t = blockIdx.y; t < n_tiles; t += gridDim.y) {
                // the window's first dword in the parent, and the LDS byte of this lane's first code
                uint32_t a4, p0;
                if (!rev) {
                    a4 = t * (SWG_TRANSLATE_TILE_NT / 4u);
                    p0 = 4u * SWG_TRANSLATE_PAD_DWORDS + 12u * lane;
                } else {
                    const uint32_t hi = L - 1u - t * SWG_TRANSLATE_TILE_NT; // (t < n_tiles: 768 t < 3 plen[0] <= L)
                    const uint32_t lo = hi >= SWG_TRANSLATE_TILE_NT + 3u ? hi - (SWG_TRANSLATE_TILE_NT + 3u) : 0u;
                    a4 = lo >> 2;
                    p0 = 4u * SWG_TRANSLATE_PAD_DWORDS + (hi - 4u * a4) - 12u * lane; // (a lane past the frame's end is not read)
                }
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); // (the last tile's reads are behind us)
                __builtin_amdgcn_wave_barrier();
                for (uint32_t k = lane; k < SWG_TRANSLATE_WINDOW_DWORDS; k += 64u) {
                    const uint32_t g = a4 + k;
                    tile[wave][SWG_TRANSLATE_PAD_DWORDS + k] = translate_codes4(g < nd_in ? src[g] : 0u);
                }
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                __builtin_amdgcn_wave_barrier();
                const uint32_t j = t * 64u + lane; // this lane's dword of every frame
                if (4u * j >= plen[0]) continue;   // (frame 0 is the longest)
                uint32_t w = 0u, m = 0u; // codes first to last from bit 27 down; bit k: no base at position k
#pragma unroll
                for (uint32_t k = 0; k < 14u; ++k) {
                    const uint32_t c = tb[rev ? p0 - k : p0 + k];
                    w = (w << 2) | (c & 3u);
                    m |= (c >> 2) << k;
                }
                if (rev) w ^= 0x0AAAAAAAu; // the complement of code c is c ^ 2 (T <-> A, C <-> G)
#pragma unroll
                for (uint32_t f = 0; f < 3u; ++f) {
                    if (4u * j >= plen[f]) continue;
                    uint32_t v = 0u;
#pragma unroll
                    for (uint32_t k = 0; k < 4u; ++k) {
                        const bool held = 4u * j + k < plen[f];
                        const bool nobase = ((m >> (f + 3u * k)) & 7u) != 0u;
                        const uint32_t known = s_tab[(w >> (2u * (11u - f - 3u * k))) & 63u];
                        const uint32_t b = !held ? 0u : nobase ? unknown_byte : known;
                        n_unknown += held && nobase ? 1ull : 0ull;
                        n_stops += held && !nobase && known == (31u << 3) ? 1ull : 0ull;
                        v |= b << (8u * k);
                    }
                    o_codes[obase[f] + j] = v;
                }
            }
        }
    }
    unsigned long long v[2] = {n_stops, n_unknown};
#pragma unroll
    for (int q = 0; q < 2; ++q) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v[q] += __shfl_xor(v[q], d, 64);
    }
    if (lane == 0u) {
#pragma unroll
        for (int q = 0; q < 2; ++q)
            if (v[q] != 0ull) atomicAdd(&totals[q], v[q]);
    }
}

// ---------------------------------------------------------------------------
// the call
// ---------------------------------------------------------------------------
#define TRANSLATE_TRY(expr)                                                                                                  \
    do {                                                                                                                     \
        hipError_t e_ = (expr);                                                                                              \
        if (e_ != hipSuccess)                                                                                                \
            return swg_set_ctx_error(ctx, e_ == hipErrorOutOfMemory ? SWG_ERR_NOMEM : SWG_ERR_HIP, "swg_db_translate: %s failed: %s", #expr, \
                                     hipGetErrorString(e_));                                                                 \
    } while (0)

static int translate_device(swg_ctx *ctx, const swg_db *parent, const swg_translate_params &p, const std::vector<uint32_t> &dst, swg_db *db,
                            void **tmp, hipEvent_t *ev)
{
    const size_t pns = (size_t)parent->n_bins * SWG_BIN, ns = (size_t)db->n_bins * SWG_BIN, code_bytes = db->codes.size();
    std::vector<uint64_t> off_dw(ns + 1);
    for (size_t i = 0; i <= ns; ++i) off_dw[i] = db->code_off[i] / 4;
    uint32_t tab[64];
    for (int c = 0; c < 64; ++c) tab[c] = (uint32_t)p.codon[c] << 3;
    unsigned long long totals[2] = {0, 0};
    TRANSLATE_TRY(hipSetDevice(ctx->device));
    db->device = ctx->device;
    TRANSLATE_TRY(hipMalloc(&db->d_codes, std::max<size_t>(4, code_bytes)));
    TRANSLATE_TRY(hipMalloc(&db->d_code_off, (ns + 1) * 8));
    TRANSLATE_TRY(hipMalloc(&db->d_lens, std::max<size_t>(4, ns * 4)));
    TRANSLATE_TRY(hipMalloc(&db->d_order, std::max<size_t>(4, ns * 4)));
    TRANSLATE_TRY(hipMalloc(&tmp[0], std::max<size_t>(4, dst.size() * 4)));
    TRANSLATE_TRY(hipMalloc(&tmp[1], sizeof tab + sizeof totals));
    uint32_t *d_dst = static_cast<uint32_t *>(tmp[0]), *d_tab = static_cast<uint32_t *>(tmp[1]);
    unsigned long long *d_totals = reinterpret_cast<unsigned long long *>(d_tab + 64);
    TRANSLATE_TRY(hipEventCreate(&ev[0]));
    TRANSLATE_TRY(hipEventCreate(&ev[1]));
    hipStream_t s = ctx->stream;
    TRANSLATE_TRY(hipMemcpyAsync(db->d_code_off, off_dw.data(), (ns + 1) * 8, hipMemcpyHostToDevice, s));
    if (ns) {
        TRANSLATE_TRY(hipMemcpyAsync(db->d_lens, db->lens.data(), ns * 4, hipMemcpyHostToDevice, s));
        TRANSLATE_TRY(hipMemcpyAsync(db->d_order, db->order.data(), ns * 4, hipMemcpyHostToDevice, s));
    }
    if (!dst.empty()) TRANSLATE_TRY(hipMemcpyAsync(d_dst, dst.data(), dst.size() * 4, hipMemcpyHostToDevice, s));
    TRANSLATE_TRY(hipMemcpyAsync(d_tab, tab, sizeof tab, hipMemcpyHostToDevice, s));
    TRANSLATE_TRY(hipMemsetAsync(d_totals, 0, sizeof totals, s));
    TRANSLATE_TRY(hipEventRecord(ev[0], s));
    if (pns && code_bytes) {
        // x: four slots per workgroup; y: as many shares of a slot's tiles as fill the chip when the slots alone do not
        const uint32_t gx = (uint32_t)std::min<size_t>((pns + 3) / 4, 4096);
        const uint32_t tiles = (parent->lens[0] / 3u + SWG_TRANSLATE_TILE_CODONS - 1u) / SWG_TRANSLATE_TILE_CODONS;
        const uint32_t gy = std::max(1u, std::min(std::min(tiles, 4096u / gx), 1024u));
        hipLaunchKernelGGL(swg_translate_kernel, dim3(gx, gy), dim3(256), 0, s, parent->d_codes, parent->d_code_off, parent->d_lens, (uint32_t)pns,
                           d_dst, db->d_code_off, db->d_codes, d_tab, (uint32_t)p.unknown << 3, d_totals);
        TRANSLATE_TRY(hipGetLastError());
    }
    TRANSLATE_TRY(hipEventRecord(ev[1], s));
    TRANSLATE_TRY(hipMemcpyAsync(totals, d_totals, sizeof totals, hipMemcpyDeviceToHost, s));
    TRANSLATE_TRY(hipStreamSynchronize(s));
    float ms = 0.f;
    TRANSLATE_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
    // the host image: the device's bytes, in one copy
    const auto t0 = std::chrono::steady_clock::now();
    if (code_bytes) TRANSLATE_TRY(hipMemcpy(db->codes.data(), db->d_codes, code_bytes, hipMemcpyDeviceToHost));
    const auto t1 = std::chrono::steady_clock::now();
    db->translated = true;
    db->translate_info.params = p;
    db->translate_info.codons = db->residues;
    db->translate_info.stops = totals[0];
    db->translate_info.unknown_codons = totals[1];
    db->translate_info.kernel_ms = ms;
    db->translate_info.host_image_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    db->upload_bytes = (ns + 1) * 8 + ns * 8 + dst.size() * 4 + sizeof tab; // tables only: no residue crossed PCIe towards the device
    return SWG_OK;
}

extern "C" int swg_db_translate(swg_ctx *ctx, const swg_db *parent, const swg_translate_params *params, swg_db **out)
{
    if (out) *out = nullptr;
    if (!ctx || !parent || !out) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "swg_db_translate: NULL argument");
    if (parent->root)
        return swg_set_ctx_error(ctx, SWG_ERR_ARG, "swg_db_translate: the parent is a view: translate the root and take the view of the result "
                                                   "(frame g of sequence i is sequence 6 i + g)");
    swg_translate_params p;
    const int rp = swg_translate_params_get("swg_db_translate", params, &p);
    if (rp != SWG_OK) return swg_set_ctx_error(ctx, rp, "%s", swg_global_error());
    if ((uint64_t)parent->n_total * 6u >= 0xFFFFFFF0ull)
        return swg_set_ctx_error(ctx, SWG_ERR_ARG, "swg_db_translate: six frames of %zu sequences are too many sequences", parent->n_total);
    if (parent->tokens_only)
        return swg_set_ctx_error(ctx, SWG_ERR_STATE, "swg_db_translate: a database built from 16-lane batches has no residue bytes to translate");
    if (parent->device != ctx->device || !parent->d_codes)
        return swg_set_ctx_error(ctx, SWG_ERR_STATE, "swg_db_translate: the parent is not resident on device %d", ctx->device);
    swg_db *db = nullptr;
    std::vector<uint32_t> dst;
    void *tmp[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    int rc;
    try {
        db = new swg_db();
        swg_translate_slots(parent, db, &dst);
        rc = translate_device(ctx, parent, p, dst, db, tmp, ev);
    } catch (const std::exception &) {
        rc = swg_set_ctx_error(ctx, SWG_ERR_NOMEM, "swg_db_translate: out of host memory");
    }
    if (rc != SWG_OK) (void)hipStreamSynchronize(ctx->stream); // nothing queued may still read what is freed below
    for (void *t : tmp) (void)hipFree(t);
    for (hipEvent_t e : ev)
        if (e) (void)hipEventDestroy(e);
    if (rc != SWG_OK) {
        if (db) swg_db_release_device(db);
        delete db;
        return rc;
    }
    *out = db;
    return SWG_OK;
}

extern "C" int swg_db_translate_info(const swg_db *db, swg_translate_info *out)
{
    if (!db || !out) return swg_set_global_error(SWG_ERR_ARG, "swg_db_translate_info: NULL argument");
    if (!db->translated) return swg_set_global_error(SWG_ERR_STATE, "swg_db_translate_info: not a database that swg_db_translate made");
    *out = db->translate_info;
    return SWG_OK;
}
