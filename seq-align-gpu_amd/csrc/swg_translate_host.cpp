// swg_translate_host.cpp -- the host half of the six-frame translation (include/swg.h; no GPU needed): NCBI's
// codon tables, the host twin of the device kernel (swg_translate_seq, and swg_translate_flat over a whole database), and
// the arithmetic that takes a hit of a translated database back to the nucleotide record.
#include "swg_host_internal.h"
#include "../../include/swg_host.h"

#include <cstring>

namespace {
// NCBI genetic codes as letters in TCAG order (codon 16 b1 + 4 b2 + b3 with T = 0, C = 1, A = 2, G = 3)
struct NcbiCode {
    int id;
    const char *aa;
};
const NcbiCode kCodes[] = {
    {1, "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"},
    {2, "FFLLSSSSYY**CCWWLLLLPPPPHHQQRRRRIIMMTTTTNNKKSS**VVVVAAAADDEEGGGG"},
    {3, "FFLLSSSSYY**CCWWTTTTPPPPHHQQRRRRIIMMTTTTNNKKSSRRVVVVAAAADDEEGGGG"},
    {4, "FFLLSSSSYY**CCWWLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"},
    {5, "FFLLSSSSYY**CCWWLLLLPPPPHHQQRRRRIIMMTTTTNNKKSSSSVVVVAAAADDEEGGGG"},
    {6, "FFLLSSSSYYQQCC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"},
    {11, "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"},
};

// 2-bit code of a residue index, or 4 where it names no base (the three planes of include/swg.h)
inline unsigned nt_code(int8_t idx)
{
    const unsigned i = (unsigned)idx & 31u;
    if ((unsigned)idx > 31u || !((SWG_NT_PLANE_BASE >> i) & 1u)) return 4u;
    return ((SWG_NT_PLANE_LO >> i) & 1u) | (((SWG_NT_PLANE_HI >> i) & 1u) << 1);
}

int check_params(const char *what, const swg_translate_params *p)
{
    for (int c = 0; c < 64; ++c)
        if (p->codon[c] < 1 || p->codon[c] > 31)
            return swg_set_global_error(SWG_ERR_ARG, "%s: codon table entry %d is %d, outside 1..31", what, c, (int)p->codon[c]);
    if (p->unknown < 1 || p->unknown > 31) return swg_set_global_error(SWG_ERR_ARG, "%s: unknown is %d, outside 1..31", what, (int)p->unknown);
    return SWG_OK;
}

// the frames of one sequence, parameters checked
void translate_one(const int8_t *nt, size_t L, const swg_translate_params &p, int8_t *const out[6])
{
    for (size_t f = 0; f < 3; ++f) {
        const size_t n = L >= f + 3 ? (L - f) / 3 : 0;
        for (size_t k = 0; k < n; ++k) {
            const size_t a = f + 3 * k;
            const unsigned b1 = nt_code(nt[a]), b2 = nt_code(nt[a + 1]), b3 = nt_code(nt[a + 2]);
            out[f][k] = ((b1 | b2 | b3) & 4u) ? p.unknown : p.codon[16u * b1 + 4u * b2 + b3];
            // the same offsets of the reverse complement: position r of it is the complement (code ^ 2) of nt[L - 1 - r]
            const unsigned r1 = nt_code(nt[L - 1 - a]), r2 = nt_code(nt[L - 2 - a]), r3 = nt_code(nt[L - 3 - a]);
            out[3 + f][k] = ((r1 | r2 | r3) & 4u) ? p.unknown : p.codon[16u * (r1 ^ 2u) + 4u * (r2 ^ 2u) + (r3 ^ 2u)];
        }
    }
}
} // namespace

extern "C" int swg_codon_table(int ncbi_id, swg_translate_params *out)
{
    if (!out) return swg_set_global_error(SWG_ERR_ARG, "swg_codon_table: NULL argument");
    for (const NcbiCode &c : kCodes)
        if (c.id == ncbi_id) {
            for (int k = 0; k < 64; ++k) out->codon[k] = (int8_t)(c.aa[k] == '*' ? 31 : c.aa[k] - 'A' + 1);
            out->unknown = SWG_TRANSLATE_UNKNOWN_DEFAULT;
            return SWG_OK;
        }
    return swg_set_global_error(SWG_ERR_ARG, "swg_codon_table: genetic code %d is not one of 1, 2, 3, 4, 5, 6, 11", ncbi_id);
}

// p, or code 1 for NULL, checked
int swg_translate_params_get(const char *what, const swg_translate_params *p, swg_translate_params *out)
{
    if (p)
        *out = *p;
    else
        (void)swg_codon_table(1, out);
    return check_params(what, out);
}

extern "C" int swg_translate_seq(const int8_t *nt, size_t nt_len, const swg_translate_params *p, int8_t *out[6], size_t len_out[6])
{
    if (!out || !len_out || (nt_len > 0 && !nt)) return swg_set_global_error(SWG_ERR_ARG, "swg_translate_seq: NULL argument");
    swg_translate_params q;
    const int rc = swg_translate_params_get("swg_translate_seq", p, &q);
    if (rc != SWG_OK) return rc;
    for (size_t g = 0; g < 6; ++g) {
        len_out[g] = nt_len >= g % 3 + 3 ? (nt_len - g % 3) / 3 : 0;
        if (len_out[g] > 0 && !out[g]) return swg_set_global_error(SWG_ERR_ARG, "swg_translate_seq: out[%zu] is NULL", g);
    }
    translate_one(nt, nt_len, q, out);
    return SWG_OK;
}

extern "C" int swg_translate_flat(const int8_t *flat, const uint64_t *offsets, size_t n, const swg_translate_params *p, int8_t *out_flat,
                                  uint64_t *out_offsets)
{
    if (!out_offsets || (n > 0 && (!flat || !offsets || !out_flat))) return swg_set_global_error(SWG_ERR_ARG, "swg_translate_flat: NULL argument");
    swg_translate_params q;
    const int rc = swg_translate_params_get("swg_translate_flat", p, &q);
    if (rc != SWG_OK) return rc;
    out_offsets[0] = 0;
    for (size_t i = 0; i < n; ++i) {
        if (offsets[i + 1] < offsets[i]) return swg_set_global_error(SWG_ERR_ARG, "swg_translate_flat: offsets not monotone at %zu", i);
        const size_t L = (size_t)(offsets[i + 1] - offsets[i]);
        for (size_t g = 0; g < 6; ++g) out_offsets[6 * i + g + 1] = out_offsets[6 * i + g] + (L >= g % 3 + 3 ? (L - g % 3) / 3 : 0);
    }
#pragma omp parallel for schedule(dynamic, 256) num_threads(swg_host_threads())
    for (long long i = 0; i < (long long)n; ++i) {
        int8_t *o[6];
        for (size_t g = 0; g < 6; ++g) o[g] = out_flat + out_offsets[6 * i + g];
        translate_one(flat + offsets[i], (size_t)(offsets[i + 1] - offsets[i]), q, o);
    }
    return SWG_OK;
}

extern "C" void swg_translate_hit(uint32_t index, uint32_t *nt_index, int *frame)
{
    if (nt_index) *nt_index = index / 6u;
    if (frame) *frame = (int)(index % 6u);
}

extern "C" int swg_translate_coords(int frame, uint32_t nt_len, uint32_t d_begin, uint32_t d_end, uint32_t *nt_begin, uint32_t *nt_end)
{
    if (!nt_begin || !nt_end) return swg_set_global_error(SWG_ERR_ARG, "swg_translate_coords: NULL argument");
    if (frame < 0 || frame > 5) return swg_set_global_error(SWG_ERR_ARG, "swg_translate_coords: frame %d outside 0..5", frame);
    const uint32_t f = (uint32_t)frame % 3u, n = swg_frame_len(nt_len, f);
    if (d_begin >= d_end || d_end > n)
        return swg_set_global_error(SWG_ERR_ARG, "swg_translate_coords: residues [%u, %u) of a frame of %u", d_begin, d_end, n);
    if (frame < 3) {
        *nt_begin = f + 3u * d_begin;
        *nt_end = f + 3u * d_end;
    } else {
        *nt_begin = nt_len - f - 3u * d_end;
        *nt_end = nt_len - f - 3u * d_begin;
    }
    return SWG_OK;
}
