// sanitize_prune_bytes.cpp -- the host code of the byte-wide k-mer tables and the third-level pruning bound: the width
// rule (swg_debug_prune_table_bits), the 256-segment mirror (swg_debug_prune_kmer_refine3), the third choice
// (swg_debug_prune_refine3_choice) and the stage list with its flag (swg_debug_prune_stages3), all in swg_diag_host.cpp,
// as a stand-alone program for AddressSanitizer / UBSan.  No GPU and no libswg.so: the host file is compiled in, and the
// few symbols its planner expects from the kernel file are defined here (the planner is not run).
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -fopenmp -D__HIP_PLATFORM_AMD__ \
//       -I$ROCM_PATH/include tools/sanitize_prune_bytes.cpp seq-align-gpu_amd/csrc/swg_diag_host.cpp -x c \
//       seq-align-gpu_amd/host/swg_threads.c -o sanitize_prune_bytes && ./sanitize_prune_bytes [rounds]
//
// Every round draws a random table, an index query or a PSSM of 1..300 columns whose largest score is at one of the width
// rule's edges, gap scores and a database of sequences of 0..150 residues, and checks: the width is bytes exactly where
// k x the largest colmax entry is at most 255, and then no entry of the 256-segment table is above 255; the bound at 256
// segments is never above the unsegmented one, nor above the 128-segment one where the 256 segments refine the 128; the
// table's row maxima are the unsegmented table; segments without columns hold 0; other segment counts are refused.  The
// third choice answers 0 or 256 for every option value and refuses the others; the stage list with the third level
// tiles the segments like the one without and carries the flag exactly on the stages that carry the list's.
// Exit status 0 = every round agreed.
#include "../seq-align-gpu_amd/csrc/swg_host_internal.h"

#include <cstdio>
#include <cstdlib>
#include <random>

// (the kernel file's geometry tables: not reached from the mirror)
int swg_num_variants(int) { return 0; }
SwgKernelInfo swg_variant_info(int, int) { return SwgKernelInfo(); }
int swg_num_diag_variants() { return 0; }
SwgKernelInfo swg_diag_variant_info(int) { return SwgKernelInfo(); }
size_t swg_diag_dyn_lds_bytes(int, int, int, bool) { return 0; }
size_t swg_diag32q_lds_bytes(int, int, int) { return 0; }
int swg_diag_padded_cols(int K, bool) { return K; }
size_t swg_diag_slice_bytes(int, int, bool) { return 0; }

#define CHECK(c)                                                                \
    do {                                                                        \
        if (!(c)) {                                                             \
            fprintf(stderr, "round %d: %s failed (line %d)\n", round, #c, __LINE__); \
            return 1;                                                           \
        }                                                                       \
    } while (0)

int main(int argc, char **argv)
{
    const int rounds = argc > 1 ? atoi(argv[1]) : 6;
    std::mt19937_64 rng(0x5EED);
    const size_t entries = (size_t)swg_kmer_entries(4);
    const int tops[] = {63, 64, 51, 52, 127, 11};
    for (int round = 0; round < rounds; ++round) {
        const size_t lq = round == 0 ? 1 : round == 1 ? 256 : 1 + rng() % 300;
        const bool pssm = round & 1;
        const int top = tops[round % 6];
        std::vector<int8_t> rows((pssm ? lq : 32) * 32), q(lq);
        for (int8_t &v : rows) v = (int8_t)((int)(rng() % 16) - 6);
        for (int8_t &v : q) v = (int8_t)(1 + rng() % 31);
        // the largest score: once, in a row the query reads, at a residue of its own class or of class 21
        rows[(pssm ? rng() % lq : (size_t)q[rng() % lq]) * 32 + (round & 2 ? 28 : 5)] = (int8_t)top;
        const int8_t *idx = pssm ? nullptr : q.data();
        const int bits4 = swg_debug_prune_table_bits(rows.data(), idx, lq, 4), bits5 = swg_debug_prune_table_bits(rows.data(), idx, lq, 5);
        CHECK(bits4 == (4 * top <= 255 ? 8 : 16) && bits5 == (5 * top <= 255 ? 8 : 16));
        CHECK(swg_debug_prune_table_bits(rows.data(), idx, lq, 3) == SWG_ERR_ARG && swg_debug_prune_table_bits(nullptr, idx, lq, 4) == SWG_ERR_ARG);
        CHECK(swg_debug_prune_table_bits(rows.data(), idx, 0, 4) == SWG_ERR_ARG);
        const int go = -(int)(rng() % 12), ge = -(int)(rng() % 3);
        const size_t n = 1 + rng() % 40;
        std::vector<uint64_t> off(n + 1, 0);
        for (size_t i = 0; i < n; ++i) off[i + 1] = off[i] + rng() % 151;
        std::vector<int8_t> flat(off[n] + 1);
        for (int8_t &v : flat) v = (int8_t)(1 + rng() % 31);
        std::vector<uint16_t> t1(entries), t(entries * 256);
        std::vector<uint64_t> u1(n), u128(n), u(n), u2(n);
        CHECK(swg_debug_prune_kmer(rows.data(), idx, lq, go, ge, 4, flat.data(), off.data(), n, t1.data(), u1.data()) == SWG_OK);
        CHECK(swg_debug_prune_kmer_refine(rows.data(), idx, lq, go, ge, 128, flat.data(), off.data(), n, nullptr, u128.data()) == SWG_OK);
        CHECK(swg_debug_prune_kmer_refine3(rows.data(), idx, lq, go, ge, 256, flat.data(), off.data(), n, t.data(), u.data()) == SWG_OK);
        const size_t W = (lq + 255) / 256, W128 = (lq + 127) / 128;
        for (size_t e = 0; e < entries; ++e) {
            uint16_t m = 0;
            for (size_t s = 0; s < 256; ++s) {
                m = std::max(m, t[e * 256 + s]);
                if (s * W >= lq) CHECK(t[e * 256 + s] == 0);
            }
            CHECK(m == t1[e]);
            if (bits4 == 8) CHECK(m <= 255);
        }
        for (size_t i = 0; i < n; ++i) {
            CHECK(u[i] <= u1[i]);
            if (W128 == 2 * W) CHECK(u[i] <= u128[i]);
        }
        CHECK(swg_debug_prune_kmer_refine3(rows.data(), idx, lq, go, ge, 256, flat.data(), off.data(), n, nullptr, u2.data()) == SWG_OK);
        CHECK(u2 == u);
        for (int S3 : {0, 1, 32, 64, 128, 255, 257, 512, -1})
            CHECK(swg_debug_prune_kmer_refine3(rows.data(), idx, lq, go, ge, S3, flat.data(), off.data(), n, nullptr, u2.data()) == SWG_ERR_ARG);
        // the choice: every option value, either width
        int64_t in[10] = {0, 1, 3000, (int64_t)(rng() % 4000000000ull), 0, 0, 0, 0, 0, 0}, out[4];
        for (int64_t r3 : {0, 1, 256})
            for (int64_t b : {0, 8, 16}) {
                in[8] = r3, in[9] = b;
                CHECK(swg_debug_prune_refine3_choice(in, out) == SWG_OK);
                CHECK(r3 == 256 ? out[3] == 256 : r3 == 1 ? out[3] == 0 : (out[3] == 0 || (out[3] == 256 && out[2] == 128 && b != 16)));
            }
        in[8] = 128;
        CHECK(swg_debug_prune_refine3_choice(in, out) == SWG_ERR_ARG);
        in[8] = 0, in[9] = 32;
        CHECK(swg_debug_prune_refine3_choice(in, out) == SWG_ERR_ARG);
        // the stages of 1..4 segments under a random plan, with and without the third level
        const int64_t n_seg = 1 + (int64_t)(rng() % 4);
        std::vector<int64_t> ask = {(int64_t)(rng() % 12), (int64_t)(rng() & 1), 64 * (int64_t)(rng() % 3), (int64_t)(rng() & 1), n_seg}, ask3;
        for (int64_t i = 0, at = 0; i < n_seg; ++i) {
            const int64_t end = at + 1 + (int64_t)(rng() % 9);
            ask.push_back(at), ask.push_back(end), at = end;
        }
        ask3 = ask;
        ask3.insert(ask3.begin() + 4, 256);
        std::vector<int64_t> st(4 * (2 * (size_t)n_seg + 1)), st3(st.size());
        size_t n_st = 0, n_st3 = 0;
        CHECK(swg_debug_prune_stages(ask.data(), st.data(), st.size() / 4, &n_st) == SWG_OK);
        CHECK(swg_debug_prune_stages3(ask3.data(), st3.data(), st3.size() / 4, &n_st3) == SWG_OK && n_st3 == n_st);
        for (size_t i = 0; i < n_st; ++i) {
            CHECK(st3[4 * i] == st[4 * i] && st3[4 * i + 1] == st[4 * i + 1] && st3[4 * i + 2] == st[4 * i + 2]);
            const int64_t with = st[4 * i + 3] & SWG_STAGE_LIST ? st[4 * i + 3] | SWG_STAGE_REFINE3 : st[4 * i + 3];
            CHECK(st3[4 * i + 3] == with);
        }
        CHECK(swg_debug_prune_stages3(ask3.data(), nullptr, 0, &n_st3) == SWG_OK && n_st3 == n_st);
        ask3[5] = -1;
        CHECK(swg_debug_prune_stages3(ask3.data(), st3.data(), st3.size() / 4, &n_st3) == SWG_ERR_ARG);
    }
    printf("sanitize_prune_bytes: %d rounds agreed\n", rounds);
    return 0;
}
