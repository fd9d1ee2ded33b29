// sanitize_prune_refine.cpp -- the host mirror of the second-level pruning bound (swg_debug_prune_kmer_refine) and its
// choice (swg_debug_prune_refine_choice, swg_diag_host.cpp), as a stand-alone program for AddressSanitizer / UBSan.  No
// GPU and no libswg.so: the host file is compiled in, and the few symbols its planner expects from the kernel file are
// defined here (the planner is not run).
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -fopenmp -D__HIP_PLATFORM_AMD__ \
//       -I$ROCM_PATH/include tools/sanitize_prune_refine.cpp seq-align-gpu_amd/csrc/swg_diag_host.cpp -x c \
//       seq-align-gpu_amd/host/swg_threads.c -o sanitize_prune_refine && ./sanitize_prune_refine [rounds]
//
// Every round draws a random table, an index query or a PSSM of 1..160 columns (fewer columns than segments among them),
// gap scores and a database of sequences of 0..150 residues, and checks: the bound at 32, 64 and 128 segments is never
// above the unsegmented one; the table's row maxima are the unsegmented table; segments without columns hold 0; other
// segment counts are refused.  The stage list (swg_debug_prune_stages) is drawn too: its stages tile the segments in
// order, and a caller's room for fewer stages than there are is respected.  Exit status 0 = every round agreed.
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
    for (int round = 0; round < rounds; ++round) {
        const size_t lq = round == 0 ? 1 : 1 + rng() % 160;
        const bool pssm = round & 1;
        std::vector<int8_t> rows((pssm ? lq : 32) * 32), q(lq);
        for (int8_t &v : rows) v = (int8_t)((int)(rng() % 16) - 6);
        for (int8_t &v : q) v = (int8_t)(1 + rng() % 31);
        const int go = -(int)(rng() % 12), ge = -(int)(rng() % 3);
        const size_t n = 1 + rng() % 40;
        std::vector<uint64_t> off(n + 1, 0);
        for (size_t i = 0; i < n; ++i) off[i + 1] = off[i] + rng() % 151;
        std::vector<int8_t> flat(off[n] + 1);
        for (int8_t &v : flat) v = (int8_t)(1 + rng() % 31);
        const int8_t *idx = pssm ? nullptr : q.data();
        std::vector<uint16_t> t1(entries);
        std::vector<uint64_t> u1(n), u(n);
        CHECK(swg_debug_prune_kmer(rows.data(), idx, lq, go, ge, 4, flat.data(), off.data(), n, t1.data(), u1.data()) == SWG_OK);
        for (int S2 : {32, 64, 128}) {
            std::vector<uint16_t> t(entries * (size_t)S2);
            CHECK(swg_debug_prune_kmer_refine(rows.data(), idx, lq, go, ge, S2, flat.data(), off.data(), n, t.data(), u.data()) == SWG_OK);
            const size_t W = (lq + (size_t)S2 - 1) / (size_t)S2;
            for (size_t e = 0; e < entries; ++e) {
                uint16_t m = 0;
                for (size_t s = 0; s < (size_t)S2; ++s) {
                    m = std::max(m, t[e * S2 + s]);
                    if (s * W >= lq) CHECK(t[e * S2 + s] == 0);
                }
                CHECK(m == t1[e]);
            }
            for (size_t i = 0; i < n; ++i) CHECK(u[i] <= u1[i]);
            // (without a table of the caller's)
            std::vector<uint64_t> u2(n);
            CHECK(swg_debug_prune_kmer_refine(rows.data(), idx, lq, go, ge, S2, flat.data(), off.data(), n, nullptr, u2.data()) == SWG_OK);
            CHECK(u2 == u);
        }
        for (int S2 : {0, 1, 16, 48, 129, 256, -1})
            CHECK(swg_debug_prune_kmer_refine(rows.data(), idx, lq, go, ge, S2, flat.data(), off.data(), n, nullptr, u.data()) == SWG_ERR_ARG);
        int64_t in[8] = {0, 1, 3000, (int64_t)(rng() % 4000000000ull), 0, 0, 0, 0}, out[3];
        for (int64_t refine : {0, 1, 64, 128}) {
            in[7] = refine;
            CHECK(swg_debug_prune_refine_choice(in, out) == SWG_OK);
            CHECK(out[2] == 0 || out[2] == 64 || out[2] == 128);
        }
        in[7] = 32;
        CHECK(swg_debug_prune_refine_choice(in, out) == SWG_ERR_ARG);
        // the stages of 1..4 segments under a random plan: they tile the segments in order
        const int64_t n_seg = 1 + (int64_t)(rng() % 4);
        std::vector<int64_t> ask = {(int64_t)(rng() % 12), (int64_t)(rng() & 1), 64 * (int64_t)(rng() % 3), (int64_t)(rng() & 1), n_seg};
        for (int64_t i = 0, at = 0; i < n_seg; ++i) {
            const int64_t end = at + 1 + (int64_t)(rng() % 9);
            ask.push_back(at), ask.push_back(end), at = end;
        }
        std::vector<int64_t> st(4 * (2 * (size_t)n_seg + 1));
        size_t n_st = 0;
        CHECK(swg_debug_prune_stages(ask.data(), st.data(), st.size() / 4, &n_st) == SWG_OK);
        CHECK(n_st >= (size_t)n_seg && n_st <= (size_t)n_seg + 1);
        for (size_t i = 0; i < n_st; ++i) {
            CHECK(st[4 * i] < st[4 * i + 1] && st[4 * i] == (i ? st[4 * i - 3] : 0));
            CHECK(st[4 * i] >= ask[5 + 2 * st[4 * i + 2]] && st[4 * i + 1] <= ask[6 + 2 * st[4 * i + 2]]);
        }
        CHECK(st[4 * n_st - 3] == ask.back());
        size_t n_again = 0;
        CHECK(swg_debug_prune_stages(ask.data(), st.data(), 1, &n_again) == SWG_OK && n_again == n_st);
        CHECK(swg_debug_prune_stages(ask.data(), nullptr, 0, &n_again) == SWG_OK && n_again == n_st);
    }
    printf("sanitize_prune_refine: %d rounds agreed\n", rounds);
    return 0;
}
