// sanitize_prune_deep.cpp -- the host code of the fourth-level pruning bound: its mirror, which holds no table
// (swg_debug_prune_kmer_refine4), its choice (swg_debug_prune_refine4_choice) and the stage list with its flag
// (swg_debug_prune_stages4), all in swg_diag_host.cpp, as a stand-alone program for AddressSanitizer / UBSan.  No GPU
// and no libswg.so: the host file is compiled in, and the few symbols its planner expects from the kernel file are
// defined here (the planner is not run).
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -fopenmp -D__HIP_PLATFORM_AMD__ \
//       -I$ROCM_PATH/include tools/sanitize_prune_deep.cpp seq-align-gpu_amd/csrc/swg_diag_host.cpp -x c \
//       seq-align-gpu_amd/host/swg_threads.c -o sanitize_prune_deep && ./sanitize_prune_deep [rounds]
//
// Every round draws a random table, an index query or a PSSM of 1..40 columns, gap scores and a database of sequences of
// 0..150 residues, padding rows inside some, and checks the mirror against the table-holding mirror of k = 5: at up to 32
// columns the 256 segments are one column each and the bound is swg_debug_prune_kmer_seg's at 32 segments; at any length
// the bound is never above the unsegmented one of k = 5; one sequence at a time gives what the batch gives (a batch
// shares the rows of equal prefixes, a lone sequence's blocks share none with another's); 128 and 256 are the only
// segment counts.  One round runs a database of more than one batch.  The choice answers 0 or 256 for every option value
// and width and refuses the others; the stage list with the fourth level tiles the segments like the one without and
// carries the flag exactly on the stages that carry the list's.  Exit status 0 = every round agreed.
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
    const int rounds = argc > 1 ? atoi(argv[1]) : 4;
    std::mt19937_64 rng(0x5EED);
    for (int round = 0; round < rounds; ++round) {
        const size_t lq = round == 0 ? 1 : round == 1 ? 32 : 1 + rng() % 40;
        const bool pssm = round & 1;
        std::vector<int8_t> rows((pssm ? lq : 32) * 32), q(lq);
        for (int8_t &v : rows) v = (int8_t)((int)(rng() % 16) - 6);
        for (int8_t &v : q) v = (int8_t)(1 + rng() % 31);
        const int8_t *idx = pssm ? nullptr : q.data();
        const int go = -(int)(rng() % 12), ge = -(int)(rng() % 3);
        // (round 2: 700 sequences, some 14 000 blocks a batch of 32 768 does not hold ... with the long ones below)
        const size_t n = round == 2 ? 700 : 1 + rng() % 40;
        std::vector<uint64_t> off(n + 1, 0);
        for (size_t i = 0; i < n; ++i) off[i + 1] = off[i] + (round == 2 ? 150 + rng() % 151 : rng() % 151);
        std::vector<int8_t> flat(off[n] + 1);
        for (int8_t &v : flat) v = (int8_t)(1 + rng() % 31);
        for (size_t i = 0; i < n; i += 5) // (the shorter sequence of a pair, filled up with padding rows)
            for (uint64_t r = off[i] + (off[i + 1] - off[i]) / 2; r < off[i + 1]; ++r) flat[r] = 0;
        std::vector<uint64_t> u(n), u128(n), u5(n), u32(n), one(1);
        CHECK(swg_debug_prune_kmer_refine4(rows.data(), idx, lq, go, ge, 256, flat.data(), off.data(), n, u.data()) == SWG_OK);
        CHECK(swg_debug_prune_kmer_refine4(rows.data(), idx, lq, go, ge, 128, flat.data(), off.data(), n, u128.data()) == SWG_OK);
        CHECK(swg_debug_prune_kmer(rows.data(), idx, lq, go, ge, 5, flat.data(), off.data(), n, nullptr, u5.data()) == SWG_OK);
        for (size_t i = 0; i < n; ++i) CHECK(u[i] <= u5[i] && u128[i] <= u5[i]);
        if (lq <= 32) {
            CHECK(swg_debug_prune_kmer_seg(rows.data(), idx, lq, go, ge, 5, 32, flat.data(), off.data(), n, nullptr, u32.data()) == SWG_OK);
            CHECK(u == u32 && u128 == u32);
        }
        for (size_t i = 0; i < n; i += 1 + n / 7) {
            const uint64_t o1[2] = {0, off[i + 1] - off[i]};
            CHECK(swg_debug_prune_kmer_refine4(rows.data(), idx, lq, go, ge, 256, flat.data() + off[i], o1, 1, one.data()) == SWG_OK);
            CHECK(one[0] == u[i]);
        }
        CHECK(swg_debug_prune_kmer_refine4(rows.data(), idx, lq, go, ge, 256, flat.data(), off.data(), 0, nullptr) == SWG_OK);
        for (int S4 : {0, 1, 32, 64, 255, 257, 512, -1})
            CHECK(swg_debug_prune_kmer_refine4(rows.data(), idx, lq, go, ge, S4, flat.data(), off.data(), n, u.data()) == SWG_ERR_ARG);
        CHECK(swg_debug_prune_kmer_refine4(rows.data(), idx, lq, 1, ge, 256, flat.data(), off.data(), n, u.data()) == SWG_ERR_ARG);
        CHECK(swg_debug_prune_kmer_refine4(nullptr, idx, lq, go, ge, 256, flat.data(), off.data(), n, u.data()) == SWG_ERR_ARG);
        // the choice: every option value, either width of either table
        int64_t in[12] = {0, 1, 3000, (int64_t)(rng() % 4000000000ull), 0, 0, 0, 0, 0, 0, 0, 0}, out[5];
        for (int64_t r4 : {0, 1, SWG_REFINE4_FORCED})
            for (int64_t b4 : {0, 8, 16})
                for (int64_t b5 : {0, 8, 16}) {
                    in[9] = b4, in[10] = r4, in[11] = b5;
                    CHECK(swg_debug_prune_refine4_choice(in, out) == SWG_OK);
                    CHECK(b5 == 16 || r4 == 1 ? out[4] == 0 : r4 ? out[4] == 256 : (out[4] == 0 || (out[4] == 256 && out[3] == 256 && b4 != 16)));
                }
        in[10] = 256;
        CHECK(swg_debug_prune_refine4_choice(in, out) == SWG_ERR_ARG);
        in[10] = 0, in[11] = 32;
        CHECK(swg_debug_prune_refine4_choice(in, out) == SWG_ERR_ARG);
        // the stages of 1..4 segments under a random plan, with and without the fourth level
        const int64_t n_seg = 1 + (int64_t)(rng() % 4);
        std::vector<int64_t> ask = {(int64_t)(rng() % 12), (int64_t)(rng() & 1), 64 * (int64_t)(rng() % 3), (int64_t)(rng() & 1), 256 * (int64_t)(rng() & 1), n_seg}, ask4;
        for (int64_t i = 0, at = 0; i < n_seg; ++i) {
            const int64_t end = at + 1 + (int64_t)(rng() % 9);
            ask.push_back(at), ask.push_back(end), at = end;
        }
        ask4 = ask;
        ask4.insert(ask4.begin() + 5, 256);
        std::vector<int64_t> st(4 * (2 * (size_t)n_seg + 1)), st4(st.size());
        size_t n_st = 0, n_st4 = 0;
        CHECK(swg_debug_prune_stages3(ask.data(), st.data(), st.size() / 4, &n_st) == SWG_OK);
        CHECK(swg_debug_prune_stages4(ask4.data(), st4.data(), st4.size() / 4, &n_st4) == SWG_OK && n_st4 == n_st);
        for (size_t i = 0; i < n_st; ++i) {
            CHECK(st4[4 * i] == st[4 * i] && st4[4 * i + 1] == st[4 * i + 1] && st4[4 * i + 2] == st[4 * i + 2]);
            const int64_t with = st[4 * i + 3] & SWG_STAGE_LIST ? st[4 * i + 3] | SWG_STAGE_REFINE4 : st[4 * i + 3];
            CHECK(st4[4 * i + 3] == with);
        }
        CHECK(swg_debug_prune_stages4(ask4.data(), nullptr, 0, &n_st4) == SWG_OK && n_st4 == n_st);
        ask4[6] = -1;
        CHECK(swg_debug_prune_stages4(ask4.data(), st4.data(), st4.size() / 4, &n_st4) == SWG_ERR_ARG);
    }
    printf("sanitize_prune_deep: %d rounds agreed\n", rounds);
    return 0;
}
