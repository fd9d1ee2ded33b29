// sanitize_prune_adjacent.cpp -- the host code of the fifth pruning level: the choice (swg_prune_refine5_choice,
// swg_debug_prune_refine5_choice), the stage list with its flag (swg_prune_stages, swg_debug_prune_stages6) and the mirror
// (swg_debug_prune_kmer_refine5), all in swg_diag_host.cpp, as a stand-alone program for AddressSanitizer / UBSan.  No GPU
// and no libswg.so: the host files are compiled in, and the few symbols the planner expects from the kernel file are
// defined here (the planner is not run).
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -fopenmp -D__HIP_PLATFORM_AMD__ \
//       -I$ROCM_PATH/include tools/sanitize_prune_adjacent.cpp seq-align-gpu_amd/csrc/swg_diag_host.cpp -x c \
//       seq-align-gpu_amd/host/swg_threads.c -o sanitize_prune_adjacent && ./sanitize_prune_adjacent [rounds]
//
// Every round draws a plan and 1..5 segments: the list with the fifth level tiles the range like the one without it and
// differs from it in the one flag, on exactly the stages that carry the list (never under the prefix cut, never on an uncut
// stage); the hooks from before the level never carry the flag.  The choice answers for every option value, takes the level
// only where the query and scoring admit it, and refuses the values that are no option.  The mirror: a random substitution
// table, query of 1..70 columns and sequences of 0..40 residues (padding rows and every residue index among them), under
// gaps with e > 0 and with e = 0 -- the level is reported off exactly where e = 0 or an entry could pass 255, and where
// it is on, the bound is at most the fourth level's for every N, never below the exact form's, and its last argument
// checks hold.  Exit status 0 = every round agreed.
#include "../seq-align-gpu_amd/csrc/swg_host_internal.h"

#include <cstdio>
#include <cstdlib>
#include <random>

// (the kernel file's geometry tables: not reached from here)
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
    const int rounds = argc > 1 ? atoi(argv[1]) : 60;
    std::mt19937_64 rng(0x5EED5);
    for (int round = 0; round < rounds; ++round) {
        // the stage list
        SwgPrunePlan plan;
        plan.on = true;
        plan.fixed = rng() & 1;
        plan.refine = 64 * (int)(rng() % 3), plan.refine3 = 256 * (int)(rng() & 1), plan.refine4 = 256 * (int)(rng() & 1);
        plan.prefix_cut = !plan.fixed && rng() % 4 == 0;
        plan.gate = rng() & 1;
        plan.head_pairs = (uint32_t)(rng() % 12);
        const size_t n_seg = 1 + rng() % 5;
        std::vector<std::pair<uint32_t, uint32_t>> segs;
        uint32_t at = 0;
        for (size_t i = 0; i < n_seg; ++i) {
            const uint32_t end = at + 1 + (uint32_t)(rng() % 9);
            segs.emplace_back(at, end), at = end;
        }
        const std::vector<SwgPruneStage> plain = swg_prune_stages(plan, segs);
        plan.refine5 = 256;
        const std::vector<SwgPruneStage> fifth = swg_prune_stages(plan, segs);
        CHECK(fifth.size() == plain.size() && !plain.empty());
        for (size_t i = 0; i < plain.size(); ++i) {
            CHECK(fifth[i].begin == plain[i].begin && fifth[i].end == plain[i].end && fifth[i].segment == plain[i].segment);
            CHECK(!(plain[i].queued & SWG_STAGE_REFINE5));
            CHECK(fifth[i].queued == (plain[i].queued | (plain[i].queued & SWG_STAGE_LIST ? SWG_STAGE_REFINE5 : 0u)));
        }
        std::vector<int64_t> ask = {plan.head_pairs, plan.fixed, plan.refine, plan.prefix_cut, plan.refine3, plan.refine4, plan.gate, 256, (int64_t)n_seg};
        for (const auto &sg : segs) ask.push_back(sg.first), ask.push_back(sg.second);
        std::vector<int64_t> st(4 * (2 * n_seg + 1));
        size_t n_st = 0;
        CHECK(swg_debug_prune_stages6(ask.data(), st.data(), st.size() / 4, &n_st) == SWG_OK && n_st == fifth.size());
        for (size_t i = 0; i < n_st; ++i)
            CHECK(st[4 * i] == fifth[i].begin && st[4 * i + 1] == fifth[i].end && st[4 * i + 2] == fifth[i].segment && st[4 * i + 3] == fifth[i].queued);
        ask[7] = 0;
        CHECK(swg_debug_prune_stages6(ask.data(), st.data(), st.size() / 4, &n_st) == SWG_OK && n_st == plain.size());
        for (size_t i = 0; i < n_st; ++i) CHECK(st[4 * i + 3] == plain[i].queued);
        CHECK(swg_debug_prune_stages6(ask.data(), nullptr, 0, &n_st) == SWG_OK && n_st == plain.size());
        ask.erase(ask.begin() + 7);
        CHECK(swg_debug_prune_stages5(ask.data(), st.data(), st.size() / 4, &n_st) == SWG_OK && n_st == plain.size());
        for (size_t i = 0; i < n_st; ++i) CHECK(st[4 * i + 3] == plain[i].queued);
        // the choice
        int64_t in[15] = {(int64_t)(rng() % 3 == 0 ? 4 : 0), 1, 1 + (int64_t)(rng() % 4000), (int64_t)(rng() % 400000000000ull), 0, 0, 0, 0, 0, 8, 0, 8, 0, 1, 0}, out[6], out4[5];
        in[6] = in[0] ? (int64_t)(rng() % 33) : (rng() & 1 ? 32 : 0);
        in[10] = (int64_t[]){0, 1, 5256}[rng() % 3];
        in[11] = rng() % 4 == 0 ? 16 : 8;
        in[14] = rng() % 3 == 0; // (a caller's threshold: forced or off)
        for (int64_t ok : {0, 1})
            for (int64_t v : {0, 1, 5256}) {
                in[12] = v, in[13] = ok;
                CHECK(swg_debug_prune_refine5_choice(in, out) == SWG_OK && swg_debug_prune_refine4_choice(in, out4) == SWG_OK);
                for (int j = 0; j < 5; ++j) CHECK(out[j] == out4[j]);
                CHECK(out[5] == 0 || out[5] == 256);
                const bool can = ok && in[11] == 8 && out[0] >= 1;
                CHECK(!can || v == 1 ? out[5] == 0 : v == 5256 ? out[5] == 256 : (out[5] == 0 || (in[10] == 0 && out[4] == 256 && in[14] == 0)));
            }
        in[1] = 0, in[12] = 5256, in[13] = 1;
        CHECK(swg_debug_prune_refine5_choice(in, out) == SWG_OK && out[5] == 0);
        in[1] = 1;
        for (int64_t v : {-1, 2, 256, 5128}) {
            in[12] = v;
            CHECK(swg_debug_prune_refine5_choice(in, out) == SWG_ERR_ARG);
        }
        in[12] = 0, in[13] = 2;
        CHECK(swg_debug_prune_refine5_choice(in, out) == SWG_ERR_ARG);
        in[13] = 1, in[14] = 2;
        CHECK(swg_debug_prune_refine5_choice(in, out) == SWG_ERR_ARG);
        CHECK(swg_debug_prune_refine5_choice(nullptr, out) == SWG_ERR_ARG);
        // the mirror
        const int top = round % 5 == 4 ? 60 : 5 + (int)(rng() % 20);
        std::vector<int8_t> sub(32 * 32);
        for (auto &v : sub) v = (int8_t)((int)(rng() % (uint64_t)(top + 9)) - 8);
        const size_t lq = 1 + rng() % 70;
        std::vector<int8_t> q(lq);
        for (auto &v : q) v = (int8_t)(1 + rng() % 31);
        const size_t n = 1 + rng() % 6;
        std::vector<int8_t> flat(1, 0);
        std::vector<uint64_t> off(1, 0);
        for (size_t i = 0; i < n; ++i) {
            const size_t len = rng() % 41;
            for (size_t j = 0; j < len; ++j) flat.push_back((int8_t)(rng() % 16 == 0 ? 0 : 1 + rng() % 31));
            off.push_back(off.back() + len);
        }
        const int go = -(int)(rng() % 13), ge = round % 4 == 3 ? 0 : -(int)(1 + rng() % 3);
        int colmax = 0;
        for (size_t i = 0; i < lq; ++i)
            for (int r = 1; r < 32; ++r) colmax = std::max<int>(colmax, sub[32 * q[i] + r]);
        std::vector<uint64_t> u4(n), u5(n, ~0ull), ux(n), un(n);
        int on = -1;
        CHECK(swg_debug_prune_kmer_refine4(sub.data(), q.data(), lq, go, ge, 256, flat.data() + 1, off.data(), n, u4.data()) == SWG_OK);
        CHECK(swg_debug_prune_kmer_refine5(sub.data(), q.data(), lq, go, ge, 256, 0, flat.data() + 1, off.data(), n, u5.data(), &on) == SWG_OK);
        CHECK(on == (ge < 0 && 5 * (colmax - ge) <= 255 ? 1 : 0));
        if (!on) {
            for (size_t i = 0; i < n; ++i) CHECK(u5[i] == ~0ull);
        } else {
            CHECK(swg_debug_prune_kmer_refine5(sub.data(), q.data(), lq, go, ge, 256, 256, flat.data() + 1, off.data(), n, ux.data(), &on) == SWG_OK && on == 1);
            CHECK(swg_debug_prune_kmer_refine5(sub.data(), q.data(), lq, go, ge, 256, 1 + (int)(rng() % 9), flat.data() + 1, off.data(), n, un.data(), &on) == SWG_OK);
            for (size_t i = 0; i < n; ++i) CHECK(ux[i] <= u5[i] && u5[i] <= u4[i] && ux[i] <= un[i] && un[i] <= u4[i]);
        }
        CHECK(swg_debug_prune_kmer_refine5(sub.data(), q.data(), lq, go, ge, 128, 0, flat.data() + 1, off.data(), n, u5.data(), &on) == SWG_ERR_ARG);
        CHECK(swg_debug_prune_kmer_refine5(sub.data(), q.data(), lq, go, ge, 256, -1, flat.data() + 1, off.data(), n, u5.data(), &on) == SWG_ERR_ARG);
        CHECK(swg_debug_prune_kmer_refine5(sub.data(), q.data(), lq, 1, ge, 256, 0, flat.data() + 1, off.data(), n, u5.data(), &on) == SWG_ERR_ARG);
        CHECK(swg_debug_prune_kmer_refine5(sub.data(), q.data(), lq, go, ge, 256, 0, flat.data() + 1, off.data(), n, u5.data(), nullptr) == SWG_ERR_ARG);
        CHECK(swg_debug_prune_kmer_refine5(sub.data(), q.data(), lq, go, ge, 256, 0, flat.data() + 1, off.data(), 0, nullptr, &on) == SWG_OK);
    }
    printf("sanitize_prune_adjacent: %d rounds agreed\n", rounds);
    return 0;
}
