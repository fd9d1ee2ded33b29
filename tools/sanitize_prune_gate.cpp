// sanitize_prune_gate.cpp -- the host code of the gate in front of the first pruning level: the choice
// (swg_prune_gate_choice, swg_debug_prune_gate_choice), the stage list with its flag (swg_prune_stages,
// swg_debug_prune_stages5) and the launch's range arithmetic (swg_prune_bound_range), all in swg_diag_host.cpp, as a
// stand-alone program for AddressSanitizer / UBSan.  No GPU and no libswg.so: the host file is compiled in, and the few
// symbols its planner expects from the kernel file are defined here (the planner is not run).
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -fopenmp -D__HIP_PLATFORM_AMD__ \
//       -I$ROCM_PATH/include tools/sanitize_prune_gate.cpp seq-align-gpu_amd/csrc/swg_diag_host.cpp -x c \
//       seq-align-gpu_amd/host/swg_threads.c -o sanitize_prune_gate && ./sanitize_prune_gate [rounds]
//
// Every round draws a plan and 1..5 segments of a range that need not start at pair 0.  The list with the gate tiles the
// range like the one without it and differs from it in the one flag, on the first stage that has a threshold (the second,
// or the first under a caller's threshold) and nowhere without the gate; the hooks from before the gate never carry the
// flag.  The range: without a flagged stage every pair from 0 up front and nothing skipped; with one, from that stage's
// first pair to the range's last, the skipped words exactly the stages in front -- together they tile the range.  A model
// of the bound array walks the launches as the fill queues them and finds every word of the range written once: "not
// bounded" in front of the flagged stage, a bound from it on.  The choice answers for every option value and refuses
// the others.  Exit status 0 = every round agreed.
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
    const int rounds = argc > 1 ? atoi(argv[1]) : 200;
    std::mt19937_64 rng(0x5EED);
    for (int round = 0; round < rounds; ++round) {
        SwgPrunePlan plan;
        plan.on = true;
        plan.fixed = rng() & 1;
        plan.refine = 64 * (int)(rng() % 3), plan.refine3 = 256 * (int)(rng() & 1), plan.refine4 = 256 * (int)(rng() & 1);
        plan.prefix_cut = !plan.fixed && rng() % 4 == 0;
        plan.head_pairs = (uint32_t)(rng() % 12);
        const size_t n_seg = 1 + rng() % 5;
        std::vector<std::pair<uint32_t, uint32_t>> segs;
        uint32_t at = round % 3 == 0 ? (uint32_t)(rng() % 7) : 0u;
        const uint32_t first = at;
        for (size_t i = 0; i < n_seg; ++i) {
            const uint32_t end = at + 1 + (uint32_t)(rng() % 9);
            segs.emplace_back(at, end), at = end;
        }
        const uint32_t n_pairs = at + (uint32_t)(rng() % 3);
        const std::vector<SwgPruneStage> plain = swg_prune_stages(plan, segs);
        plan.gate = true;
        const std::vector<SwgPruneStage> gated = swg_prune_stages(plan, segs);
        CHECK(gated.size() == plain.size() && !plain.empty() && plain.front().begin == first && plain.back().end == at);
        const size_t want = plan.fixed ? 0 : 1;
        for (size_t i = 0; i < plain.size(); ++i) {
            CHECK(gated[i].begin == plain[i].begin && gated[i].end == plain[i].end && gated[i].segment == plain[i].segment);
            CHECK(!(plain[i].queued & SWG_STAGE_BOUND));
            CHECK(gated[i].queued == (plain[i].queued | (i == want ? SWG_STAGE_BOUND : 0u)));
            CHECK(i == 0 || plain[i].begin == plain[i - 1].end);
            if (i == want) CHECK(plan.fixed || (gated[i].queued & SWG_STAGE_THRESHOLD));
        }
        // the hooks: the same list through the new one, no flag through the old ones
        std::vector<int64_t> ask = {plan.head_pairs, plan.fixed, plan.refine, plan.prefix_cut, plan.refine3, plan.refine4, 1, (int64_t)n_seg};
        for (const auto &sg : segs) ask.push_back(sg.first), ask.push_back(sg.second);
        std::vector<int64_t> st(4 * (2 * n_seg + 1));
        size_t n_st = 0;
        CHECK(swg_debug_prune_stages5(ask.data(), st.data(), st.size() / 4, &n_st) == SWG_OK && n_st == gated.size());
        for (size_t i = 0; i < n_st; ++i)
            CHECK(st[4 * i] == gated[i].begin && st[4 * i + 1] == gated[i].end && st[4 * i + 2] == gated[i].segment && st[4 * i + 3] == gated[i].queued);
        ask[6] = 0;
        CHECK(swg_debug_prune_stages5(ask.data(), st.data(), st.size() / 4, &n_st) == SWG_OK && n_st == plain.size());
        for (size_t i = 0; i < n_st; ++i) CHECK(st[4 * i + 3] == plain[i].queued);
        CHECK(swg_debug_prune_stages5(ask.data(), nullptr, 0, &n_st) == SWG_OK && n_st == plain.size());
        ask.erase(ask.begin() + 6);
        CHECK(swg_debug_prune_stages4(ask.data(), st.data(), st.size() / 4, &n_st) == SWG_OK && n_st == plain.size());
        for (size_t i = 0; i < n_st; ++i) CHECK(st[4 * i + 3] == plain[i].queued);
        ask[6] = -1;
        CHECK(swg_debug_prune_stages4(ask.data(), st.data(), st.size() / 4, &n_st) == SWG_ERR_ARG);
        // the range of the launch, and the bound words as the fill's queue order writes them
        const SwgPruneBoundRange none = swg_prune_bound_range(plain, n_pairs);
        CHECK(none.stage == plain.size() && none.begin == 0 && none.end == n_pairs && none.skip_begin == none.skip_end);
        const SwgPruneBoundRange br = swg_prune_bound_range(gated, n_pairs);
        std::vector<int> word(n_pairs + 1, 0); // 0 untouched, 1 "not bounded", 2 bounded; one guard word behind the last pair
        if (want < gated.size()) {
            CHECK(br.stage == want && br.begin == gated[want].begin && br.end == at && br.end <= n_pairs);
            CHECK(br.skip_begin == first && br.skip_end == br.begin && (plan.fixed ? br.skip_end == br.skip_begin : br.skip_end > br.skip_begin));
            for (uint32_t p = br.skip_begin; p < br.skip_end; ++p) CHECK(word[p]++ == 0);
            for (size_t i = 0; i < gated.size(); ++i) {
                if (gated[i].queued & SWG_STAGE_BOUND)
                    for (uint32_t p = br.begin; p < br.end; ++p) {
                        CHECK(word[p] == 0);
                        word[p] = 2;
                    }
                // a cut stage reads the words of its own pairs only, and they are bounds by then
                if (gated[i].queued & (SWG_STAGE_LIST | SWG_STAGE_PREFIX_CUT))
                    for (uint32_t p = gated[i].begin; p < gated[i].end; ++p) CHECK(word[p] == 2);
            }
            for (uint32_t p = 0; p <= n_pairs; ++p) CHECK(word[p] == (p < first || p >= at ? 0 : p < br.begin ? 1 : 2));
        } else {
            // (one uncut stage under the K-th best: no stage has a threshold, the launch stays up front)
            CHECK(!plan.fixed && gated.size() == 1 && br.stage == gated.size() && br.begin == 0 && br.end == n_pairs && br.skip_begin == br.skip_end);
        }
        // the choice
        int64_t in[9] = {(int64_t)(rng() % 3 == 0 ? 4 : 0), 1, 1 + (int64_t)(rng() % 4000), (int64_t)(rng() % 4000000000ull), 0, 0, 0, 0, 0}, out[3];
        in[6] = in[0] ? (int64_t)(rng() % 33) : (rng() & 1 ? 32 : 0);
        for (int64_t g : {0, 1, 2}) {
            in[8] = g;
            CHECK(swg_debug_prune_gate_choice(in, out) == SWG_OK);
            const bool segmented = out[0] > 1 && out[1] > 1;
            CHECK(out[2] == 0 || out[2] == 1);
            CHECK(g == 1 || !segmented ? out[2] == 0 : g == 2 ? out[2] == 1 : (out[2] == 0 || (in[0] == 0 && in[6] == 0)));
        }
        in[1] = 0, in[8] = 2;
        CHECK(swg_debug_prune_gate_choice(in, out) == SWG_OK && out[2] == 0);
        for (int64_t g : {-1, 3, 256}) {
            in[8] = g;
            CHECK(swg_debug_prune_gate_choice(in, out) == SWG_ERR_ARG);
        }
        CHECK(swg_debug_prune_gate_choice(nullptr, out) == SWG_ERR_ARG);
    }
    printf("sanitize_prune_gate: %d rounds agreed\n", rounds);
    return 0;
}
