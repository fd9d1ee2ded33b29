// sanitize_prune.cpp -- the host code of the pruned search's levels (swg_diag_host.cpp) as one stand-alone program for
// AddressSanitizer / UBSan: the stage list (swg_prune_stages, swg_prune_bound_range, swg_debug_prune_stages .. stages6),
// the chain of choices (swg_prune_refine_choices, swg_prune_gate_choice and their hooks), the mirrors of the second to the
// fifth level's bound (swg_debug_prune_kmer_refine .. refine5) and the width rule (swg_debug_prune_table_bits).  It stands
// for the five programs the levels came with (sanitize_prune_refine, _bytes, _deep, _gate, _adjacent) and keeps their
// checks.  No GPU and no libswg.so: the host files are compiled in, and the few symbols the planner expects from the
// kernel file are defined here (the planner is not run).
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -fopenmp -D__HIP_PLATFORM_AMD__ \
//       -I$ROCM_PATH/include tools/sanitize_prune.cpp seq-align-gpu_amd/csrc/swg_diag_host.cpp -x c \
//       seq-align-gpu_amd/host/swg_threads.c -o sanitize_prune && ./sanitize_prune [rounds]
//
// Every round (200 by default) draws a plan and 1..5 segments of a range that need not start at pair 0, and an ask of
// the choice hooks.  The stage list must be the one restated here (expect_stages), through the function and through every
// hook that can express the plan; a caller's room for fewer stages is respected; the first level's range and a model of
// the bound array walked in queue order find every word of the range written once.  The chain must be the one restated
// here (expect_chain) for every option value of every level, and every hook from before a level the full hook's first
// columns; values that are no option, widths that are none and NULL are refused.  The mirrors run in the first rounds
// (they cost seconds): 6 of the second and third level's (tables against the unsegmented table, bounds never above the
// coarser one's, the width rule at its edges), 4 of the fourth's (against the table-holding mirror of k = 5, one round a
// database of more than one batch), 60 of the fifth's (off exactly where e = 0 or an entry passes 255, between the exact
// form and the fourth level's).  Exit status 0 = every round agreed.
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

typedef std::mt19937_64 Rng;
typedef std::vector<std::pair<uint32_t, uint32_t>> Segs;

// The stage list, restated: the stages are the segments, or the head and the rest of a lone segment; the first is uncut
// unless the threshold is a caller's; a cut stage queues the threshold kernel (not under a caller's threshold), the first
// level's gated launch on the first stage that has a threshold, then the prefix cut, or the refine gate (the first of
// several stages under a caller's threshold, with a second level), the levels' walks and the list.  Words as numbers: the
// stage bits are part of the hooks' answers.
static std::vector<SwgPruneStage> expect_stages(uint32_t head, bool fixed, bool prefix_cut, bool gate, const int levels[4], const Segs &segs)
{
    std::vector<SwgPruneStage> st;
    for (size_t i = 0; i < segs.size(); ++i) {
        const uint32_t b = segs[i].first, e = segs[i].second;
        if (segs.size() == 1 && head > 0 && b + head < e) {
            st.push_back(SwgPruneStage{b, b + head, 0u, 0u});
            st.push_back(SwgPruneStage{b + head, e, 0u, 0u});
        } else
            st.push_back(SwgPruneStage{b, e, (uint32_t)i, 0u});
    }
    static const uint32_t level_bit[4] = {8u, 32u, 64u, 256u};
    for (size_t i = fixed ? 0 : 1; i < st.size(); ++i) {
        uint32_t q = fixed ? 0u : 1u;
        if (gate && i == (fixed ? 0u : 1u)) q |= 128u;
        if (prefix_cut) q |= 2u;
        else {
            if (levels[0] && fixed && i == 0 && st.size() > 1) q |= 4u;
            for (int l = 0; l < 4; ++l)
                if (levels[l]) q |= level_bit[l];
            q |= 16u;
        }
        st[i].queued = q;
    }
    return st;
}

static int check_stages(Rng &rng, int round)
{
    const bool fixed = rng() & 1, prefix_cut = !fixed && rng() % 4 == 0, gate = rng() & 1;
    const uint32_t head = (uint32_t)(rng() % 12);
    const int levels[4] = {64 * (int)(rng() % 3), 256 * (int)(rng() & 1), 256 * (int)(rng() & 1), 256 * (int)(rng() & 1)};
    const size_t n_seg = 1 + rng() % 5;
    Segs segs;
    uint32_t at = round % 3 == 0 ? (uint32_t)(rng() % 7) : 0u;
    const uint32_t first = at;
    for (size_t i = 0; i < n_seg; ++i) {
        const uint32_t end = at + 1 + (uint32_t)(rng() % 9);
        segs.emplace_back(at, end), at = end;
    }
    const uint32_t n_pairs = at + (uint32_t)(rng() % 3);
    const std::vector<SwgPruneStage> want = expect_stages(head, fixed, prefix_cut, gate, levels, segs);
    CHECK(!want.empty() && want.front().begin == first && want.back().end == at && want.size() >= n_seg && want.size() <= n_seg + 1);
    SwgPrunePlan plan;
    plan.on = true, plan.head_pairs = head, plan.fixed = fixed, plan.prefix_cut = prefix_cut, plan.gate = gate;
    std::copy(levels, levels + 4, plan.refine);
    const std::vector<SwgPruneStage> got = swg_prune_stages(plan, segs);
    CHECK(got.size() == want.size());
    for (size_t i = 0; i < got.size(); ++i) {
        CHECK(got[i].begin == want[i].begin && got[i].end == want[i].end && got[i].segment == want[i].segment && got[i].queued == want[i].queued);
        CHECK(got[i].begin < got[i].end && (i == 0 || got[i].begin == got[i - 1].end));
        CHECK(got[i].begin >= segs[got[i].segment].first && got[i].end <= segs[got[i].segment].second);
    }
    // every hook, with the words it lacks at 0: the list restated for that plan
    typedef int (*Hook)(const int64_t *, int64_t *, size_t, size_t *);
    const Hook hooks[5] = {swg_debug_prune_stages, swg_debug_prune_stages3, swg_debug_prune_stages4, swg_debug_prune_stages5, swg_debug_prune_stages6};
    const int64_t full[8] = {head, fixed, levels[0], prefix_cut, levels[1], levels[2], gate, levels[3]};
    for (int h = 0; h < 5; ++h) {
        const int words = 4 + h; // (in front of n)
        std::vector<int64_t> ask(full, full + words);
        ask.push_back((int64_t)n_seg);
        for (const auto &sg : segs) ask.push_back(sg.first), ask.push_back(sg.second);
        const int part[4] = {levels[0], words > 4 ? levels[1] : 0, words > 5 ? levels[2] : 0, words > 7 ? levels[3] : 0};
        const std::vector<SwgPruneStage> w = expect_stages(head, fixed, prefix_cut, words > 6 && gate, part, segs);
        std::vector<int64_t> st(4 * (2 * n_seg + 1));
        size_t n_st = 0, n_again = 0;
        CHECK(hooks[h](ask.data(), st.data(), st.size() / 4, &n_st) == SWG_OK && n_st == w.size());
        for (size_t i = 0; i < n_st; ++i)
            CHECK(st[4 * i] == w[i].begin && st[4 * i + 1] == w[i].end && st[4 * i + 2] == w[i].segment && st[4 * i + 3] == w[i].queued);
        CHECK(hooks[h](ask.data(), st.data(), 1, &n_again) == SWG_OK && n_again == n_st);
        CHECK(hooks[h](ask.data(), nullptr, 0, &n_again) == SWG_OK && n_again == n_st);
        ask[words] = -1;
        CHECK(hooks[h](ask.data(), st.data(), st.size() / 4, &n_st) == SWG_ERR_ARG);
        CHECK(hooks[h](nullptr, st.data(), st.size() / 4, &n_st) == SWG_ERR_ARG);
    }
    // the range of the first level's launch, and the bound words as the fill's queue order writes them
    const SwgPruneBoundRange br = swg_prune_bound_range(got, n_pairs);
    const size_t flagged = fixed ? 0 : 1;
    if (!gate || flagged >= got.size()) {
        // (no gate; or one uncut stage under the K-th best: no stage has a threshold, the launch stays up front)
        CHECK(br.stage == got.size() && br.begin == 0 && br.end == n_pairs && br.skip_begin == br.skip_end);
        return 0;
    }
    std::vector<int> word(n_pairs + 1, 0); // 0 untouched, 1 "not bounded", 2 bounded; one guard word behind the last pair
    CHECK(br.stage == flagged && br.begin == got[flagged].begin && br.end == at && br.end <= n_pairs);
    CHECK(br.skip_begin == first && br.skip_end == br.begin && (fixed ? br.skip_end == br.skip_begin : br.skip_end > br.skip_begin));
    for (uint32_t p = br.skip_begin; p < br.skip_end; ++p) CHECK(word[p]++ == 0);
    for (size_t i = 0; i < got.size(); ++i) {
        CHECK(((got[i].queued & SWG_STAGE_BOUND) != 0) == (i == flagged));
        if (got[i].queued & SWG_STAGE_BOUND)
            for (uint32_t p = br.begin; p < br.end; ++p) {
                CHECK(word[p] == 0);
                word[p] = 2;
            }
        // a cut stage reads the words of its own pairs only, and they are bounds by then
        if (got[i].queued & (SWG_STAGE_LIST | SWG_STAGE_PREFIX_CUT))
            for (uint32_t p = got[i].begin; p < got[i].end; ++p) CHECK(word[p] == 2);
    }
    for (uint32_t p = 0; p <= n_pairs; ++p) CHECK(word[p] == (p < first || p >= at ? 0 : p < br.begin ? 1 : 2));
    return 0;
}

// The chain, restated from the measured shares and seconds (profiles/prune_refine_ab.txt, prune_bytes_ab.txt,
// prune_deep_ab.txt, prune_adjacent_ab.txt): in = the full choice hook's words, (k, S) the first level's answer.
static void expect_chain(const int64_t *in, int64_t k, int64_t S, int64_t want[4], bool *third_pays)
{
    const double lq = (double)in[2], rows = (double)in[3], table_rate = SWG_KMER_TABLE_RATE, fill_rate = swg_kmer_fill_rate((size_t)in[2]);
    auto pays = [&](double cells, double share, double walk) { return in[2] > 0 && cells * lq / table_rate + walk * rows <= 0.5 * (share * rows / fill_rate); };
    const double cells4 = 234256.0 * 4, cells5 = 234256.0 * 26;
    const bool pruned = in[1] != 0 && k >= 1, first_auto = in[0] == 0 && in[6] == 0, bytes4 = in[9] != 16, bytes5 = in[11] != 16;
    *third_pays = pays(cells4, 0.0151, 1.74e-12);
    want[0] = !pruned ? 0 : in[7] > 1 ? in[7] : in[7] == 1 || !first_auto || k != 4 || S <= 1 ? 0 : pays(cells4, 0.0428, 2.1e-12) ? 128 : pays(cells4, 0.0234, 2.1e-12) ? 64 : 0;
    want[1] = !pruned ? 0 : in[8] > 1 ? 256 : in[8] == 1 || !first_auto || in[7] != 0 || want[0] != 128 || !bytes4 || !*third_pays ? 0 : 256;
    want[2] = !pruned || !bytes5 ? 0
              : in[10] > 1   ? 256
              : in[10] == 1 || !first_auto || in[7] != 0 || in[8] != 0 || want[1] != 256 || !pays(cells5, 0.0374, 1.31e-12) ? 0
                                                                                                                             : 256;
    want[3] = !pruned || !bytes5 || !in[13] ? 0 : in[12] > 1 ? 256 : in[12] == 1 || in[10] != 0 || want[2] == 0 || in[14] || !pays(cells5, 0.0254, 4.0e-12) ? 0 : 256;
}

static int check_choices(Rng &rng, int round)
{
    typedef int (*Hook)(const int64_t *, int64_t *);
    const Hook hooks[4] = {swg_debug_prune_refine_choice, swg_debug_prune_refine3_choice, swg_debug_prune_refine4_choice, swg_debug_prune_refine5_choice};
    static const int64_t values[4][3] = {{0, 1, 64}, {0, 1, 256}, {0, 1, 5256}, {0, 1, 5256}};
    static const int option_word[4] = {7, 8, 10, 12};
    int64_t in[15] = {(int64_t)(rng() % 3 == 0 ? 4 : 0), 1, 1 + (int64_t)(rng() % 4000), (int64_t)(rng() % 400000000000ull), 0, 0, 0, 0, 0, 8, 0, 8, 0, 1, 0};
    in[6] = in[0] ? (int64_t)(rng() % 33) : (rng() & 1 ? 32 : 0);
    if (round % 7 == 0) in[2] = 3000, in[3] = (int64_t)(rng() % 4000000000ull); // (around the levels' floors)
    for (int combos = 0; combos < 24; ++combos) {
        for (int l = 0; l < 4; ++l) in[option_word[l]] = values[l][rng() % 3];
        if (in[7] == 64 && (rng() & 1)) in[7] = 128;
        in[9] = (int64_t[]){0, 8, 16}[rng() % 3], in[11] = (int64_t[]){0, 8, 16}[rng() % 3], in[13] = rng() & 1, in[14] = rng() % 3 == 0;
        int64_t out[6], want[4], part[6], kS[4];
        bool third_pays = false;
        CHECK(swg_debug_prune_kmer_choice_seg(in, kS) == SWG_OK);
        CHECK(hooks[3](in, out) == SWG_OK && out[0] == kS[0] && out[1] == kS[1]);
        expect_chain(in, out[0], out[1], want, &third_pays);
        for (int l = 0; l < 4; ++l) CHECK(out[2 + l] == want[l]);
        // the function itself, and the gate, which keeps the third level's floor
        SwgKmerAsk a;
        a.forced = (long)in[0], a.pruned = in[1] != 0, a.lq = (size_t)in[2], a.pair_rows = (uint64_t)in[3], a.fill_rate = swg_kmer_fill_rate(a.lq);
        a.forced_segments = (long)in[6], a.table_bits = in[9] == 16 ? 16 : 8, a.table_bits5 = in[11] == 16 ? 16 : 8, a.refine5_ok = in[13] != 0, a.fixed = in[14] != 0;
        for (int l = 0; l < 4; ++l) a.forced_refine[l] = (long)in[option_word[l]];
        int levels[SWG_REFINE_LEVELS];
        swg_prune_refine_choices(a, (int)out[0], (int)out[1], levels);
        for (int l = 0; l < 4; ++l) CHECK(levels[l] == want[l]);
        for (int64_t g : {0, 1, 2}) {
            int64_t gin[9] = {in[0], in[1], in[2], in[3], 0, 0, in[6], 0, g}, gout[3];
            CHECK(swg_debug_prune_gate_choice(gin, gout) == SWG_OK && gout[0] == out[0] && gout[1] == out[1]);
            const bool segmented = out[0] > 1 && out[1] > 1;
            CHECK(gout[2] == (g == 1 || !segmented ? 0 : g == 2 ? 1 : in[0] == 0 && in[6] == 0 && third_pays ? 1 : 0));
        }
        // the hooks from before a level: the first columns, whatever the later words hold
        for (int h = 0; h < 3; ++h) {
            CHECK(hooks[h](in, part) == SWG_OK);
            int64_t cut[15];
            std::copy(in, in + 15, cut);
            for (int l = h + 1; l < 4; ++l) cut[option_word[l]] = 0;
            CHECK(hooks[3](cut, out) == SWG_OK);
            for (int j = 0; j < 3 + h; ++j) CHECK(part[j] == out[j]);
        }
    }
    // not pruned: nothing, forced or not
    int64_t out[6];
    in[1] = 0, in[7] = 128, in[8] = 256, in[10] = 5256, in[12] = 5256, in[9] = 8, in[11] = 8, in[13] = 1, in[14] = 0;
    CHECK(hooks[3](in, out) == SWG_OK && out[2] == 0 && out[3] == 0 && out[4] == 0 && out[5] == 0);
    in[1] = 1;
    // what is no option, no width, no flag; NULL
    static const int64_t bad[4][4] = {{-1, 2, 32, 256}, {-1, 2, 128, 5256}, {-1, 2, 256, 5128}, {-1, 2, 256, 5128}};
    for (int l = 0; l < 4; ++l)
        for (int64_t v : bad[l]) {
            const int64_t keep = in[option_word[l]];
            in[option_word[l]] = v;
            for (int h = l; h < 4; ++h) CHECK(hooks[h](in, out) == SWG_ERR_ARG);
            in[option_word[l]] = keep;
        }
    in[9] = 32;
    for (int h = 1; h < 4; ++h) CHECK(hooks[h](in, out) == SWG_ERR_ARG);
    in[9] = 8, in[11] = 32;
    for (int h = 2; h < 4; ++h) CHECK(hooks[h](in, out) == SWG_ERR_ARG);
    in[11] = 8, in[13] = 2;
    CHECK(hooks[3](in, out) == SWG_ERR_ARG);
    in[13] = 1, in[14] = 2;
    CHECK(hooks[3](in, out) == SWG_ERR_ARG);
    in[14] = 0;
    CHECK(hooks[3](in, out) == SWG_OK);
    for (int h = 0; h < 4; ++h) CHECK(hooks[h](nullptr, out) == SWG_ERR_ARG && hooks[h](in, nullptr) == SWG_ERR_ARG);
    int64_t gin[9] = {0, 1, 3000, 1000, 0, 0, 0, 0, 0}, gout[3];
    for (int64_t g : {-1, 3, 256}) {
        gin[8] = g;
        CHECK(swg_debug_prune_gate_choice(gin, gout) == SWG_ERR_ARG);
    }
    CHECK(swg_debug_prune_gate_choice(nullptr, gout) == SWG_ERR_ARG);
    return 0;
}

// The second and third levels' mirrors and the width rule: a random table, an index query or a PSSM of 1..300 columns
// whose largest score is at one of the width rule's edges, gap scores and a database of sequences of 0..150 residues.
static int check_k4_mirrors(Rng &rng, int round)
{
    const size_t entries = (size_t)swg_kmer_entries(4);
    const int tops[] = {63, 64, 51, 52, 127, 11};
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
    std::vector<uint16_t> t1(entries);
    std::vector<uint64_t> u1(n), u128(n), u(n), u2(n);
    CHECK(swg_debug_prune_kmer(rows.data(), idx, lq, go, ge, 4, flat.data(), off.data(), n, t1.data(), u1.data()) == SWG_OK);
    for (int S : {32, 64, 128, 256}) {
        auto mirror = S == 256 ? swg_debug_prune_kmer_refine3 : swg_debug_prune_kmer_refine;
        std::vector<uint16_t> t(entries * (size_t)S);
        CHECK(mirror(rows.data(), idx, lq, go, ge, S, flat.data(), off.data(), n, t.data(), u.data()) == SWG_OK);
        const size_t W = (lq + (size_t)S - 1) / (size_t)S;
        for (size_t e = 0; e < entries; ++e) {
            uint16_t m = 0;
            for (size_t s = 0; s < (size_t)S; ++s) {
                m = std::max(m, t[e * S + s]);
                if (s * W >= lq) CHECK(t[e * S + s] == 0);
            }
            CHECK(m == t1[e]);
            if (bits4 == 8) CHECK(m <= 255);
        }
        for (size_t i = 0; i < n; ++i) CHECK(u[i] <= u1[i]);
        if (S == 128) u128 = u;
        if (S == 256 && (lq + 127) / 128 == 2 * W) // (the 256 segments refine the 128)
            for (size_t i = 0; i < n; ++i) CHECK(u[i] <= u128[i]);
        // (without a table of the caller's)
        CHECK(mirror(rows.data(), idx, lq, go, ge, S, flat.data(), off.data(), n, nullptr, u2.data()) == SWG_OK);
        CHECK(u2 == u);
    }
    for (int S2 : {0, 1, 16, 48, 129, 256, -1})
        CHECK(swg_debug_prune_kmer_refine(rows.data(), idx, lq, go, ge, S2, flat.data(), off.data(), n, nullptr, u.data()) == SWG_ERR_ARG);
    for (int S3 : {0, 1, 32, 64, 128, 255, 257, 512, -1})
        CHECK(swg_debug_prune_kmer_refine3(rows.data(), idx, lq, go, ge, S3, flat.data(), off.data(), n, nullptr, u2.data()) == SWG_ERR_ARG);
    return 0;
}

// The fourth level's mirror, which holds no table, against the table-holding mirror of k = 5: a query of 1..40 columns,
// sequences of 0..150 residues, padding rows inside some; round 2 a database of more than one batch.
static int check_fourth_mirror(Rng &rng, int round)
{
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
    if (lq <= 32) { // (the 256 segments are one column each: the bound is the 32-segment one's)
        CHECK(swg_debug_prune_kmer_seg(rows.data(), idx, lq, go, ge, 5, 32, flat.data(), off.data(), n, nullptr, u32.data()) == SWG_OK);
        CHECK(u == u32 && u128 == u32);
    }
    for (size_t i = 0; i < n; i += 1 + n / 7) { // (one sequence at a time gives what the batch gives)
        const uint64_t o1[2] = {0, off[i + 1] - off[i]};
        CHECK(swg_debug_prune_kmer_refine4(rows.data(), idx, lq, go, ge, 256, flat.data() + off[i], o1, 1, one.data()) == SWG_OK);
        CHECK(one[0] == u[i]);
    }
    CHECK(swg_debug_prune_kmer_refine4(rows.data(), idx, lq, go, ge, 256, flat.data(), off.data(), 0, nullptr) == SWG_OK);
    for (int S4 : {0, 1, 32, 64, 255, 257, 512, -1})
        CHECK(swg_debug_prune_kmer_refine4(rows.data(), idx, lq, go, ge, S4, flat.data(), off.data(), n, u.data()) == SWG_ERR_ARG);
    CHECK(swg_debug_prune_kmer_refine4(rows.data(), idx, lq, 1, ge, 256, flat.data(), off.data(), n, u.data()) == SWG_ERR_ARG);
    CHECK(swg_debug_prune_kmer_refine4(nullptr, idx, lq, go, ge, 256, flat.data(), off.data(), n, u.data()) == SWG_ERR_ARG);
    return 0;
}

// The fifth level's mirror: a random substitution table, a query of 1..70 columns and sequences of 0..40 residues (padding
// rows and every residue index among them), under gaps with e > 0 and with e = 0.
static int check_fifth_mirror(Rng &rng, int round)
{
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
    return 0;
}

int main(int argc, char **argv)
{
    const int rounds = argc > 1 ? atoi(argv[1]) : 200;
    Rng rng(0x5EED);
    for (int round = 0; round < rounds; ++round) {
        if (check_stages(rng, round) || check_choices(rng, round)) return 1;
        if (round < 6 && check_k4_mirrors(rng, round)) return 1;
        if (round < 4 && check_fourth_mirror(rng, round)) return 1;
        if (round < 60 && check_fifth_mirror(rng, round)) return 1;
    }
    printf("sanitize_prune: %d rounds agreed\n", rounds);
    return 0;
}
