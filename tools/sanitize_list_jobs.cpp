// sanitize_list_jobs.cpp -- the host job table of swg_search_lists (swg_list_jobs, swg_pack.cpp) on random candidate
// lists, as a stand-alone program for AddressSanitizer / UBSan.  No GPU and no libswg.so: the packer is compiled in, and
// the few symbols it expects from the API layer are defined here.
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -fopenmp -D__HIP_PLATFORM_AMD__ \
//       -I$ROCM_PATH/include tools/sanitize_list_jobs.cpp seq-align-gpu_amd/csrc/swg_pack.cpp -x c \
//       seq-align-gpu_amd/host/swg_threads.c -o sanitize_list_jobs && ./sanitize_list_jobs [rounds]
//
// Every round packs a random database (whole, or one shard of three), draws lists of every awkward shape -- empty, one
// entry, odd and even sizes, duplicates, everything, the same list twice --, optionally through a view of a random
// subset, and checks the table against a restatement with std::set.  Exit status 0 = every round agreed.
#include "../seq-align-gpu_amd/csrc/swg_host_internal.h"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>

static std::string g_err;
int swg_set_global_error(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
extern "C" const char *swg_global_error(void) { return g_err.c_str(); }
void swg_db_release_device(swg_db *) {}
void swg_db_release_search_state(swg_db *) {}

#define CHECK(c)                                                                \
    do {                                                                        \
        if (!(c)) {                                                             \
            fprintf(stderr, "round %d: %s failed (line %d)\n", round, #c, __LINE__); \
            return 1;                                                           \
        }                                                                       \
    } while (0)

int main(int argc, char **argv)
{
    const int rounds = argc > 1 ? atoi(argv[1]) : 40;
    std::mt19937_64 rng(0x5EED);
    for (int round = 0; round < rounds; ++round) {
        const size_t n = 1 + rng() % 700;
        std::vector<uint64_t> off(n + 1, 0);
        for (size_t i = 0; i < n; ++i) off[i + 1] = off[i] + 1 + rng() % 90;
        std::vector<int8_t> flat(off[n]);
        for (auto &r : flat) r = (int8_t)(1 + rng() % 25);
        const int shards = round % 3 == 2 ? 3 : 1, rank = shards == 3 ? (int)(rng() % 3) : 0;
        swg_db *db = nullptr;
        CHECK(swg_db_pack(flat.data(), off.data(), n, rank, shards, &db) == SWG_OK);
        swg_db *use = db, *view = nullptr;
        std::set<uint32_t> in_view;
        if (round % 4 == 1) { // through a view of a random half
            std::vector<uint32_t> pick, slots;
            for (size_t i = 0; i < n; ++i)
                if (rng() & 1) pick.push_back((uint32_t)i);
            CHECK(swg_view_select(db, pick.data(), pick.size(), &slots) == SWG_OK);
            view = swg_view_host(db, slots);
            use = view;
            in_view.insert(pick.begin(), pick.end());
        }
        const size_t nq = 1 + rng() % 12;
        std::vector<uint64_t> c_off(nq + 1, 0);
        std::vector<uint32_t> cand;
        for (size_t q = 0; q < nq; ++q) {
            const size_t shape = rng() % 7;
            size_t len = shape == 0 ? 0 : shape == 1 ? 1 : shape == 2 ? n : 1 + rng() % (2 * n);
            if (shape == 3 && q > 0) { // the previous list once more
                cand.insert(cand.end(), cand.begin() + (long)c_off[q - 1], cand.begin() + (long)c_off[q]);
            } else if (shape == 2) {
                for (size_t i = 0; i < n; ++i) cand.push_back((uint32_t)(n - 1 - i));
            } else {
                for (size_t i = 0; i < len; ++i) cand.push_back((uint32_t)(rng() % n));
            }
            c_off[q + 1] = cand.size();
        }
        SwgListJobs J;
        CHECK(swg_list_jobs(use, cand.empty() ? nullptr : cand.data(), c_off.data(), 0, nq, &J) == SWG_OK);
        const swg_db *root = db;
        CHECK(J.row_pairs.size() == nq + 1 && J.row_pairs[0] == 0 && J.entry_job.size() == cand.size());
        CHECK(J.slots.size() == 2 * J.row_pairs[nq]);
        for (size_t q = 0; q < nq; ++q) {
            std::set<uint32_t> want; // the held slots of the list's distinct entries
            for (uint64_t e = c_off[q]; e < c_off[q + 1]; ++e)
                for (size_t s = 0; s < root->order.size(); ++s)
                    if (root->order[s] == cand[e] && (!view || in_view.count(cand[e]))) want.insert((uint32_t)s);
            const size_t b = 2 * J.row_pairs[q], e2 = 2 * J.row_pairs[q + 1];
            CHECK(e2 - b == want.size() + (want.size() & 1));
            size_t at = b;
            uint64_t residues = 0;
            for (const uint32_t s : want) {
                CHECK(J.slots[at++] == s);
                residues += root->lens[s];
            }
            if (want.size() & 1) CHECK(J.slots[at] == 0xFFFFFFFFu);
            CHECK(J.row_residues[q] == residues);
            CHECK(J.row_longest[q] == (want.empty() ? 0u : root->lens[*want.begin()]));
            for (uint64_t e = c_off[q]; e < c_off[q + 1]; ++e) {
                const uint32_t j = J.entry_job[e];
                if (j == 0xFFFFFFFFu) {
                    for (const uint32_t s : want) CHECK(root->order[s] != cand[e]);
                } else {
                    CHECK(j >= b && j < e2 && J.slots[j] != 0xFFFFFFFFu && root->order[J.slots[j]] == cand[e]);
                }
            }
        }
        // the launch's workgroups dealt over J: every row with pairs exactly once in the table's row order, none empty
        for (const uint64_t resident : {(uint64_t)1, (uint64_t)64, (uint64_t)1024}) {
            std::vector<uint2> wgs;
            swg_lists_deal(J, 1 + rng() % 16, resident, (rng() & 1) != 0, &wgs);
            std::vector<uint32_t> count(nq, 0);
            for (size_t b = 0; b < wgs.size(); ++b) {
                CHECK(wgs[b].x < nq && J.row_pairs[wgs[b].x + 1] > J.row_pairs[wgs[b].x] && wgs[b].y == count[wgs[b].x]);
                ++count[wgs[b].x];
            }
            for (size_t q = 0; q < nq; ++q) CHECK((count[q] > 0) == (J.row_pairs[q + 1] > J.row_pairs[q]));
        }
        CHECK(J.pair_blocks.size() == J.slots.size() / 2 + 1);
        // a second chunk of the same call: queries [1, nq)
        if (nq > 1) {
            SwgListJobs K;
            CHECK(swg_list_jobs(use, cand.data(), c_off.data(), 1, nq - 1, &K) == SWG_OK);
            CHECK(K.entry0 == c_off[1] && K.row_pairs.size() == nq && K.slots.size() == J.slots.size() - 2 * J.row_pairs[1]);
        }
        // the hook, with too small and large enough a buffer, and an index beyond the database
        size_t ns = 0;
        std::vector<uint32_t> out(J.slots.size() + 1);
        std::vector<uint64_t> pre(nq + 1);
        CHECK(swg_debug_list_jobs(use, cand.data(), c_off.data(), nq, nullptr, 0, &ns, pre.data()) == SWG_OK && ns == J.slots.size());
        CHECK(swg_debug_list_jobs(use, cand.data(), c_off.data(), nq, out.data(), out.size(), &ns, pre.data()) == SWG_OK);
        CHECK(std::equal(J.slots.begin(), J.slots.end(), out.begin()) && pre == J.row_pairs);
        if (!cand.empty()) {
            cand.back() = (uint32_t)n;
            CHECK(swg_list_jobs(use, cand.data(), c_off.data(), 0, nq, &J) == SWG_ERR_ARG);
        }
        if (view) swg_db_free(view);
        swg_db_free(db);
    }
    printf("%d rounds agreed\n", rounds);
    return 0;
}
