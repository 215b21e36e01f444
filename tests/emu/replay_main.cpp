// CPU test build only (tests/replay_cases.py build_driver): a program of its own around the engine's host code and the one-lane build of its
// device code, so that the replay window (gaz_replay_*) runs under -fsanitize=address,undefined with caller buffers that are exactly as large as
// the header says they must be — a library loaded into Python cannot.
// It appends generations of ragged games (a game without rows among them) until the ring has wrapped and whole generations have left, evicts,
// builds plans for both splits and reads every epoch back in batches of odd sizes, with and without the index arrays.  Every buffer is a heap
// block of exactly n * state_bytes / n * A floats / n floats / n u32 / n bytes.  Checked here: the row accounting of gaz_replay_info, that a plan
// is ascending and below the live rows, that an epoch's source rows are a permutation of its plan, that a symmetry is below n_aug, that a row
// sampled without augmentation is the stored row, and the refusals at the limits.
//   replay_asan key=value ...      keys: game (0 TicTacToe, 1 Connect4, 2 Gomoku) capacity seed
//   exit status 0 = every check held, 2 = anything else.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>
#include "../../include/gaz_engine.h"

static gaz_replay* h = nullptr;
static int fail(const char* what) { fprintf(stderr, "%s: %s\n", what, h ? gaz_replay_last_error(h) : gaz_replay_last_error(nullptr)); return 2; }

int main(int argc, char** argv) {
    std::map<std::string, std::string> kv = {{"game", "1"}, {"capacity", "61"}, {"seed", "4"}};
    for (int i = 1; i < argc; ++i) {
        const char* eq = strchr(argv[i], '=');
        const std::string key(argv[i], eq ? (size_t)(eq - argv[i]) : 0);
        if (!eq || !kv.count(key)) { fprintf(stderr, "unknown argument %s\n", argv[i]); return 2; }
        kv[key] = eq + 1;
    }
    const int game = atoi(kv["game"].c_str());
    const long long cap = atoll(kv["capacity"].c_str());
    static const int dims[3][3] = {{18, 9, 8}, {168, 7, 2}, {450, 225, 8}};                // state bytes, actions, augmentations
    const int SB = dims[game][0], A = dims[game][1], NA = dims[game][2];

    gaz_replay_config c;
    memset(&c, 0, sizeof(c));
    c.struct_size = sizeof(c) - 4; c.game = game; c.capacity_rows = cap; c.seed = (uint64_t)atoll(kv["seed"].c_str()); c.test_fraction = 0.25; c.target_ratio = 0.5;
    if (gaz_replay_create(&c, &h) == 0 || !strstr(gaz_replay_last_error(nullptr), "struct_size")) return fail("a stale struct_size was not refused");
    c.struct_size = sizeof(c);
    if (gaz_replay_create(&c, &h)) return fail("create");

    unsigned rng = 12345u + (unsigned)game;
    auto next = [&]() { rng = rng * 1664525u + 1013904223u; return rng >> 8; };
    long long live = 0;
    std::vector<long long> gen_rows;                                                    // rows of the live generations, oldest first
    for (int gen = 0; gen < 6; ++gen) {
        // two appends per generation, games of 0 .. 6 rows, about a third of the capacity per generation
        for (int part = 0; part < 2; ++part) {
            std::vector<int32_t> games;
            long long R = 0;
            while (R < cap / 6) {
                const int rows = (int)(next() % 7);
                const int32_t g6[6] = {rows, 0, 0, 0, (int32_t)R, 0};
                games.insert(games.end(), g6, g6 + 6);
                R += rows;
            }
            std::vector<int8_t> boards((size_t)R * SB);
            std::vector<float> pol((size_t)R * A), val((size_t)R);
            for (auto& x : boards) x = (int8_t)next();
            for (auto& x : pol) x = (float)(next() % 1000) / 1000.0f;
            for (auto& x : val) x = (float)(next() % 2001) / 1000.0f - 1.0f;
            if (gaz_replay_append(h, gen, (int32_t)(games.size() / 6), games.data(), boards.data(), pol.data(), val.data(), R)) return fail("append");
            if (part == 0) gen_rows.push_back(0);
            gen_rows.back() += R; live += R;
            while (live > cap) { live -= gen_rows.front(); gen_rows.erase(gen_rows.begin()); }
        }
        int64_t info[8]; int32_t n_gens = 0;
        std::vector<int64_t> g3(3 * gen_rows.size());
        if (gaz_replay_info(h, info, (int32_t)gen_rows.size(), g3.data(), &n_gens)) return fail("info");
        if (info[0] != live || n_gens != (int32_t)gen_rows.size() || info[3] != gen || info[4] < 0 || info[4] > live) return fail("info does not match the rows appended");
        for (size_t i = 0; i < gen_rows.size(); ++i) if (g3[3 * i + 2] != gen_rows[i]) return fail("a generation's rows");

        for (int split = 0; split < 2; ++split) {
            int64_t M = -1;
            if (gaz_replay_begin_epoch(h, split, (uint32_t)gen, gen, 1.0, 0.4, &M)) return fail("begin_epoch");
            if (M < 0 || M > live) return fail("a plan larger than the window");
            std::vector<uint32_t> plan((size_t)M);
            if (gaz_replay_read_plan(h, 0, M, plan.data())) return fail("read_plan");
            for (int64_t i = 0; i < M; ++i) if (plan[i] >= (uint32_t)live || (i && plan[i] <= plan[i - 1])) return fail("the plan is not ascending below the live rows");
            if (gaz_replay_sample(h, M, 1, 1) == 0 || !strstr(gaz_replay_last_error(h), "of an epoch of")) return fail("a batch beyond the plan was not refused");
            std::vector<int> hit((size_t)live, 0);
            const int sizes[4] = {1, 7, 64, 5};
            int64_t first = 0;
            for (int call = 0; first < M; ++call) {
                const int n = (int)std::min<int64_t>(sizes[call % 4], M - first);
                const int augment = call % 3 != 2;
                std::vector<int8_t> b((size_t)n * SB);
                std::vector<float> p((size_t)n * A), v((size_t)n);
                std::vector<uint32_t> rows((size_t)n);
                std::vector<uint8_t> sym((size_t)n);
                if (gaz_replay_sample(h, first, n, augment)) return fail("sample");
                if (gaz_replay_read_batch(h, b.data(), p.data(), v.data(), rows.data(), sym.data())) return fail("read_batch");
                for (int q = 0; q < n; ++q) {
                    if (rows[q] >= (uint32_t)live || sym[q] >= NA || (!augment && sym[q])) return fail("a source row or a symmetry out of range");
                    hit[rows[q]]++;
                    if (!augment) {                                                     // the stored row itself
                        std::vector<int8_t> sb((size_t)SB); std::vector<float> sp((size_t)A); float sv = 0; int32_t meta[3];
                        if (gaz_replay_read_rows(h, rows[q], 1, sb.data(), sp.data(), &sv, meta)) return fail("read_rows");
                        if (memcmp(sb.data(), &b[(size_t)q * SB], SB) || memcmp(sp.data(), &p[(size_t)q * A], (size_t)A * 4) || sv != v[q]) return fail("an un-augmented row differs from the store");
                        if (meta[0] > gen || meta[1] < 0 || meta[2] < 0) return fail("a row's meta");
                    }
                }
                if (call % 2 && gaz_replay_read_batch(h, b.data(), nullptr, nullptr, nullptr, nullptr)) return fail("read_batch with null outputs");
                first += n;
            }
            for (int64_t i = 0; i < M; ++i) if (hit[plan[i]] != 1) return fail("the epoch is not a permutation of its plan");
            if (gaz_replay_sample(h, M, 0, 1)) return fail("n = 0 at the end of the epoch was refused");
        }
    }
    if (gaz_replay_append(h, 2, 0, nullptr, nullptr, nullptr, nullptr, 0) == 0 || !strstr(gaz_replay_last_error(h), "non-decreasing")) return fail("an older generation was not refused");
    if (gaz_replay_evict(h, 5)) return fail("evict");
    int64_t info[8];
    if (gaz_replay_info(h, info, 0, nullptr, nullptr) || info[2] != 5 || info[7] != -1) return fail("info after evict");
    if (gaz_replay_evict(h, 100) || gaz_replay_info(h, info, 0, nullptr, nullptr) || info[0] != 0 || info[1] != 0) return fail("evict everything");
    int64_t M = -1;
    if (gaz_replay_begin_epoch(h, 0, 0, 0, 1.0, 0.0, &M) || M != 0) return fail("the plan of an empty window");
    printf("game %d: capacity %lld, six generations\n", game, cap);
    gaz_replay_destroy(h);
    return 0;
}
