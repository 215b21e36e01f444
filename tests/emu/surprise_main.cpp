// CPU test build only (tests/surprise_cases.py build_driver): a program of its own around the engine's host code and the one-lane build of its
// device code, so that the WEIGHTED drain (gaz_engine_set_sample_weighting, gaz_engine_drain_samples2) runs under
// -fsanitize=address,undefined with caller buffers that are exactly as large as the header says they must be — a library loaded into Python cannot.
// It plays `games` games with the playout cap on, switches the mode on and empties the ring through the C ABI at the buffer limits:
//   max_rows = 0 (refused: the message names the oldest game's rows), one row short (refused, nothing lost), exactly its rows with max_games = 1,
//   max_rows = 2 * max_T (always progress), then max_games = 3 per call, every second call without row_ply.
// Every buffer is a heap block of exactly n_aug * max_rows * state_bytes / n_aug * max_rows * A floats / max_rows floats / max_rows bytes /
// 6 * max_games ints.  Checked here: the row accounting (first rows contiguous, n_rows closing the last game), row_ply ascending and below T,
// games[i][5] == the plies that are missing from row_ply, a game's rows <= 2 * T.
//   surprise_asan key=value ...      keys: game n_games games run_iterations fast_iterations max_actions seed lambda fast_factor
//   exit status 0 = every game was handed out once and every check held, 2 = anything else.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <utility>
#include <vector>
#include "../../include/gaz_engine.h"

static gaz_engine* h = nullptr;
static gaz_sample_layout sl;
static std::set<std::pair<int, int>> handed;

static int fail(const char* what) { fprintf(stderr, "%s: %s\n", what, h ? gaz_engine_last_error(h) : ""); return 2; }

// one drain with buffers of exactly the documented sizes -> 0 ok, 1 refused by the engine, 2 a check failed
static int drain(int max_games, long long max_rows, bool with_plies, int* n_out, long long* rows_out) {
    auto room = [](size_t k) { return k ? k : (size_t)1; };      // (max_rows = 0: a pointer that is not null)
    std::vector<int32_t> games((size_t)6 * max_games);
    std::vector<int8_t> boards(room((size_t)sl.n_aug * max_rows * sl.state_bytes));
    std::vector<float> policies(room((size_t)sl.n_aug * max_rows * sl.A)), values(room((size_t)max_rows));
    std::vector<uint8_t> plies(room((size_t)max_rows));
    int32_t n = 0; int64_t R = 0;
    if (gaz_engine_drain_samples2(h, max_games, max_rows, games.data(), boards.data(), policies.data(), values.data(), with_plies ? plies.data() : nullptr, &n, &R))
        return 1;
    *n_out = n; *rows_out = R;
    if (n > max_games || R > max_rows) return fail("more than the caller's room");
    for (int i = 0; i < n; ++i) {
        const int32_t* g = &games[(size_t)6 * i];
        const long long r0 = g[4], r1 = i + 1 < n ? games[(size_t)6 * (i + 1) + 4] : R;
        if (r0 < 0 || r1 < r0 || r1 > R || (i == 0 && r0 != 0)) return fail("first rows are not contiguous");
        if (r1 - r0 > 2LL * g[0] || g[0] < 1 || g[0] > sl.max_T) return fail("a game with more than 2 T rows");
        if (!handed.insert({g[2], g[3]}).second) return fail("a game was handed out twice");
        if (with_plies) {
            std::vector<int> per(g[0], 0);
            for (long long r = r0; r < r1; ++r) {
                if (plies[r] >= g[0] || (r > r0 && plies[r] < plies[r - 1])) return fail("row_ply is not ascending below T");
                per[plies[r]]++;
            }
            int none = 0;
            for (int c : per) none += c == 0;
            if (none != g[5]) return fail("games[i][5] is not the number of plies without a row");
        }
        for (long long r = r0; r < r1; ++r) if (!(values[r] >= -1.0f && values[r] <= 1.0f)) return fail("a value outside [-1, 1]");
    }
    return 0;
}

int main(int argc, char** argv) {
    std::map<std::string, std::string> kv = {{"game", "Connect4"}, {"n_games", "8"}, {"games", "16"}, {"run_iterations", "30"}, {"fast_iterations", "6"},
        {"max_actions", "42"}, {"seed", "3"}, {"lambda", "0.5"}, {"fast_factor", "1.5"}};
    for (int i = 1; i < argc; ++i) {
        const char* eq = strchr(argv[i], '=');
        const std::string key(argv[i], eq ? (size_t)(eq - argv[i]) : 0);
        if (!eq || !kv.count(key)) { fprintf(stderr, "unknown argument %s\n", argv[i]); return 2; }
        kv[key] = eq + 1;
    }
    auto num = [&](const char* k) { return atoll(kv[k].c_str()); };
    gaz_engine_config c;
    memset(&c, 0, sizeof(c));
    c.struct_size = sizeof(c);
    c.game = kv["game"] == "TicTacToe" ? GAZ_GAME_TICTACTOE : (kv["game"] == "Gomoku" ? GAZ_GAME_GOMOKU : GAZ_GAME_CONNECT4);
    c.search = GAZ_SEARCH_PUCT;
    c.n_games = (int32_t)num("n_games"); c.run_iterations = (int32_t)num("run_iterations"); c.max_actions = (int32_t)num("max_actions");
    c.num_explore_actions_first = 3; c.num_explore_actions_second = 2;
    c.c_puct_init = 2.5; c.c_puct_base = 19652.0; c.dirichlet_alpha = 0.5; c.dirichlet_epsilon = 0.25; c.use_dirichlet = 1;
    c.ring_capacity = (int32_t)num("games") + 4;
    c.seed = (uint64_t)num("seed"); c.hash_salt = 6; c.evaluator = GAZ_EVAL_HASH; c.net_filters = 128;
    c.c_visit = 50.0; c.c_scale = 1.0; c.games_budget = num("games"); c.tau = -1.0; c.leaf_batch = 1; c.gumbel_batch = 1; c.game_groups = 1;
    c.fast_iterations = (int32_t)num("fast_iterations"); c.full_search_prob = c.fast_iterations ? 0.25 : 0.0;
    const long long games = num("games");

    if (gaz_engine_create(&c, &h)) { fprintf(stderr, "create: %s\n", gaz_engine_last_error(nullptr)); return 2; }
    if (gaz_engine_sample_layout(h, &sl)) return fail("sample_layout");
    if (gaz_engine_set_sample_weighting(h, 2.0, 1.5) == 0 || !strstr(gaz_engine_last_error(h), "lambda must be in [0, 1]")) return fail("lambda = 2 was not refused");
    if (gaz_engine_set_sample_weighting(h, atof(kv["lambda"].c_str()), atof(kv["fast_factor"].c_str()))) return fail("set_sample_weighting");
    double lam = -1, ff = -1;
    if (gaz_engine_get_sample_weighting(h, &lam, &ff) || lam != atof(kv["lambda"].c_str()) || ff != atof(kv["fast_factor"].c_str())) return fail("get_sample_weighting");
    uint64_t st[16];
    for (long long launches = 0;; ++launches) {
        if (gaz_engine_run_waves(h, 16) || gaz_engine_get_stats(h, st)) return fail("run_waves");
        if ((long long)st[2] >= games) break;
        if (launches > 1000000) return fail("the games did not finish");
    }
    int n = 0; long long R = 0;
    if (drain(1, 0, true, &n, &R) != 1) return fail("max_rows = 0 was not refused");
    const char* msg = gaz_engine_last_error(h);
    const char* has = strstr(msg, " has ");
    const long long need = has ? atoll(has + 5) : 0;
    if (need < 1 || need > 2LL * sl.max_T || !strstr(msg, "max_rows is 0")) return fail("the refusal does not name the rows");
    if (drain(1, need - 1, true, &n, &R) != 1) return fail("one row short was not refused");
    int rc = drain(1, need, true, &n, &R);
    if (rc || n != 1 || R != need) return rc == 1 ? fail("exactly the oldest game's rows were refused") : 2;
    rc = drain(4, 2LL * sl.max_T, false, &n, &R);
    if (rc || n < 1) return rc == 1 ? fail("max_rows = 2 * max_T made no progress") : 2;
    long long total = 1 + n, rows = need + R;
    for (int call = 0; total < games; ++call) {
        rc = drain(3, 6LL * sl.max_T, call % 2 == 0, &n, &R);
        if (rc || n < 1) return rc == 1 ? fail("drain") : fail("no game was taken");
        total += n; rows += R;
    }
    rc = drain(3, 6LL * sl.max_T, true, &n, &R);
    if (rc || n != 0 || R != 0) return fail("the empty ring gave games");
    printf("%lld games, %lld rows, lambda %g\n", total, rows, lam);
    gaz_engine_destroy(h);
    return total == games && (long long)handed.size() == games ? 0 : 2;
}
