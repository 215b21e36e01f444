// CPU test build only (tests/emu/Makefile, target capacity_asan): a program of its own around the engine's host code and the one-lane build of its
// device code, so that the error path of a full tree arena can run under -fsanitize=address,undefined — a library loaded into Python cannot.
// It drives the C ABI of include/gaz_engine.h: create, run_waves(1) + drain until a call fails, then `extra_launches` more launches with the
// error standing, then destroy.
//   capacity_asan key=value ...      keys: game search n_games run_iterations max_actions games_budget seed hash_salt nodes_per_tree extra_launches
//                                          leaf_batch compact_trees single_tree gumbel_m gumbel_batch solver eval_symmetry
//   exit status 0 = the arena-full message was seen, 3 = every game finished and no error was raised, 2 = anything else.
// Every other field of the configuration is what tests/capacity_cases.py's engines get from grok_alpha_zero_amd.engine.SelfPlayEngine.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>
#include "../../include/gaz_engine.h"

static const char* ARENA_FULL = "tree arena full (raise nodes_per_tree)";

int main(int argc, char** argv) {
    std::map<std::string, std::string> kv = {{"game", "Connect4"}, {"search", "puct"}, {"n_games", "16"}, {"run_iterations", "30"}, {"max_actions", "42"},
        {"games_budget", "32"}, {"seed", "3"}, {"hash_salt", "2"}, {"nodes_per_tree", "0"}, {"extra_launches", "64"}, {"leaf_batch", "1"},
        {"compact_trees", "0"}, {"single_tree", "0"}, {"gumbel_m", "0"}, {"gumbel_batch", "1"}, {"solver", "0"}, {"eval_symmetry", "0"}};
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
    c.search = kv["search"] == "gumbel" ? GAZ_SEARCH_GUMBEL : GAZ_SEARCH_PUCT;
    c.n_games = (int32_t)num("n_games"); c.run_iterations = (int32_t)num("run_iterations"); c.max_actions = (int32_t)num("max_actions");
    c.num_explore_actions_first = 2; c.num_explore_actions_second = 2;
    c.c_puct_init = 2.5; c.c_puct_base = 19652.0; c.dirichlet_alpha = 0.5; c.dirichlet_epsilon = 0.25; c.use_dirichlet = 1;
    c.nodes_per_tree = (int32_t)num("nodes_per_tree"); c.ring_capacity = 4 * c.n_games;
    c.seed = (uint64_t)num("seed"); c.hash_salt = (uint32_t)num("hash_salt"); c.evaluator = GAZ_EVAL_HASH; c.net_filters = 128;
    c.gumbel_m = (int32_t)num("gumbel_m"); c.c_visit = 50.0; c.c_scale = 1.0;
    c.compact_trees = (int32_t)num("compact_trees"); c.single_tree = (int32_t)num("single_tree");
    c.games_budget = num("games_budget"); c.tau = -1.0;
    c.leaf_batch = (int32_t)num("leaf_batch"); c.gumbel_batch = (int32_t)num("gumbel_batch");
    const long long games = num("games_budget");
    const int extra = (int)num("extra_launches");

    gaz_engine* h = nullptr;
    if (gaz_engine_create(&c, &h)) { fprintf(stderr, "create: %s\n", gaz_engine_last_error(nullptr)); return 2; }
    if (num("solver") && gaz_engine_set_solver(h, 1)) { fprintf(stderr, "%s\n", gaz_engine_last_error(h)); return 2; }
    if (num("eval_symmetry") && gaz_engine_set_eval_symmetry(h, 1)) { fprintf(stderr, "%s\n", gaz_engine_last_error(h)); return 2; }
    gaz_record_layout lay;
    if (gaz_engine_record_layout(h, &lay)) return 2;
    std::vector<uint8_t> buf((size_t)c.ring_capacity * lay.record_bytes);
    std::vector<int32_t> n_hist(c.n_games);
    std::vector<uint8_t> hist((size_t)c.n_games * lay.t_pad);
    long long finished = 0, launches = 0;
    bool failed = false;
    while (!failed && finished < games && launches < 10000000) {
        int32_t n = 0;
        failed = gaz_engine_run_waves(h, 1) != 0 || gaz_engine_drain_finished(h, buf.data(), c.ring_capacity, &n) != 0;
        finished += n; ++launches;
    }
    if (!failed) failed = gaz_engine_synchronize(h) != 0;
    if (!failed) {
        printf("%lld games in %lld launches, no error\n", finished, launches);
        gaz_engine_destroy(h);
        return finished == games ? 3 : 2;
    }
    const std::string first = gaz_engine_last_error(h);
    printf("after %lld launches and %lld games: %s\n", launches, finished, first.c_str());
    for (int i = 0; i < extra; ++i) {              // the error stands: the launches go on, every synchronising call repeats it, state can still be read
        int32_t n = 0;
        uint64_t st[16];
        gaz_engine_run_waves(h, 1);
        if (gaz_engine_drain_finished(h, buf.data(), c.ring_capacity, &n) == 0 || gaz_engine_get_stats(h, st) == 0) { fprintf(stderr, "the error did not stick\n"); return 2; }
        if (gaz_engine_read_positions(h, n_hist.data(), hist.data(), lay.t_pad)) { fprintf(stderr, "%s\n", gaz_engine_last_error(h)); return 2; }
    }
    const bool same = first == gaz_engine_last_error(h);
    gaz_engine_destroy(h);
    if (!same) { fprintf(stderr, "the message changed\n"); return 2; }
    return first.find(ARENA_FULL) != std::string::npos ? 0 : 2;
}
