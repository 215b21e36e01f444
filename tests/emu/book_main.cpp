// CPU test build only (tests/opening_book_cases.py build_driver): a program of its own around the engine's host code and the one-lane build of
// its device code, so that the opening book (gaz_engine_set_opening_book, gaz_engine_get_opening_book, gaz_engine_read_book_counts) runs under
// -fsanitize=address,undefined with caller buffers of exactly the documented sizes — a library loaded into Python cannot.
// It walks the refusal paths (each must fail with its text and leave the book in force as it was), sets a book whose table is a heap block of
// exactly n_entries * stride bytes, plays three games per slot, takes half of them as records (the prefix is an entry of the book, its plies
// are kind 3 with zero rows) and the rest as samples (a game has T - games[i][5] rows), reads the counters into a block of exactly n_entries
// words, and removes the book.
//   book_asan key=value ...      keys: game n_games run_iterations max_actions seed mode gumbel game_groups
//   exit status 0 = every check held, 2 = anything else.
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
typedef std::vector<std::vector<int>> Book;

static int fail(const char* what) { fprintf(stderr, "%s: %s\n", what, h ? gaz_engine_last_error(h) : ""); return 2; }

static int set_book(const Book& b, int mode, int stride_override = 0, uint32_t size = sizeof(gaz_book_params), int n_override = -2, bool null_actions = false) {
    size_t stride = 1;
    for (const auto& e : b) if (e.size() > stride) stride = e.size();
    std::vector<uint8_t> acts(b.size() * stride ? b.size() * stride : 1);            // exactly n_entries * stride bytes
    std::vector<int32_t> lens(b.size() ? b.size() : 1);
    for (size_t i = 0; i < b.size(); ++i) { lens[i] = (int32_t)b[i].size(); for (size_t k = 0; k < b[i].size(); ++k) acts[i * stride + k] = (uint8_t)b[i][k]; }
    gaz_book_params p; p.struct_size = size; p.n_entries = n_override != -2 ? n_override : (int32_t)b.size(); p.stride = stride_override ? stride_override : (int32_t)stride; p.mode = mode;
    return gaz_engine_set_opening_book(h, &p, null_actions ? nullptr : acts.data(), lens.data());
}

// a refused call: non-zero, its text, and the book in force unchanged
static int refused(int rc, const char* text, int n_before, int mode_before) {
    if (rc == 0) { fprintf(stderr, "accepted: %s\n", text); return 2; }
    if (!strstr(gaz_engine_last_error(h), text)) return fail(text);
    int32_t n = -1, m = -1;
    if (gaz_engine_get_opening_book(h, &n, &m) || n != n_before || m != mode_before) return fail("a refused call changed the book in force");
    return 0;
}

int main(int argc, char** argv) {
    std::map<std::string, std::string> kv = {{"game", "Connect4"}, {"n_games", "6"}, {"run_iterations", "16"}, {"max_actions", "42"}, {"seed", "3"}, {"mode", "1"},
        {"gumbel", "0"}, {"game_groups", "1"}};
    for (int i = 1; i < argc; ++i) {
        const char* eq = strchr(argv[i], '=');
        const std::string key(argv[i], eq ? (size_t)(eq - argv[i]) : 0);
        if (!eq || !kv.count(key)) { fprintf(stderr, "unknown argument %s\n", argv[i]); return 2; }
        kv[key] = eq + 1;
    }
    auto num = [&](const char* k) { return atoll(kv[k].c_str()); };
    const bool ttt = kv["game"] == "TicTacToe", gmk = kv["game"] == "Gomoku";
    gaz_engine_config c;
    memset(&c, 0, sizeof(c));
    c.struct_size = sizeof(c);
    c.game = ttt ? GAZ_GAME_TICTACTOE : (gmk ? GAZ_GAME_GOMOKU : GAZ_GAME_CONNECT4);
    c.search = num("gumbel") ? GAZ_SEARCH_GUMBEL : GAZ_SEARCH_PUCT;
    c.n_games = (int32_t)num("n_games"); c.run_iterations = (int32_t)num("run_iterations"); c.max_actions = ttt ? 9 : (int32_t)num("max_actions");
    c.num_explore_actions_first = 3; c.num_explore_actions_second = 2;
    c.c_puct_init = 2.5; c.c_puct_base = 19652.0; c.dirichlet_alpha = 0.5; c.dirichlet_epsilon = 0.25; c.use_dirichlet = 1;
    const long long games = 3LL * c.n_games;
    c.ring_capacity = (int32_t)games + 4;
    c.seed = (uint64_t)num("seed"); c.hash_salt = 6; c.evaluator = GAZ_EVAL_HASH; c.net_filters = 128;
    c.gumbel_m = num("gumbel") ? 4 : 0; c.c_visit = 50.0; c.c_scale = 1.0; c.games_budget = games; c.tau = -1.0; c.leaf_batch = 1; c.gumbel_batch = 1;
    c.game_groups = (int32_t)num("game_groups");
    const int mode = (int)num("mode");

    Book book;
    if (ttt) book = {{}, {4}, {0, 1, 2, 4, 3, 5, 7, 6}};
    else if (gmk) {
        // n legal plies that leave Gomoku running: the stones follow the colouring ((x + 2 y) % 4) / 2 of the board, in raster order
        std::vector<int> cells[2];
        for (int y = 0; y < 15; ++y) for (int x = 0; x < 15; ++x) cells[((x + 2 * y) % 4) / 2].push_back(y * 15 + x);
        for (int n : {66, 68, 70}) { std::vector<int> e; for (int i = 0; i < n; ++i) e.push_back(cells[i % 2][i / 2]); book.push_back(e); }
    } else book = {{}, {3}, {0, 0, 0, 0, 0, 0}, {0, 1, 0, 1, 2, 3, 2, 3, 4, 5, 4, 5, 6, 0, 6, 1, 2, 3}, {3, 3, 2, 4, 2}};

    if (gaz_engine_create(&c, &h)) { fprintf(stderr, "create: %s\n", gaz_engine_last_error(nullptr)); return 2; }
    gaz_record_layout lay;
    gaz_sample_layout sl;
    if (gaz_engine_record_layout(h, &lay) || gaz_engine_sample_layout(h, &sl)) return fail("layouts");

    // ---- refusals, on an engine without a book and then with one
    const Book one = ttt ? Book{{4}} : (gmk ? Book{{112}} : Book{{3}});
    for (int round = 0; round < 2; ++round) {
        const int nb = round ? (int)one.size() : 0, mb = round ? 2 : 0;
        if (round && set_book(one, 2)) return fail("set_opening_book");
        if (refused(set_book(one, 1, 0, 8), "struct_size", nb, mb)) return 2;
        if (refused(set_book(one, 3), "mode must be 0", nb, mb)) return 2;
        if (refused(set_book(one, 1, 0, sizeof(gaz_book_params), -1), "n_entries must be in", nb, mb)) return 2;
        if (refused(set_book(one, 1, 0, sizeof(gaz_book_params), (1 << 20) + 1), "n_entries must be in", nb, mb)) return 2;
        if (refused(set_book(one, 1, lay.max_T + 1), "stride must be in", nb, mb)) return 2;
        if (refused(set_book(Book{{1, 2, 3}}, 1, 2), "is outside [0, stride = 2]", nb, mb)) return 2;
        if (refused(set_book(one, 1, 0, sizeof(gaz_book_params), -2, true), "must not be null", nb, mb)) return 2;
        if (refused(gaz_engine_set_opening_book(h, nullptr, nullptr, nullptr), "null argument", nb, mb)) return 2;
        if (refused(set_book(Book{{}, {1, 1}, {250}}, 1), gmk || ttt ? "entry 1: illegal move 1 at ply 1" : "entry 2: illegal move 250 at ply 0", nb, mb)) return 2;
        if (ttt && refused(set_book(Book{{0, 3, 1, 4, 2}}, 1), "entry 0: the game is over after ply 4", nb, mb)) return 2;
        if (!ttt && !gmk && refused(set_book(Book{{0, 1, 0, 1, 0, 1, 0}}, 1), "entry 0: the game is over after ply 6", nb, mb)) return 2;
        if (gmk && refused(set_book(Book{{0, 15, 1, 16, 2, 17, 3, 18, 4}}, 1), "entry 0: the game is over after ply 8", nb, mb)) return 2;
        std::vector<int> too_long;
        for (int i = 0; i < c.max_actions; ++i) too_long.push_back(gmk ? i : (ttt ? i : i % 7));
        if (c.max_actions <= lay.max_T && refused(set_book(Book{too_long}, 1), "leaves no move below max_actions", nb, mb)) return 2;
    }

    // ---- the book, three games per slot
    if (set_book(book, mode)) return fail("set_opening_book");
    int32_t n_in = -1, m_in = -1;
    if (gaz_engine_get_opening_book(h, &n_in, &m_in) || n_in != (int)book.size() || m_in != mode) return fail("get_opening_book");
    uint64_t st[16];
    for (long long launches = 0;; ++launches) {
        if (gaz_engine_run_waves(h, 16) || gaz_engine_get_stats(h, st)) return fail("run_waves");
        if ((long long)st[2] >= games) break;
        if (launches > 1000000) return fail("the games did not finish");
    }
    std::set<std::pair<int, int>> handed;
    std::map<std::pair<int, int>, int> entry_of;     // (slot, game_seq >> 1) -> entry, mode 2
    // half of the games as records
    const int half = (int)(games / 2);
    std::vector<uint8_t> recs((size_t)half * lay.record_bytes);
    int32_t got = 0;
    if (gaz_engine_drain_finished(h, recs.data(), half, &got) || got != half) return fail("drain_finished");
    long long prefix_plies_seen = 0;
    for (int i = 0; i < got; ++i) {
        const uint8_t* r = recs.data() + (size_t)i * lay.record_bytes;
        int32_t hdr[4]; memcpy(hdr, r + lay.off_hdr, 16);
        if (!handed.insert({hdr[2], hdr[3]}).second) return fail("a game was handed out twice");
        int n = 0;
        while (n < hdr[0] && (r[lay.off_move_kind + n] & 3) == 3) ++n;
        for (int p = n; p < hdr[0]; ++p) if ((r[lay.off_move_kind + p] & 3) != 1) return fail("a searched ply is not kind 1");
        int which = -1;
        for (size_t e = 0; e < book.size(); ++e) {
            if ((int)book[e].size() != n) continue;
            bool same = true;
            for (int p = 0; p < n; ++p) same = same && r[lay.off_actions + p] == book[e][p];
            if (same) which = (int)e;
        }
        if (which < 0) return fail("a record's prefix is no entry of the book");
        for (int p = 0; p < n; ++p) {
            float q; uint32_t rv; memcpy(&q, r + lay.off_q + 4 * p, 4); memcpy(&rv, r + lay.off_root_visits + 4 * p, 4);
            if (q != 0.0f || rv != 0u) return fail("a prefix row is not zero");
            for (int a = 0; a < lay.A; ++a) { uint32_t w; memcpy(&w, r + lay.off_policy + 4 * ((size_t)p * lay.A + a), 4); if (w) return fail("a prefix policy row is not zero"); }
        }
        if (mode == 2) {
            auto key = std::make_pair((int)hdr[2], (int)((uint32_t)hdr[3] >> 1));
            if (entry_of.count(key) && entry_of[key] != which && book[entry_of[key]] != book[which]) return fail("the two games of a pair start from different entries");
            entry_of[key] = which;
        }
        prefix_plies_seen += n;
    }
    // the rest as samples, buffers of exactly the documented sizes
    const long long rest = games - half, max_rows = rest * sl.max_T;
    std::vector<int32_t> g6((size_t)6 * rest);
    std::vector<int8_t> boards((size_t)sl.n_aug * max_rows * sl.state_bytes);
    std::vector<float> policies((size_t)sl.n_aug * max_rows * sl.A), values((size_t)max_rows);
    std::vector<uint8_t> plies((size_t)max_rows);
    int32_t ng = 0; int64_t R = 0;
    if (gaz_engine_drain_samples2(h, (int32_t)rest, max_rows, g6.data(), boards.data(), policies.data(), values.data(), plies.data(), &ng, &R) || ng != rest) return fail("drain_samples2");
    long long left_out = 0;
    for (int i = 0; i < ng; ++i) {
        const int32_t* g = &g6[(size_t)6 * i];
        const long long r0 = g[4], r1 = i + 1 < ng ? g6[(size_t)6 * (i + 1) + 4] : R;
        if (!handed.insert({g[2], g[3]}).second) return fail("a game was handed out twice");
        if (r1 - r0 != g[0] - g[5] || g[5] < 0 || r1 - r0 < 1) return fail("a game's rows are not T minus the plies left out");
        if (plies[r0] != g[5]) return fail("the first row of a game is not its first searched ply");      // (cap off: only the prefix is left out)
        left_out += g[5];
    }
    // ---- the counters, into a block of exactly n_entries words
    std::vector<uint64_t> counts(book.size());
    uint64_t out[8];
    if (gaz_engine_read_book_counts(h, counts.data(), out)) return fail("read_book_counts");
    uint64_t sum = 0, plies_want = 0;
    for (size_t e = 0; e < book.size(); ++e) { sum += counts[e]; plies_want += counts[e] * book[e].size(); }
    if (sum != (uint64_t)games || out[0] != (uint64_t)games || out[1] != plies_want || out[2] || out[7]) return fail("the counters do not add up");
    if ((long long)plies_want != prefix_plies_seen + left_out) return fail("the prefix plies of the games are not the counters'");
    if (gaz_engine_read_book_counts(h, nullptr, out) == 0) return fail("read_book_counts(NULL) with a book in force was not refused");
    // ---- removal
    gaz_book_params off; off.struct_size = sizeof(off); off.n_entries = 0; off.stride = 0; off.mode = 0;
    if (gaz_engine_set_opening_book(h, &off, nullptr, nullptr)) return fail("removing the book");
    if (gaz_engine_get_opening_book(h, &n_in, &m_in) || n_in != 0 || m_in != 0) return fail("get_opening_book after the removal");
    if (gaz_engine_read_book_counts(h, nullptr, out) || out[0] != (uint64_t)games) return fail("read_book_counts after the removal");
    printf("%lld games, %llu prefix plies, counts", games, (unsigned long long)plies_want);
    for (uint64_t cnt : counts) printf(" %llu", (unsigned long long)cnt);
    printf("\n");
    gaz_engine_destroy(h);
    return (long long)handed.size() == games ? 0 : 2;
}
