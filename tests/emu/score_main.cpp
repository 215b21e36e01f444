// CPU test build only (tests/score_cases.py build_driver): a program of its own around the engine's host code and the one-lane build of its
// device code, so that the held-out loss (gaz_engine_score_outputs / gaz_engine_score_replay) runs under -fsanitize=address,undefined with caller
// buffers that are exactly as large as the header says they must be — a library loaded into Python cannot.
// score_outputs: n = 0, 1, 2, 7, 127, 128, 129, 257 rows under all four modes (and -1), heap blocks of exactly n * A floats / n floats / n doubles /
// n bytes, rows with NaN and inf among them, per-row outputs present and NULL.  score_replay: a tiny window scored by the hash evaluator at batch
// sizes 1, 3 and the engine's whole batch, with and without augmentation.  Checked here: the counts add up, bad rows carry zeros, the totals do
// not depend on the batch size, and the refusals at the limits.
//   score_asan game=0|1|2       exit status 0 = every check held, 2 = anything else.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../include/gaz_engine.h"

static gaz_engine* h = nullptr;
static int fail(const char* what) { fprintf(stderr, "%s: %s\n", what, gaz_engine_last_error(h)); return 2; }

int main(int argc, char** argv) {
    int game = 1;
    for (int i = 1; i < argc; ++i) {
        if (strncmp(argv[i], "game=", 5) != 0) { fprintf(stderr, "unknown argument %s\n", argv[i]); return 2; }
        game = atoi(argv[i] + 5);
    }
    static const int dims[3][3] = {{18, 9, 9}, {168, 7, 42}, {450, 225, 225}};            // state bytes, actions, longest game
    const int SB = dims[game][0], A = dims[game][1];

    gaz_engine_config c;
    memset(&c, 0, sizeof(c));
    c.struct_size = sizeof(c); c.game = game; c.n_games = 8; c.run_iterations = 8; c.max_actions = dims[game][2]; c.c_puct_init = 2.5; c.c_puct_base = 19652.0;
    c.dirichlet_alpha = 0.5; c.dirichlet_epsilon = 0.25; c.seed = 3; c.evaluator = GAZ_EVAL_HASH; c.hash_salt = 6; c.game_groups = 1; c.nodes_per_tree = 64;
    if (gaz_engine_create(&c, &h)) { fprintf(stderr, "create: %s\n", gaz_engine_last_error(nullptr)); return 2; }

    unsigned rng = 777u + (unsigned)game;
    auto next = [&]() { rng = rng * 1664525u + 1013904223u; return rng >> 8; };
    auto unit = [&]() { return (float)(next() & 0xFFFF) / 65536.0f; };

    // ---- gaz_engine_score_outputs
    const int sizes[] = {0, 1, 2, 7, 127, 128, 129, 257};
    for (int n : sizes) for (int mode = -1; mode <= 3; ++mode) for (int per_row = 0; per_row < 2; ++per_row) {
        float* pp = new float[(size_t)n * A]; float* tp = new float[(size_t)n * A]; float* pv = new float[n]; float* tv = new float[n];
        int bad = 0;
        for (int r = 0; r < n; ++r) {
            float sum = 0.f;
            for (int a = 0; a < A; ++a) { pp[(size_t)r * A + a] = (mode == 1 || mode == 3) ? unit() * 40.f - 20.f : unit(); tp[(size_t)r * A + a] = (next() & 3) ? unit() : 0.f; sum += tp[(size_t)r * A + a]; }
            for (int a = 0; a < A; ++a) tp[(size_t)r * A + a] = sum > 0.f ? tp[(size_t)r * A + a] / sum : 0.f;
            pv[r] = unit() * 2.f - 1.f; tv[r] = (float)((int)(next() % 3) - 1);
            if (r % 11 == 3) { pp[(size_t)r * A + (next() % A)] = (r & 1) ? NAN : INFINITY; ++bad; }
            else if (r % 13 == 5) { pv[r] = (r & 1) ? -INFINITY : NAN; ++bad; }
        }
        double* ce = per_row ? new double[n] : nullptr; double* en = per_row ? new double[n] : nullptr; double* se = per_row ? new double[n] : nullptr;
        uint8_t* fl = per_row ? new uint8_t[n] : nullptr;
        gaz_score_totals t; memset(&t, 0xAB, sizeof(t)); t.struct_size = sizeof(t);
        if (gaz_engine_score_outputs(h, pp, pv, tp, tv, n, mode, &t, ce, en, se, fl)) return fail("score_outputs");
        if (t.rows != n || t.bad_rows != bad || t.top1 > n - bad || t.value_sign > t.value_rows || t.value_rows > n - bad || t.policy_mode != (mode < 0 ? 0 : mode)) {
            fprintf(stderr, "score_outputs n %d mode %d: counts rows %lld bad %lld (want %d)\n", n, mode, (long long)t.rows, (long long)t.bad_rows, bad); return 2;
        }
        if (!(std::isfinite(t.ce_sum) && std::isfinite(t.entropy_sum) && std::isfinite(t.se_sum))) { fprintf(stderr, "score_outputs n %d mode %d: a sum is not finite\n", n, mode); return 2; }
        for (int r = 0; per_row && r < n; ++r) {
            const bool b = (fl[r] & 8) != 0;
            if (b != (r % 11 == 3 || r % 13 == 5) || (b && (fl[r] != 8 || ce[r] != 0.0 || en[r] != 0.0 || se[r] != 0.0)) || !std::isfinite(ce[r])) { fprintf(stderr, "score_outputs n %d mode %d row %d\n", n, mode, r); return 2; }
        }
        delete[] pp; delete[] tp; delete[] pv; delete[] tv; delete[] ce; delete[] en; delete[] se; delete[] fl;
    }
    gaz_score_totals stale; memset(&stale, 0, sizeof(stale)); stale.struct_size = sizeof(stale) - 8;
    if (gaz_engine_score_outputs(h, nullptr, nullptr, nullptr, nullptr, 0, 0, &stale, nullptr, nullptr, nullptr, nullptr) == 0 || !strstr(gaz_engine_last_error(h), "struct_size"))
        return fail("a stale struct_size was not refused");

    // ---- gaz_engine_score_replay on a tiny window
    gaz_replay_config rc; memset(&rc, 0, sizeof(rc));
    rc.struct_size = sizeof(rc); rc.game = game; rc.capacity_rows = 37; rc.seed = 5; rc.test_fraction = 0.0; rc.target_ratio = NAN;
    gaz_replay* w = nullptr;
    if (gaz_replay_create(&rc, &w)) { fprintf(stderr, "replay_create: %s\n", gaz_replay_last_error(nullptr)); return 2; }
    gaz_score_totals t; memset(&t, 0, sizeof(t)); t.struct_size = sizeof(t);
    if (gaz_engine_score_replay(h, w, 4, 0, &t, nullptr, nullptr, nullptr, nullptr, nullptr) == 0 || !strstr(gaz_engine_last_error(h), "no plan")) return fail("a window without a plan was scored");
    const int R = 29;
    const int32_t games[3][6] = {{9, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 9, 0}, {20, 0, 0, 0, 9, 0}};
    {
        std::vector<int8_t> boards((size_t)R * SB); std::vector<float> pol((size_t)R * A), val((size_t)R);
        for (auto& b : boards) b = (int8_t)(next() % 3) - 1;
        for (int r = 0; r < R; ++r) {
            float sum = 0.f;
            for (int a = 0; a < A; ++a) { pol[(size_t)r * A + a] = (next() & 1) ? unit() + 0.01f : 0.f; sum += pol[(size_t)r * A + a]; }
            for (int a = 0; a < A; ++a) pol[(size_t)r * A + a] = sum > 0.f ? pol[(size_t)r * A + a] / sum : 0.f;
            val[r] = (float)((int)(next() % 3) - 1);
        }
        if (gaz_replay_append(w, 0, 3, &games[0][0], boards.data(), pol.data(), val.data(), R)) { fprintf(stderr, "append: %s\n", gaz_replay_last_error(w)); return 2; }
    }
    int64_t M = 0;
    if (gaz_replay_begin_epoch(w, 0, 1, 0, 1.0, 0.0, &M) || M != R) { fprintf(stderr, "begin_epoch: %s\n", gaz_replay_last_error(w)); return 2; }
    for (int augment = 0; augment < 2; ++augment) {
        gaz_score_totals first; memset(&first, 0, sizeof(first));
        const int batches[] = {1, 3, 8};
        for (int bi = 0; bi < 3; ++bi) {
            double* ce = new double[R]; double* en = new double[R]; double* se = new double[R]; uint8_t* fl = new uint8_t[R];
            double ms = -1.0;
            memset(&t, 0xCD, sizeof(t)); t.struct_size = sizeof(t);
            if (gaz_engine_score_replay(h, w, batches[bi], augment, &t, ce, en, se, fl, &ms)) return fail("score_replay");
            if (t.rows != R || t.bad_rows != 0 || !std::isfinite(t.ce_sum) || !(t.se_sum >= 0.0) || ms < 0.0) { fprintf(stderr, "score_replay: totals\n"); return 2; }
            if (bi == 0) first = t;
            else if (memcmp(&first, &t, sizeof(t)) != 0) { fprintf(stderr, "score_replay: the totals depend on batch_rows (%d)\n", batches[bi]); return 2; }
            for (int r = 0; r < R; ++r) if ((fl[r] & 8) || !std::isfinite(ce[r]) || !(se[r] >= 0.0)) { fprintf(stderr, "score_replay row %d\n", r); return 2; }
            delete[] ce; delete[] en; delete[] se; delete[] fl;
        }
    }
    memset(&t, 0, sizeof(t)); t.struct_size = sizeof(t);
    if (gaz_engine_score_replay(h, w, 0, 0, &t, nullptr, nullptr, nullptr, nullptr, nullptr) == 0 || !strstr(gaz_engine_last_error(h), "batch_rows must be in [1, 8]")) return fail("batch_rows 0 was accepted");
    if (gaz_engine_score_replay(h, w, 9, 0, &t, nullptr, nullptr, nullptr, nullptr, nullptr) == 0 || !strstr(gaz_engine_last_error(h), "batch_rows must be in [1, 8]")) return fail("batch_rows 9 was accepted");
    if (gaz_replay_begin_epoch(w, 1, 0, 0, 1.0, 0.0, &M) || M != 0) { fprintf(stderr, "begin_epoch (test): %s\n", gaz_replay_last_error(w)); return 2; }
    if (gaz_engine_score_replay(h, w, 8, 1, &t, nullptr, nullptr, nullptr, nullptr, nullptr) || t.rows != 0 || t.ce_sum != 0.0) return fail("an empty plan");
    double ms = 0.0;
    if (gaz_engine_score_rows_timed(h, 2, &ms)) return fail("score_rows_timed");
    gaz_replay_destroy(w);
    gaz_engine_destroy(h);
    printf("ok\n");
    return 0;
}
