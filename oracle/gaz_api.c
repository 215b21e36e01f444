/*
 * ORACLE — TEST INFRASTRUCTURE ONLY (see gaz_det.h header).
 * gaz_api.c — flat entry points for ctypes (tests, fixture generator): the injected
 * noise stream and the numeric helpers, so Python draws exactly what the C oracle draws.
 */
#include "gaz_det.h"
#include "gaz_games.h"
#include "gaz_puct.h"

static gaz_event mk(uint64_t seed, uint32_t slot, uint32_t seq, uint32_t tree, uint32_t event, uint32_t purpose) {
    gaz_event e; e.key[0] = (uint32_t)seed; e.key[1] = (uint32_t)(seed >> 32);
    e.slot = slot; e.game_seq = seq; e.event = event; e.tree = tree; e.purpose = purpose; return e;
}
void gaz_api_dirichlet(uint64_t seed, uint32_t slot, uint32_t seq, uint32_t tree, uint32_t event, double alpha, int n, double* out) {
    gaz_event e = mk(seed, slot, seq, tree, event, GAZ_P_DIRICHLET); gaz_dirichlet(&e, alpha, n, out);
}
uint32_t gaz_api_pick(uint64_t seed, uint32_t slot, uint32_t seq, uint32_t tree, uint32_t event, uint32_t n) {
    gaz_event e = mk(seed, slot, seq, tree, event, GAZ_P_TERMINAL_PICK); return gaz_pick(&e, n);
}
double gaz_api_uniform(uint64_t seed, uint32_t slot, uint32_t seq, uint32_t tree, uint32_t event, uint32_t purpose) {
    gaz_event e = mk(seed, slot, seq, tree, event, purpose); return gaz_uniform(&e);
}
void gaz_api_gumbel(uint64_t seed, uint32_t slot, uint32_t seq, uint32_t tree, uint32_t event, int n, double* out) {
    gaz_event e = mk(seed, slot, seq, tree, event, GAZ_P_GUMBEL);
    for (int i = 0; i < n; ++i) out[i] = gaz_gumbel(&e, (uint32_t)i);
}
void gaz_api_philox(const uint32_t* ctr, const uint32_t* key, uint32_t* out) { gaz_philox(ctr, key, out); }
double gaz_api_log(double x) { return gaz_log(x); }
double gaz_api_exp(double x) { return gaz_exp(x); }
/* the rest of the det math, one call per function, for the det probe's cases (tests/det_cases.py).  The Gumbel entry points
 * (gaz_api_softmax, _compute_pi, _compute_pi_stable, _det_select) wrap functions static to gaz_gumbel.c and sit at its end. */
double gaz_api_pow(double x, double y) { return gaz_pow(x, y); }
double gaz_api_sqrt(double x) { return gaz_sqrt(x); }
void gaz_api_draw(uint64_t seed, uint32_t slot, uint32_t seq, uint32_t tree, uint32_t event, uint32_t purpose, uint32_t lane, uint32_t attempt, uint32_t* out) {
    gaz_event e = mk(seed, slot, seq, tree, event, purpose); gaz_draw(&e, lane, attempt, out);
}
uint64_t gaz_api_k52(uint32_t a, uint32_t b) { return gaz_k52(a, b); }
double gaz_api_u_open(uint32_t a, uint32_t b) { return gaz_u_open(a, b); }
double gaz_api_u_half(uint32_t a, uint32_t b) { return gaz_u_half(a, b); }
uint32_t gaz_api_pick_p(uint64_t seed, uint32_t slot, uint32_t seq, uint32_t tree, uint32_t event, uint32_t purpose, uint32_t n) {
    gaz_event e = mk(seed, slot, seq, tree, event, purpose); return gaz_pick(&e, n);
}
double gaz_api_gumbel_p(uint64_t seed, uint32_t slot, uint32_t seq, uint32_t tree, uint32_t event, uint32_t purpose, uint32_t lane) {
    gaz_event e = mk(seed, slot, seq, tree, event, purpose); return gaz_gumbel(&e, lane);
}
/* *draws: the Philox draws the variate consumed (the attempt counter starts at 0) */
double gaz_api_normal(uint64_t seed, uint32_t slot, uint32_t seq, uint32_t tree, uint32_t event, uint32_t purpose, uint32_t lane, uint32_t* draws) {
    gaz_event e = mk(seed, slot, seq, tree, event, purpose); uint32_t attempt = 0;
    double v = gaz_normal(&e, lane, &attempt); *draws = attempt; return v;
}
/* *test: 1 = the squeeze accepted, 2 = the log test */
double gaz_api_gamma(uint64_t seed, uint32_t slot, uint32_t seq, uint32_t tree, uint32_t event, uint32_t purpose, uint32_t lane, double alpha,
                     uint32_t* draws, int* test) {
    gaz_event e = mk(seed, slot, seq, tree, event, purpose); return gaz_gamma_info(&e, lane, alpha, draws, test);
}
void gaz_api_puct_factors(uint64_t parent_visits, double c_init, double c_base, double* s, double* c) { gaz_puct_factors(parent_visits, c_init, c_base, 0, s, c); }
int gaz_api_puct_scores(const float* priors, const float* values, const uint32_t* visits, int n, double s, double c, double* scores) {
    return gaz_puct_scores(priors, values, visits, n, s, c, scores);
}
float gaz_api_np_sum_f32(const float* a, int n) { return gaz_np_sum_f32(a, n); }
double gaz_api_np_sum_f64(const double* a, int n) { return gaz_np_sum_f64(a, n); }

/* game rule entry points for the Game_Tester-style fixtures */
int gaz_api_legal_actions(int game, const int8_t* board, int* out) { gaz_game_desc g = gaz_game(game); return gaz_legal_actions(&g, board, out); }
void gaz_api_do_action(int game, int8_t* board, int action, int player) { gaz_game_desc g = gaz_game(game); gaz_do_action(&g, board, action, player); }
int gaz_api_check_win(int game, const int8_t* board, int player, int last_action) { gaz_game_desc g = gaz_game(game); return gaz_check_win(&g, board, player, last_action); }
void gaz_api_input_state(int game, const int8_t* board, int current_player, const int* hist, int n_hist, int8_t* out) {
    gaz_game_desc g = gaz_game(game); gaz_input_state(&g, board, current_player, hist, n_hist, out);
}
