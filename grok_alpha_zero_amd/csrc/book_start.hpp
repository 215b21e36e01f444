// book_start.hpp — the two kernels of the opening book (book.hpp): validation of a table at gaz_engine_set_opening_book, and the start of the
// games that wait in PH_NEW_GAME, launched in front of every tree step while a book is set.
#pragma once
#include "book.hpp"
#include "puct_core.hpp"

namespace gaz {

// cell of ply i of a legal action sequence (Connect4: the landing row follows from the earlier moves in the column, as in samples.hpp)
template <class G> GAZ_DEV int book_cell(const uint8_t* a, int i) {
    if (G::ID == GAME_C4) {
        int below = 0;
        for (int e = 0; e < i; ++e) below += a[e] == a[i];
        return (G::H - 1 - below) * G::W + a[i];
    }
    return a[i];
}

// Validation (gaz_engine_set_opening_book): one team per entry replays it with the rules the search uses.  status[i] = 0 = the entry can start a
// game; else (ply << 8) | reason: BOOK_BAD_ILLEGAL at the first illegal ply (an action index out of range included), BOOK_BAD_OVER at the first
// ply after which the game is won or drawn (its last ply included: a game must have a move to search), BOOK_BAD_LONG for a length that leaves
// no move below max_actions.  Lengths outside [0, stride] never get here (the host refuses them first); they are clamped all the same.
enum : int32_t { BOOK_OK = 0, BOOK_BAD_ILLEGAL = 1, BOOK_BAD_OVER = 2, BOOK_BAD_LONG = 3 };
template <class G> GAZ_KERNEL_TEAMS k_book_validate(const uint8_t* actions, const int32_t* lengths, int n_entries, int stride, int max_actions, int32_t* status) {
    constexpr int PER = WAVE / G::TEAM;
    GAZ_SHARED int8_t boards[PER][G::BPAD];
    const int i = block_id() * PER + team_in_wave<G>();
    if (i >= n_entries) return;
    int8_t* board = boards[team_in_wave<G>()];
    int n = lengths[i];
    n = n < 0 ? 0 : (n > stride ? stride : (n > G::MAXT ? G::MAXT : n));
    const uint8_t* a = actions + (size_t)i * stride;
    for (int c = tlane<G>(); c < G::BPAD; c += G::TEAM) board[c] = 0;
    wave_sync();
    int st = n >= max_actions ? ((n << 8) | BOOK_BAD_LONG) : BOOK_OK;
    int player = -1;
    for (int p = 0; p < n && st == BOOK_OK; ++p) {
        const int act = a[p];
        if (act >= G::A || !action_legal<G>(board, act)) { st = (p << 8) | BOOK_BAD_ILLEGAL; break; }
        const int cell = landing_cell<G>(board, act);
        const bool win = wins_after<G>(board, cell, player);
        const int empties = G::DRAWS ? count_empty<G>(board) : 2;
        if (win || (G::DRAWS && empties == 1)) st = (p << 8) | BOOK_BAD_OVER;
        wave_sync();
        if (tlane<G>() == 0) board[cell] = (int8_t)player;
        wave_sync();
        player = -player;
    }
    if (tlane<G>() == 0) status[i] = st;
}

// The start: every game of [g0, g1) that WAITS — in PH_NEW_GAME (a new engine, gaz_engine_reset_games), or parked in PH_HALT by the budget of
// 1 the tree steps run under while a book is set (book.hpp) with its next game within the TRUE budget, E.games_budget here — becomes what
// k_set_position(entry, n) makes of a slot: the prefix on the board, hist / n_hist / next_player following from it, both trees fresh with event
// counter 0, roots_todo as k_set_position sets it — and what PH_NEW_GAME makes of it besides (winner, host_move, move_evals, cap_state).  The
// record carries the prefix in actions[0, n), zeros in every per-move field of rows [0, n) and MK_BOOK in move_kind[0, n).  With n = 0 this is
// PH_NEW_GAME's own start, word for word.  Without a book (it was just removed) the parked slots go on to PH_NEW_GAME instead.
template <class G> GAZ_DEV bool book_game_waits(const DevParams<G>& E, const GameState<G>& gs) {
    if (gs.phase == PH_NEW_GAME) return true;
    if (gs.phase != PH_HALT || E.sync_moves) return false;               // (sync mode: a finished game halts until the host resets it)
    const long long k = (long long)(gs.game_seq - E.first_game_seq);     // ring_push's rule, with the true budget
    return !(E.games_budget > 0 && k * (long long)E.n_games + (long long)(gs.slot_id - E.slot_offset) >= E.games_budget);
}
template <class G> GAZ_KERNEL_TEAMS k_book_start(DevParams<G> E, int g0, int g1) {
    using RL = RecLayout<G>;
    constexpr int PER = WAVE / G::TEAM;
    const int g = g0 + block_id() * PER + team_in_wave<G>();
    if (g >= g1 || g >= E.n_games) return;
    GameState<G>& gs = E.games[g];
    if (!book_game_waits<G>(E, gs)) return;
    BookBlock* bk = book_block(E.stats);
    const int ne = bk->n_entries;
    if (ne <= 0) {                                    // the book was removed: the tree step starts the game on the empty board
        wave_sync();
        if (tlane<G>() == 0) gs.phase = PH_NEW_GAME;
        return;
    }
    const int idx = book_draw(E.key0, E.key1, gs.slot_id, gs.game_seq, bk->mode, ne);
    int n = bk->lengths[idx];
    n = n < 0 ? 0 : (n > bk->stride ? bk->stride : (n >= G::MAXT ? G::MAXT - 1 : n));      // (validated at set time; a table is data all the same)
    const uint8_t* a = bk->actions + (size_t)idx * bk->stride;
    uint8_t* rec = E.recs + (size_t)g * RL::SIZE;
    {
        uint32_t* q = reinterpret_cast<uint32_t*>(rec + RL::OFF_Q); uint32_t* rv = reinterpret_cast<uint32_t*>(rec + RL::OFF_RV);
        uint32_t* ev = reinterpret_cast<uint32_t*>(rec + RL::OFF_EV);
        for (int i = tlane<G>(); i < n; i += G::TEAM) { q[i] = 0u; rv[i] = 0u; ev[i] = 0u; rec[RL::OFF_MK + i] = MK_BOOK; rec[RL::OFF_ACT + i] = a[i]; }
        uint32_t* pol = reinterpret_cast<uint32_t*>(rec + RL::OFF_POL); uint32_t* nn = reinterpret_cast<uint32_t*>(rec + RL::OFF_N);
        uint32_t* w = reinterpret_cast<uint32_t*>(rec + RL::OFF_W); uint32_t* p = reinterpret_cast<uint32_t*>(rec + RL::OFF_P);
        for (int i = tlane<G>(); i < n * G::A; i += G::TEAM) { pol[i] = 0u; nn[i] = 0u; w[i] = 0u; p[i] = 0u; }
    }
    for (int c = tlane<G>(); c < G::BPAD; c += G::TEAM) gs.board[c] = 0;
    wave_sync();
    for (int i = tlane<G>(); i < n; i += G::TEAM) {   // a validated prefix: no two plies share a cell
        const int cell = book_cell<G>(a, i);
        if (cell >= 0 && cell < G::HW) gs.board[cell] = (int8_t)((i & 1) ? 1 : -1);
        gs.hist[i] = a[i];
    }
    wave_sync();
    if (tlane<G>() == 0) {
        gs.n_hist = n; gs.next_player = (n & 1) ? 1 : -1; gs.roots_todo = (E.single_tree || E.gstate) ? 1 : 3; gs.phase = PH_ROOT; gs.winner = RUNNING;
        gs.host_move = -1; gs.move_evals = 0; gs.cap_state = 0;
        for (int t = 0; t < 2; ++t) { TreeState& ts = E.trees[(size_t)g * 2 + t]; ts.root = -1; ts.event = 0; ts.n_nodes = 0; ts.root_visits = 0; }
        atomic_add(&bk->counts[idx], 1ull);
        atomic_add(&bk->started, 1ull);
        if (n) atomic_add(&bk->plies, (unsigned long long)n);
    }
}

}  // namespace gaz
