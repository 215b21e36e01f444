// engine.hip — host side of libgaz_engine.so: owns the HBM state, launches the wave kernel + evaluator
// once per simulation wave on one HIP stream, and implements the C ABI of include/gaz_engine.h.
#include <stdio.h>
#include <chrono>
#include <functional>
#include <string>
#include <vector>
#include "../../include/gaz_engine.h"
#include "rt.hpp"
#include "puct_core.hpp"
#include "gumbel_core.hpp"
#include "samples.hpp"
#include "book_start.hpp"
#include "tree_export.hpp"
#include "evaluator.hpp"
#include "match.hpp"
#include "det_probe.hpp"
#include "replay.hpp"
#include "score.hpp"
#include "optim.hpp"

using namespace gaz;

static std::string g_create_error;

#define HIP_OK(expr)                                                                  \
    do { hipError_t _e = (expr); if (_e != hipSuccess) { return fail(std::string(#expr) + ": " + hipGetErrorString(_e)); } } while (0)

// ------------------------------------------------------------------------------------------ kernels
// one TEAM of lanes per game of [g0, g1): a whole wavefront (Gomoku), or a 16-lane row — four games per wavefront (wave.hpp "Teams")
template <class G> GAZ_DEV void wave_body(const DevParams<G>& E, int g0, int g1) {
    constexpr int PER = WAVE / G::TEAM;
    GAZ_SHARED Scratch<G> S[PER];
    GAZ_SHARED PuctLocal<G> L[PER];
    const int t = team_in_wave<G>();
    const int g = g0 + block_id() * PER + t;
    if (g < g1) game_step<G>(E, g, S[t], L[t]);
}
template <class G> GAZ_KERNEL k_wave(DevParams<G> E, int g0, int g1) { wave_body<G>(E, g0, g1); }
template <class G> GAZ_KERNEL_TEAMS k_wave_teams(DevParams<G> E, int g0, int g1) { wave_body<G>(E, g0, g1); }

// leaf-batched PUCT search (gaz_engine_config::leaf_batch > 1): the same launch shapes, the K-leaf step of puct_core.hpp
template <class G> GAZ_DEV void wave_body_lb(const DevParams<G>& E, const LeafBatch& B, int g0, int g1) {
    constexpr int PER = WAVE / G::TEAM;
    GAZ_SHARED Scratch<G> S[PER];
    GAZ_SHARED PuctLocal<G> L[PER];
    const int t = team_in_wave<G>();
    const int g = g0 + block_id() * PER + t;
    if (g < g1) game_step_lb<G>(E, B, g, S[t], L[t]);
}
template <class G> GAZ_KERNEL_TEAMS k_wave_lb(DevParams<G> E, LeafBatch B, int g0, int g1) { wave_body_lb<G>(E, B, g0, g1); }

// gaz_engine_read_batch with leaf batching: pending[g * K + j] = the request in row g * K + j (0 = none)
template <class G> GAZ_KERNEL k_gather_pending_lb(DevParams<G> E, int K, int32_t* out) {
    const int g = block_id();
    if (g >= E.n_games) return;
    const GameState<G>& gs = E.games[g];
    const int n = gs.pend_kind == PEND_ROOT ? 1 : (gs.pend_kind == PEND_EXPAND ? gs.pend_depth : 0);
    for (int j = lane_id(); j < K; j += WAVE) out[(size_t)g * K + j] = j < n ? gs.pend_kind : PEND_NONE;
}

// gaz_engine_get_stats [15] with leaf batching: the reserved counts (NodeHdr::pad[0]) of every node record the trees have allocated, summed —
// 0 whenever no search is between two launches of a move (a move never ends with a leaf in flight)
template <class G> GAZ_KERNEL k_count_reserved(DevParams<G> E, unsigned long long* out) {
    const int g = block_id();
    if (g >= E.n_games) return;
    unsigned long long sum = 0;
    for (int t = 0; t < 2; ++t) {
        const int n = (int)E.trees[(size_t)g * 2 + t].n_nodes;
        for (int i = lane_id(); i < n; i += WAVE) sum += node_at(E, g, t, i).hdr()->pad[0];
    }
    if (sum) atomic_add(out, sum);
}

template <class G> GAZ_DEV void wave_body_gumbel(const DevParams<G>& E, int g0, int g1) {
    constexpr int PER = WAVE / G::TEAM;
    GAZ_SHARED Scratch<G> S[PER];
    GAZ_SHARED GumbelLocal<G> L[PER];
    const int t = team_in_wave<G>();
    const int g = g0 + block_id() * PER + t;
    if (g < g1) g_game_step<G>(E, g, S[t], L[t]);
}
template <class G> GAZ_KERNEL k_wave_gumbel(DevParams<G> E, int g0, int g1) { wave_body_gumbel<G>(E, g0, g1); }
template <class G> GAZ_KERNEL_TEAMS k_wave_gumbel_teams(DevParams<G> E, int g0, int g1) { wave_body_gumbel<G>(E, g0, g1); }

// batched sequential halving (gaz_engine_config::gumbel_batch > 1): the same launch shapes, the chunk step of gumbel_core.hpp
template <class G> GAZ_DEV void wave_body_gb(const DevParams<G>& E, const GumbelBatch& B, int g0, int g1) {
    constexpr int PER = WAVE / G::TEAM;
    GAZ_SHARED Scratch<G> S[PER];
    GAZ_SHARED GumbelLocal<G> L[PER];
    const int t = team_in_wave<G>();
    const int g = g0 + block_id() * PER + t;
    if (g < g1) g_game_step_gb<G>(E, B, g, S[t], L[t]);
}
template <class G> GAZ_KERNEL_TEAMS k_wave_gb(DevParams<G> E, GumbelBatch B, int g0, int g1) { wave_body_gb<G>(E, B, g0, g1); }

// gaz_engine_read_batch with gumbel_batch = K: pending[g * K + j] = the request in row g * K + j (0 = none).  Rows of a chunk can be idle
// while others wait (a candidate that used its visits, or whose visit ended at a terminal), so every row answers for itself
template <class G> GAZ_KERNEL k_gather_pending_gb(DevParams<G> E, GumbelBatch B, int32_t* out) {
    const int g = block_id();
    if (g >= E.n_games) return;
    const int kind = E.games[g].pend_kind;               // (PEND_NONE after a reset: stale rows of a game reset mid-move are not reported)
    for (int j = lane_id(); j < B.K; j += WAVE)
        out[(size_t)g * B.K + j] = kind == PEND_ROOT ? (j == 0 ? PEND_ROOT : PEND_NONE) : (kind == PEND_EXPAND && B.rows[(size_t)g * B.K + j].pend ? PEND_EXPAND : PEND_NONE);
}

// evaluation cache: store (state row, outputs) of every request the evaluator just answered; runs between the evaluator
// pass and the next tree launch, so the tree kernels only ever read the table
template <class G> GAZ_KERNEL k_cache_insert(DevParams<G> E, int g0, int g1) {
    const int g = g0 + block_id();
    if (g < g1) cache_insert<G>(E, g);
}

// sqrt(pv) and the exploration factor of every parent visit count below PUCT_TABLE_N, computed by the code the kernel would run
template <int UNUSED> GAZ_KERNEL_WIDE k_init_puct_table(double* table, double c_init, double c_base, int n) {
#ifdef GAZ_HOST_EMU
    const int i = block_id();
#else
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
#endif
    if (i < n) { table[2 * i] = dsqrt((double)i); table[2 * i + 1] = puct_c_of((double)i, c_init, c_base); }
}

template <class G> GAZ_KERNEL k_init_games(DevParams<G> E, int first_seq) {
    const int g = block_id();
    if (g >= E.n_games || lane_id() != 0) return;
    GameState<G>& gs = E.games[g];
    memset(&gs, 0, sizeof(gs));
    gs.phase = (E.games_budget > 0 && (long long)g >= E.games_budget) ? PH_HALT : PH_NEW_GAME;     // fewer games wanted than slots
    gs.pend_kind = PEND_NONE; gs.game_seq = (uint32_t)first_seq; gs.host_move = -1; gs.winner = RUNNING;
    gs.slot_id = E.slot_offset + (uint32_t)g;
    E.trees[g * 2].root = -1; E.trees[g * 2 + 1].root = -1;
}

template <class G> GAZ_KERNEL k_reset_games(DevParams<G> E, const int32_t* slots, int n) {
    const int i = block_id();
    if (i >= n || lane_id() != 0) return;
    const int g = slots ? slots[i] : i;
    if (g < 0 || g >= E.n_games) return;
    GameState<G>& gs = E.games[g];
    const uint32_t seq = gs.game_seq + ((gs.phase == PH_NEW_GAME && gs.n_evals == 0) ? 0u : 1u);
    const uint64_t ne = gs.n_evals, ns = gs.n_sims, np = gs.n_plies; const uint32_t sid = gs.slot_id;
    memset(&gs, 0, sizeof(gs));
    gs.phase = PH_NEW_GAME; gs.game_seq = seq; gs.host_move = -1; gs.winner = RUNNING; gs.n_evals = ne; gs.n_sims = ns; gs.n_plies = np; gs.slot_id = sid;
}

// put one slot at an arbitrary position (MCTS attaches to a live game object, MCTS.py:296-313): replay `n` actions on an empty
// board, then let the state machine build the root(s) there.  The record's prefix rows [0, n) hold the prefix as their actions and
// zeros in every per-move field (no search ran there): the record of the slot's previous game would otherwise show through.
template <class G> GAZ_KERNEL k_set_position(DevParams<G> E, int g, const int32_t* actions, int n) {
    using RL = RecLayout<G>;
    if (block_id() != 0 || g < 0 || g >= E.n_games) return;
    {
        uint8_t* rec = E.recs + (size_t)g * RL::SIZE;
        const int m = n < G::MAXT ? n : G::MAXT;
        uint32_t* q = reinterpret_cast<uint32_t*>(rec + RL::OFF_Q); uint32_t* rv = reinterpret_cast<uint32_t*>(rec + RL::OFF_RV);
        uint32_t* ev = reinterpret_cast<uint32_t*>(rec + RL::OFF_EV);
        for (int i = lane_id(); i < m; i += WAVE) { q[i] = 0u; rv[i] = 0u; ev[i] = 0u; rec[RL::OFF_MK + i] = MK_NONE; }
        uint32_t* pol = reinterpret_cast<uint32_t*>(rec + RL::OFF_POL); uint32_t* nn = reinterpret_cast<uint32_t*>(rec + RL::OFF_N);
        uint32_t* w = reinterpret_cast<uint32_t*>(rec + RL::OFF_W); uint32_t* p = reinterpret_cast<uint32_t*>(rec + RL::OFF_P);
        for (int i = lane_id(); i < m * G::A; i += WAVE) { pol[i] = 0u; nn[i] = 0u; w[i] = 0u; p[i] = 0u; }
    }
    if (lane_id() != 0) return;
    GameState<G>& gs = E.games[g];
    const uint32_t seq = gs.game_seq, sid = gs.slot_id; const uint64_t ne = gs.n_evals, ns = gs.n_sims, np = gs.n_plies;
    memset(&gs, 0, sizeof(gs));
    gs.game_seq = seq; gs.n_evals = ne; gs.n_sims = ns; gs.n_plies = np; gs.host_move = -1; gs.winner = RUNNING; gs.slot_id = sid;
    int player = -1;
    for (int i = 0; i < n && i < G::MAXT; ++i) {
        const int a = actions[i];
        gs.board[landing_cell<G>(gs.board, a)] = (int8_t)player;
        gs.hist[i] = (uint8_t)a; player = -player;
        E.recs[(size_t)g * RL::SIZE + RL::OFF_ACT + i] = (uint8_t)a;
    }
    gs.n_hist = n < G::MAXT ? n : G::MAXT; gs.next_player = player;
    gs.roots_todo = (E.single_tree || E.gstate) ? 1 : 3; gs.phase = (E.sync_moves && E.single_tree) ? PH_IDLE : PH_ROOT; gs.pend_kind = PEND_NONE;
    for (int t = 0; t < 2; ++t) { TreeState& ts = E.trees[(size_t)g * 2 + t]; ts.root = -1; ts.n_nodes = 0; ts.root_visits = 0; ts.event = 0; }
}

// gaz_engine_read_positions: the action history of every slot's game in progress (what gaz_engine_set_position takes)
template <class G> GAZ_KERNEL k_read_positions(DevParams<G> E, int32_t* n_hist, uint8_t* hist, int stride) {
    const int g = block_id();
    if (g >= E.n_games) return;
    const GameState<G>& gs = E.games[g];
    const int n = gs.phase == PH_HALT ? 0 : gs.n_hist;
    for (int i = lane_id(); i < stride; i += WAVE) hist[(size_t)g * stride + i] = i < n ? gs.hist[i] : (uint8_t)0;
    if (lane_id() == 0) n_hist[g] = n;
}

template <class G> GAZ_KERNEL k_start_search(DevParams<G> E) {      // PH_IDLE -> build the missing root(s), then MCTS.run
    const int g = block_id();
    if (g >= E.n_games || lane_id() != 0) return;
    if (E.games[g].phase == PH_IDLE) E.games[g].phase = PH_ROOT;
}

// Game-rules probe (gaz_engine_probe_rules): one wavefront per position, the position given as an action history from the empty
// board.  Runs the DEVICE rule code the search uses — landing_cell / wins_after (do_action_MCTS + check_win_MCTS), build_legal
// (get_legal_actions_MCTS), encode_input (get_input_state_MCTS), terminal_probe (get_terminal_actions_fn), make_priors without
// noise (get_legal_actions_policy_MCTS, normalize=True) — so the reference's Game classes can be compared with it directly.
template <class G> GAZ_KERNEL k_probe_rules(DevParams<G> E, const int32_t* actions, const int32_t* n_actions, int n_pos, int stride,
                                            int8_t* o_board, uint8_t* o_legal, int32_t* o_winner, int8_t* o_input, int32_t* o_term,
                                            const float* policy_in, float* o_policy) {
    GAZ_SHARED Scratch<G> S;
    const int p = block_id();
    if (p >= n_pos) return;
    const int n = n_actions[p];
    for (int c = lane_id(); c < G::BPAD; c += WAVE) S.board[c] = 0;
    wave_sync();
    int player = -1, winner = RUNNING;
    for (int i = 0; i < n; ++i) {
        const int a = actions[(size_t)p * stride + i];
        if (!action_legal<G>(S.board, a)) { if (lane_id() == 0) o_winner[p] = -99; return; }   // not a legal history
        const int cell = landing_cell<G>(S.board, a);
        const bool win = wins_after<G>(S.board, cell, player);
        const int empties = G::DRAWS ? count_empty<G>(S.board) : 2;
        winner = win ? player : ((G::DRAWS && empties == 1) ? 0 : RUNNING);        // check_win after this move
        wave_sync();
        if (lane_id() == 0) S.board[cell] = (int8_t)player;
        wave_sync();
        player = -player;
    }
    for (int c = lane_id(); c < G::HW; c += WAVE) o_board[(size_t)p * G::HW + c] = S.board[c];
    const int n_legal = build_legal<G>(S.board, S.legal);
    for (int a = lane_id(); a < G::A; a += WAVE) { o_legal[(size_t)p * G::A + a] = 0; o_term[(size_t)p * G::A + a] = -1; if (o_policy) o_policy[(size_t)p * G::A + a] = 0.0f; }
    wave_sync();
    for (int i = lane_id(); i < n_legal; i += WAVE) o_legal[(size_t)p * G::A + S.legal[i]] = 1;
    uint8_t h3[3];
    for (int i = 0; i < 3; ++i) h3[i] = (n - 1 - i >= 0) ? (uint8_t)actions[(size_t)p * stride + n - 1 - i] : 0;
    encode_input<G>(S.board, -player, h3, n, o_input + (size_t)p * (G::HW * G::C));
    if (lane_id() == 0) o_winner[p] = winner;
    if (policy_in && o_policy && n_legal > 0) {
        DevParams<G> E2 = E; E2.use_dirichlet = 0;
        make_priors<G>(E2, 0, E.games[0], E.trees[0], 0, S, policy_in + (size_t)p * G::A, n_legal);   // game / tree state: untouched without noise
        for (int i = lane_id(); i < n_legal; i += WAVE) o_policy[(size_t)p * G::A + S.legal[i]] = S.pri[i];
        wave_sync();
    }
    if (winner != RUNNING) return;                                                 // the search never expands a finished position
    bool any_win;
    const int nt = terminal_probe<G>(S.board, S.legal, n_legal, player, S.tact, S.twin, any_win, E.fast_find_win != 0);
    for (int i = lane_id(); i < nt; i += WAVE) o_term[(size_t)p * G::A + S.tact[i]] = S.twin[i] ? 1 : 0;
}

// gaz_engine_repack: move the running game of physical slot `src` into the halted slot `dst` (dst < src).  Everything a game owns
// travels: its tree arena slice, both tree heads, the path buffer, the record in progress, the Gumbel state, the rows of the
// evaluator batch (a pending request's answer is waiting there) — and the GameState is SWAPPED, so the halted slot's lifetime
// counters stay in the sum gaz_engine_get_stats reports.  The game keeps its identity (GameState::slot_id).
template <class G> GAZ_KERNEL_WIDE k_move_slots(DevParams<G> E, const int32_t* moves, int n_moves, size_t arena_slot_bytes, size_t gstate_bytes) {
#ifdef GAZ_HOST_EMU
    const int b = block_id(), T = 1, t = 0;
#else
    const int b = blockIdx.x, T = blockDim.x, t = threadIdx.x;
#endif
    if (b >= n_moves) return;
    const int src = moves[2 * b], dst = moves[2 * b + 1];
    auto copy16 = [&](void* d, const void* s_, size_t bytes) {        // bytes % 16 == 0
        uint4* dd = reinterpret_cast<uint4*>(d); const uint4* ss = reinterpret_cast<const uint4*>(s_);
        for (size_t i = t; i < bytes / 16; i += T) dd[i] = ss[i];
    };
    auto copy1 = [&](void* d, const void* s_, size_t bytes) {
        uint8_t* dd = reinterpret_cast<uint8_t*>(d); const uint8_t* ss = reinterpret_cast<const uint8_t*>(s_);
        for (size_t i = t; i < bytes; i += T) dd[i] = ss[i];
    };
    copy16(E.arena + (size_t)dst * arena_slot_bytes, E.arena + (size_t)src * arena_slot_bytes, arena_slot_bytes);
    copy16(E.recs + (size_t)dst * RecLayout<G>::SIZE, E.recs + (size_t)src * RecLayout<G>::SIZE, RecLayout<G>::SIZE);
    copy1(E.paths + (size_t)dst * PathCap<G>::V, E.paths + (size_t)src * PathCap<G>::V, sizeof(PathEnt) * PathCap<G>::V);
    copy1(&E.trees[(size_t)dst * 2], &E.trees[(size_t)src * 2], 2 * sizeof(TreeState));
    if (E.gstate) copy1(reinterpret_cast<uint8_t*>(E.gstate) + (size_t)dst * gstate_bytes, reinterpret_cast<uint8_t*>(E.gstate) + (size_t)src * gstate_bytes, gstate_bytes);
    copy1(E.nn_in + (size_t)dst * (G::HW * G::C), E.nn_in + (size_t)src * (G::HW * G::C), G::HW * G::C);
    copy1(E.nn_policy + (size_t)dst * G::A, E.nn_policy + (size_t)src * G::A, 4 * G::A);
    copy1(E.nn_value + dst, E.nn_value + src, 4);
    copy1(E.row_sym() + dst, E.row_sym() + src, 1);                      // the symmetry the row was encoded under answers with it
    if (E.eval_done) copy1(E.eval_done + dst, E.eval_done + src, 4);
    // swap the two GameStates word by word (each thread its own words: no staging needed)
    uint32_t* ga = reinterpret_cast<uint32_t*>(&E.games[src]); uint32_t* gb = reinterpret_cast<uint32_t*>(&E.games[dst]);
    for (size_t i = t; i < sizeof(GameState<G>) / 4; i += T) { const uint32_t x = ga[i]; ga[i] = gb[i]; gb[i] = x; }
}

// gaz_engine_debug_fused_fault on a path without the fused launch (other games / searches / the CPU emulation build): what a trunk workgroup
// that gave up leaves behind — its boards marked with the wave's epoch, their outputs NOT those of this wave's requests (poisoned here, so that
// a tree step that consumed them could not go unnoticed), the fault counter raised.
template <class G> GAZ_KERNEL k_debug_skip(DevParams<G> E, uint32_t* eval_done, int n, unsigned mod, int32_t* fault) {
    const int g = block_id();
    if (g >= n || lane_id() != 0) return;
    if ((unsigned)(g / 3) % mod != 1u) { eval_done[g] = E.wave_epoch; return; }      // evaluated this wave
    for (int a = 0; a < G::A; ++a) E.nn_policy[(size_t)g * G::A + a] = __builtin_nanf("");
    E.nn_value[g] = __builtin_nanf("");
    if (g % 3 == 0) atomic_add(fault, (int32_t)1);
}

template <class G> GAZ_KERNEL k_release(DevParams<G> E, const int32_t* moves) {
    const int g = block_id();
    if (g >= E.n_games || lane_id() != 0) return;
    GameState<G>& gs = E.games[g];
    if (gs.phase == PH_IDLE && moves && moves[g] >= 0 && gs.n_hist < G::MAXT) E.recs[(size_t)g * RecLayout<G>::SIZE + RecLayout<G>::OFF_MK + gs.n_hist] = MK_NONE;   // played without a search
    if (gs.phase == PH_WAIT_HOST || (gs.phase == PH_IDLE && moves && moves[g] >= 0)) { gs.host_move = moves ? moves[g] : -1; gs.phase = PH_APPLY; }
}

// gaz_engine_set_solver(1): tag the edges into the terminal parents that were made while the solver was off (their status is derived from their
// record, puct_core.hpp rule 1), in every record the trees have allocated.  One wavefront per game, a lane per node record; the stream is idle.
template <class G> GAZ_KERNEL k_solver_retag(DevParams<G> E) {
    const int g = block_id();
    if (g >= E.n_games) return;
    for (int t = 0; t < 2; ++t) {
        const TreeState& ts = E.trees[(size_t)g * 2 + t];
        if (ts.root < 0) continue;
        const int n = (int)(ts.n_nodes < (uint32_t)E.nodes_per_tree ? ts.n_nodes : (uint32_t)E.nodes_per_tree);
        for (int i = lane_id(); i < n; i += WAVE) {
            const NodeRef<G> nd = node_at(E, g, t, i);
            if (nd.hdr()->flags & NF_TERMINAL_PARENT) continue;
            int nc = nd.hdr()->n_children;
            if (nc > G::A) nc = G::A;
            for (int s = 0; s < nc; ++s) {
                const int32_t w = nd.child()[s];
                if (w < 0 || child_tag(w) != ST_UNKNOWN || w >= E.nodes_per_tree) continue;
                const NodeRef<G> x = node_at(E, g, t, w);
                if (!(x.hdr()->flags & NF_TERMINAL_PARENT)) continue;
                int xn = x.hdr()->n_children, st = ST_DRAW;
                if (xn > G::A) xn = G::A;
                for (int k = 0; k < xn; ++k) if (x.child()[k] == CHILD_LEAF_WIN) st = ST_WIN;
                nd.child()[s] = w | (st << CHILD_TAG_SHIFT);
            }
        }
    }
}

// dense copies of the last MCTS.run result of every game (engine_get_root_stats)
template <class G> GAZ_KERNEL k_gather_root(DevParams<G> E, uint32_t* oN, float* oW, float* oP, float* oPol, uint32_t* oRV,
                                             float* oQ, int32_t* oChosen, int32_t* oPhase, int32_t* oPending) {
    using RL = RecLayout<G>;
    const int g = block_id();
    if (g >= E.n_games) return;
    const GameState<G>& gs = E.games[g];
    const uint8_t* rec = E.recs + (size_t)g * RL::SIZE;
    const int ply = gs.n_hist < G::MAXT ? gs.n_hist : G::MAXT - 1;
    for (int a = lane_id(); a < G::A; a += WAVE) {
        oN[(size_t)g * G::A + a] = reinterpret_cast<const uint32_t*>(rec + RL::OFF_N)[(size_t)ply * G::A + a];
        oW[(size_t)g * G::A + a] = reinterpret_cast<const float*>(rec + RL::OFF_W)[(size_t)ply * G::A + a];
        oP[(size_t)g * G::A + a] = reinterpret_cast<const float*>(rec + RL::OFF_P)[(size_t)ply * G::A + a];
        oPol[(size_t)g * G::A + a] = reinterpret_cast<const float*>(rec + RL::OFF_POL)[(size_t)ply * G::A + a];
    }
    if (lane_id() == 0) {
        oRV[g] = reinterpret_cast<const uint32_t*>(rec + RL::OFF_RV)[ply];
        oQ[g] = reinterpret_cast<const float*>(rec + RL::OFF_Q)[ply];
        oChosen[g] = gs.chosen; oPhase[g] = gs.phase; oPending[g] = gs.pend_kind;
    }
}

template <class G> GAZ_KERNEL k_count(DevParams<G> E, int32_t* out) {   // out[0] = games still searching, out[1] = pending evals
    const int g = block_id();
    if (g >= E.n_games || lane_id() != 0) return;
    const GameState<G>& gs = E.games[g];
    if (gs.phase != PH_WAIT_HOST && gs.phase != PH_HALT && gs.phase != PH_IDLE) atomic_add(&out[0], 1);
    if (gs.pend_kind != PEND_NONE) atomic_add(&out[1], 1);
    atomic_add(reinterpret_cast<unsigned long long*>(out + 2), (unsigned long long)gs.n_evals);
    atomic_add(reinterpret_cast<unsigned long long*>(out + 4), (unsigned long long)gs.n_sims);
    atomic_add(reinterpret_cast<unsigned long long*>(out + 6), (unsigned long long)gs.n_plies);
    atomic_add(reinterpret_cast<unsigned long long*>(out + 8), (unsigned long long)gs.n_hits);
}

// ------------------------------------------------------------------------------------------ engine
struct gaz_engine {
    gaz_engine_config cfg;
    std::string err;
    int grouped = 0;                                 // > 1: this engine is one of that many game groups of a GroupEngine (launch-shape defaults differ)
    virtual void note_grouped() {}
    virtual ~gaz_engine() { delete score; }
    // held-out loss (score.hpp): the scorer's buffers, made on first use; wave_open: between gaz_engine_wave_begin and gaz_engine_wave_end
    ScoreState* score = nullptr;
    bool wave_open = false;
    ScoreState* score_state() {
        if (!score) { score = new ScoreState(); score->game = cfg.game; score->device = cfg.device; score->A = cfg.game == GAZ_GAME_TICTACTOE ? 9 : (cfg.game == GAZ_GAME_CONNECT4 ? 7 : 225); }
        return score;
    }
    int score_mode() const { return cfg.policy_is_logits == 1 ? (cfg.gumbel_stablemax ? 3 : 1) : (cfg.policy_is_logits == 2 ? 2 : 0); }
    // gaz_engine_score_replay behind the checks of the totals struct; an engine of several game groups keeps this refusal
    virtual int score_replay(gaz_replay*, int, int, gaz_score_totals*, double*, double*, double*, uint8_t*, double*) {
        return fail("score_replay: game groups hold one evaluator batch each: like read_batch it needs game_groups = 1");
    }
    int fail(const std::string& m) { err = m; return 1; }
    virtual int init() = 0;
    virtual int load_weights(const gaz_tensor* t, int n) = 0;
    virtual int reset_games(const int32_t* slots, int n) = 0;
    virtual int run_move(int32_t* n_waiting) = 0;
    virtual int get_root_stats(uint32_t*, float*, float*, float*, uint32_t*, float*, int32_t*, int32_t*) = 0;
    virtual int apply_moves(const int32_t* moves) = 0;
    virtual int run_waves(int n) = 0;
    virtual int wave_begin() = 0;
    virtual int wave_end() = 0;
    virtual int batch_ptrs(void**, void**, void**) = 0;
    virtual int read_batch(int8_t*, int32_t*) = 0;
    virtual int batch_rows(int32_t*) = 0;
    virtual int write_outputs(const float*, const float*) = 0;
    virtual int evaluate(const int8_t*, int, float*, float*, int, double*) = 0;
    virtual int record_layout(gaz_record_layout*) = 0;
    virtual int drain(void* out, int max_records, int32_t* n_out) = 0;
    virtual int sample_layout(gaz_sample_layout*) = 0;
    // gaz_engine_drain_samples for one ring: the caller's arrays start at this call's first game / row, their augmentation planes are `plane_rows`
    // rows apart, games[i][4] = row_base + the row in this call.  *blocked_T = rows of the oldest game when it alone is more than max_rows (else 0).
    // row_ply (may be null): the ply of every row, from this call's first row on
    virtual int drain_samples(int max_games, int64_t max_rows, int64_t plane_rows, int64_t row_base, int32_t* games, int8_t* boards, float* policies,
                              float* values, uint8_t* row_ply, int32_t* n_games, int64_t* n_rows, int32_t* blocked_T) = 0;
    // policy surprise weighting of the rows (samples.hpp): lambda = 0 is off, the state of a new engine; read by the next drain
    double sw_lambda = 0.0, sw_fast_factor = 1.5;
    virtual int set_sample_weighting(double lambda, double fast_factor) { sw_lambda = lambda; sw_fast_factor = fast_factor; return 0; }
    virtual int get_stats(uint64_t out[16]) = 0;
    virtual int synchronize() = 0;
    virtual int timing_reset(int enable) = 0;
    virtual int timing_get(double*, double*, double*, int64_t*, int64_t*) = 0;
    virtual int dominant(char*, int, double*) = 0;
    virtual int set_position(int, const int32_t*, int) = 0;
    virtual int set_search_params(int, int) = 0;
    virtual int stop_search(int) = 0;
    virtual int start_search() = 0;
    virtual int set_hyperparams(const gaz_search_hyperparams*) = 0;
    virtual int set_resignation(const gaz_resign_params*) = 0;
    virtual int get_resign_stats(uint64_t out[8]) = 0;
    // opening book (book.hpp) behind the argument checks of the C entry point: n_entries = 0 removes the book
    virtual int set_opening_book(int n_entries, int stride, int mode, const uint8_t* actions, const int32_t* lengths) = 0;
    virtual int read_book_counts(uint64_t* counts, uint64_t out[8]) = 0;
    int book_entries = 0, book_mode = 0;             // what gaz_engine_get_opening_book reports: the book in force
    virtual int set_eval_symmetry(int32_t mode) = 0;
    virtual int get_eval_symmetry(int32_t* mode) = 0;
    virtual int read_batch_symmetry(uint8_t* sym) = 0;
    virtual int set_solver(int32_t mode) = 0;
    virtual int get_solver(int32_t* mode) = 0;
    virtual int get_solver_stats(uint64_t out[8]) = 0;
    virtual int read_head_features(int, float*, float*, int32_t*, int32_t*) = 0;
    virtual int set_fused_wave(int) = 0;
    virtual int debug_fused_fault(int) = 0;
    virtual int read_positions(int32_t*, uint8_t*, int) = 0;
    // gaz_engine_read_trees / gaz_engine_read_pv behind the argument checks of the C entry points (slots in range, tree id valid for this engine)
    // node_first / edge_first are always filled.  With `want_records`, `place` is then asked ONCE, with the totals, where the records go: it
    // returns non-zero to refuse (its own error text stands), or sets both pointers to arrays of at least that size
    typedef std::function<int(int64_t n_nodes, int64_t n_edges, gaz_tree_node** nodes, gaz_tree_edge** edges)> TreePlace;
    virtual int read_trees(const int32_t* slots, int n_slots, int tree, int max_depth, uint32_t min_visits, int64_t* node_first, int64_t* edge_first,
                           bool want_records, const TreePlace& place) = 0;
    virtual int read_pv(int tree, const int32_t* first_action, int max_len, uint8_t* actions, uint32_t* N, float* W, int32_t* len) = 0;
    int short_capacity(int64_t need_nodes, int64_t need_edges, int64_t max_nodes, int64_t max_edges) {
        return fail("read_trees: the export needs " + std::to_string(need_nodes) + " nodes and " + std::to_string(need_edges) + " edges, max_nodes is " +
                    std::to_string(max_nodes) + " and max_edges is " + std::to_string(max_edges));
    }
    virtual int repack(int32_t*, int32_t*) = 0;
    virtual int set_match(int32_t mode, uint32_t hash_salt_b) = 0;
    virtual int get_match(int32_t* mode) = 0;
    virtual int load_weights_b(const gaz_tensor* t, int n) = 0;
    virtual int read_batch_network(uint8_t* net) = 0;
    virtual int get_match_stats(uint64_t out[8]) = 0;
    virtual int get_match_timing(double out[8]) = 0;
    virtual int probe_rules(const int32_t*, const int32_t*, int, int, int8_t*, uint8_t*, int32_t*, int8_t*, int32_t*, const float*, float*) = 0;
    virtual int probe_det(int, int, const uint64_t*, int, uint64_t*, int) = 0;
};

// device allocations that live for one call (gaz_engine_read_trees / gaz_engine_read_pv)
struct CallScratch {
    std::vector<void*> p;
    ~CallScratch() { for (void* q : p) hipFree(q); }
    template <class T> T* get(size_t n) { void* q = nullptr; if (hipMalloc(&q, (n ? n : 1) * sizeof(T)) != hipSuccess) return nullptr; p.push_back(q); return (T*)q; }
};

// ------------------------------------------------------------------------------------------ config
// why k game groups cannot be made of this config (nullptr: they can)
static const char* group_fault(const gaz_engine_config& c, int k) {
    if (k < 2 || k > c.n_games) return "game_groups must be in [1, n_games]";
    if (c.sync_moves || c.evaluator == GAZ_EVAL_EXTERNAL) return "game_groups > 1 needs continuous self-play (sync_moves = 0) with a built-in evaluator";
    if (c.games_budget > 0 && c.games_budget < c.n_games) return "game_groups > 1 with a games_budget below n_games: a group could be left without a game (use game_groups = 1)";
    return nullptr;
}

// every refusal of a config that needs no device state, first fault first ("" = none), for an engine of `groups` game groups: one group is the
// engine itself; a GroupEngine checks what it needs to split the games, and each group's own config is checked when that group is made
static std::string config_fault(const gaz_engine_config& c, int groups) {
    if (c.game_groups < 0) return "game_groups must be >= 0";
    if (c.gumbel_batch < 0 || c.gumbel_batch > 64) return "gumbel_batch must be in [0, 64] (0 and 1 = one candidate of sequential halving per game and wave)";
    if (c.gumbel_batch > 1) {                     // the chunk step exists for the Gumbel search with one batch and no evaluation cache
        if (c.leaf_batch > 1) return "gumbel_batch > 1 cannot be combined with leaf_batch > 1";
        if (c.search != GAZ_SEARCH_GUMBEL) return "gumbel_batch > 1 needs search = GAZ_SEARCH_GUMBEL (the PUCT search has leaf_batch)";
        if (c.eval_cache_log2 > 0) return "gumbel_batch > 1 cannot be combined with eval_cache_log2 > 0";
        if (c.game_groups > 1) return "gumbel_batch > 1 cannot be combined with game_groups > 1";
    }
    if (c.leaf_batch < 0 || c.leaf_batch > 64) return "leaf_batch must be in [0, 64] (0 and 1 = one leaf per game and wave)";
    if (c.leaf_batch > 1) {                       // the K-leaf step exists for the PUCT search with one batch and no evaluation cache
        if (c.search == GAZ_SEARCH_GUMBEL) return "leaf_batch > 1 needs search = GAZ_SEARCH_PUCT (the Gumbel search plans its simulations itself)";
        if (c.eval_cache_log2 > 0) return "leaf_batch > 1 cannot be combined with eval_cache_log2 > 0";
        if (c.game_groups > 1) return "leaf_batch > 1 cannot be combined with game_groups > 1";
    }
    // playout cap randomisation: fast_iterations = 0 is off (and then takes no probability), else a fast limit in [1, run_iterations] and p in (0, 1]
    if (c.fast_iterations < 0) return "fast_iterations must be >= 0 (0 = no playout cap), not " + std::to_string(c.fast_iterations);
    if (c.fast_iterations > c.run_iterations) return "fast_iterations (" + std::to_string(c.fast_iterations) + ") must not exceed run_iterations (" + std::to_string(c.run_iterations) + ")";
    if (c.fast_iterations > 0 && !(c.full_search_prob > 0.0 && c.full_search_prob <= 1.0)) return "full_search_prob must be in (0, 1] with fast_iterations > 0, not " + std::to_string(c.full_search_prob);
    if (c.fast_iterations == 0 && !(c.full_search_prob == 0.0)) return "full_search_prob must be 0 with fast_iterations = 0 (the playout cap is off)";
    if (c.fast_iterations > 0 && c.move_time_limit > 0.0) return "fast_iterations > 0 cannot be combined with move_time_limit > 0 (a timed move has no iteration cap to randomise)";
    // forced playouts + policy target pruning: k = 0 is off, else a finite k > 0 on a PUCT root
    if (c.forced_playouts_k != c.forced_playouts_k) return "forced_playouts_k must be a number (0 = no forced playouts), not NaN";
    if (c.forced_playouts_k < 0.0) return "forced_playouts_k must be >= 0 (0 = no forced playouts), not " + std::to_string(c.forced_playouts_k);
    if (c.forced_playouts_k > 1.7976931348623157e308) return "forced_playouts_k must be finite (KataGo uses 2), not infinity";
    if (c.forced_playouts_k > 0.0 && c.search == GAZ_SEARCH_GUMBEL) return "forced_playouts_k > 0 cannot be combined with search = GAZ_SEARCH_GUMBEL (sequential halving has no PUCT root to force playouts at)";
    if (groups > 1) { const char* g = group_fault(c, groups); return g ? g : ""; }
    int max_t = 0, n_act = 0;
    switch (c.game) {
        case GAZ_GAME_TICTACTOE: max_t = Game<GAME_TTT>::MAXT; n_act = Game<GAME_TTT>::A; break;
        case GAZ_GAME_CONNECT4: max_t = Game<GAME_C4>::MAXT; n_act = Game<GAME_C4>::A; break;
        case GAZ_GAME_GOMOKU: max_t = Game<GAME_GMK>::MAXT; n_act = Game<GAME_GMK>::A; break;
        default: return "unknown game id";
    }
    if (c.n_games <= 0) return "n_games must be positive";
    if (c.search != GAZ_SEARCH_PUCT && c.search != GAZ_SEARCH_GUMBEL) return "unknown search id";
    if (c.search == GAZ_SEARCH_GUMBEL && (c.gumbel_m < 2 || c.run_iterations < 1)) return "Gumbel search needs m >= 2 and run_iterations >= 1";
    if (c.max_actions > max_t || c.max_actions <= 0) return "max_actions out of range for this game";
    if (!(c.move_time_limit >= 0.0) || c.move_time_limit > 1e6) return "move_time_limit must be in [0, 1e6] seconds";
    if (c.move_time_limit > 0.0 && c.sync_moves) return "move_time_limit is for continuous self-play; the per-move API has gaz_engine_stop_search";
    if (c.games_budget < 0) return "games_budget must be >= 0";
    if (c.games_budget > 0 && c.sync_moves) return "games_budget needs continuous self-play (sync_moves = 0)";
    if (c.n_opening < 0 || c.n_opening > 8) return "at most 8 opening_actions";
    for (int i = 0; i < c.n_opening; ++i) if (c.opening_actions[i] < 0 || c.opening_actions[i] >= n_act) return "opening action out of range";
    if (c.eval_cache_log2 < 0 || c.eval_cache_log2 > 28) return "eval_cache_log2 out of range (0 = off, at most 28)";
    return "";
}

// an event that lives for one call (gaz_engine_evaluate), whichever way the call returns
struct CallEvent { hipEvent_t e = 0; bool ok; CallEvent() : ok(hipEventCreate(&e) == hipSuccess) {} ~CallEvent() { if (ok) hipEventDestroy(e); } };

template <class G> struct EngineT : gaz_engine {
    using RL = RecLayout<G>;
    DevParams<G> E;
    hipStream_t stream = 0;
    Evaluator* eval = nullptr;
    // dense scratch for get_root_stats / counters
    uint32_t* dN = nullptr; float* dW = nullptr; float* dP = nullptr; float* dPol = nullptr; uint32_t* dRV = nullptr;
    float* dQ = nullptr; int32_t* dChosen = nullptr; int32_t* dPhase = nullptr; int32_t* dPending = nullptr;
    int32_t* dCount = nullptr; int32_t* dMoves = nullptr; int32_t* dSlots = nullptr;
    uint32_t ring_consumed = 0;
    bool timing = false;
    std::vector<hipEvent_t> ev;      // every timing event (owned)
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_tree, ev_eval;   // brackets around tree steps / evaluator passes
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_fused;           // brackets around fused tree + trunk launches
    int64_t n_waves_total = 0, n_waves_timed = 0;
    static constexpr int TIMING_STRIDE = 8;
    std::vector<void*> allocs;
    // leaf-batched search: K leaves per game and wave (1 = off), rows = n_games * K rows in the evaluator batch, descriptors of the leaves in flight
    int lbk = 1; size_t rows = 0; LeafBatch LB{1, nullptr};
    // batched sequential halving (Gumbel search, gumbel_batch = K > 1): lbk = K as well — the rows plumbing is the same — and the per-row state
    int gbk = 1; GumbelBatch GB{1, nullptr};

    template <class T> int dalloc(T** p, size_t n) {
        void* q = nullptr;
        HIP_OK(hipMalloc(&q, n * sizeof(T)));
        HIP_OK(hipMemset(q, 0, n * sizeof(T)));
        allocs.push_back(q); *p = (T*)q; return 0;
    }

    ~EngineT() override {
        hipStreamSynchronize(stream);
        if (E.prof) {                               // GAZ_TREE_PROF=1: phase cycles of the PUCT kernel, summed over games, to stderr
            std::vector<unsigned long long> h((size_t)E.n_games * 8);
            hipMemcpy(h.data(), E.prof, h.size() * 8, hipMemcpyDeviceToHost);
            unsigned long long t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            for (size_t i = 0; i < h.size(); ++i) t[i % 8] += h[i];
            const char* nm[7] = {"consume", "select / descent", "expand_pre", "cache_probe", "expand_post(hit)", "terminal backup", "whole launch"};
            fprintf(stderr, "[tree prof] launches/game %.0f\n", (double)t[7] / E.n_games);
            for (int k = 0; k < 7; ++k) fprintf(stderr, "[tree prof] %-18s %8.0f cycles / game-launch (%.1f %%)\n", nm[k], (double)t[k] / (double)t[7], 100.0 * t[k] / t[6]);
        }
        delete eval; delete eval_b;
        if (h_match_cnt) hipHostFree(h_match_cnt);
        for (void* p : allocs) hipFree(p);
        free_book(book_act, book_len, book_cnt);
        if (dSamples) hipFree(dSamples);
        if (hSamples) hipHostFree(hSamples);
        for (hipEvent_t e : ev) hipEventDestroy(e);
        if (pipeline_ready) {
            hipStreamSynchronize(tstream); hipStreamSynchronize(hstream);
            for (int p = 0; p < 2; ++p) for (int i = 0; i < n_grp; ++i) { hipEventDestroy(ev_tree_done[p][i]); hipEventDestroy(ev_trunk_done[p][i]); hipEventDestroy(ev_heads_done[p][i]); }
            hipEventDestroy(ev_join); hipStreamDestroy(tstream); hipStreamDestroy(hstream);
        }
        hipStreamDestroy(stream);
    }

    // nodes per tree that `it` iterations per move (and Gumbel's m) need when nodes_per_tree is left to the engine: what init() sizes the arena
    // from, and what set_hyperparams() holds later values against
    long long nodes_needed(int it, int m) const {
        const long long its = it < 3 * G::A ? 3 * G::A : it;
        if (cfg.search == GAZ_SEARCH_GUMBEL) return 2LL * (it + m) + 3 * G::A + 64;      // fresh tree every move
        if (E.compact) return 4 * its + 3 * G::A + 64;      // per half: kept subtree + one run; generous bound, ERR_ARENA_FULL if a game exceeds it
        // a tree lives for the whole game and gains <= 1 record per simulation of its own moves: every other ply, or with single_tree every ply
        const long long runs = cfg.single_tree ? (long long)cfg.max_actions + 1 : (cfg.max_actions + 1) / 2 + 1;
        return runs * (its + 2) + 64;
    }

    int init() override {
        HIP_OK(hipSetDevice(cfg.device));
        HIP_OK(hipStreamCreate(&stream));
        memset(&E, 0, sizeof(E));
        const int n = cfg.n_games;               // (the config has passed config_fault)
        const bool gumbel = cfg.search == GAZ_SEARCH_GUMBEL;
        E.c_visit = cfg.c_visit; E.c_scale = cfg.c_scale; E.gumbel_m = cfg.gumbel_m; E.g_stablemax = cfg.gumbel_stablemax; E.fast_find_win = cfg.fast_find_win;
        E.node_bytes = gumbel ? gumbel_node_bytes<G>() : NodeLayout<G>::SIZE;
        // re-root compaction: needed where a whole-game arena does not fit (Gomoku: 4.2 KB records); 0 = auto
        E.compact = gumbel ? 0 : (cfg.compact_trees == 0 ? (G::ID == GAME_GMK ? 1 : 0) : (cfg.compact_trees > 0 ? 1 : 0));
        gbk = gumbel && cfg.gumbel_batch > 1 ? cfg.gumbel_batch : 1;
        lbk = gbk > 1 ? gbk : (cfg.leaf_batch > 1 ? cfg.leaf_batch : 1); rows = (size_t)n * lbk;
        E.n_games = n; n_eff = n; E.run_iterations = cfg.run_iterations; E.max_actions = cfg.max_actions;
        E.explore_first = cfg.num_explore_actions_first; E.explore_second = cfg.num_explore_actions_second;
        E.create_new_root = cfg.create_new_root; E.sync_moves = cfg.sync_moves; E.use_dirichlet = cfg.use_dirichlet;
        int npt = cfg.nodes_per_tree;
        if (npt <= 0) {   // on top of nodes_needed: a timed Gumbel move may run 3 A iterations; the K leaves a PUCT tree holds in flight
            const bool timed = gumbel && cfg.move_time_limit > 0.0 && 3 * G::A > cfg.run_iterations;
            npt = (int)nodes_needed(timed ? 3 * G::A : cfg.run_iterations, cfg.gumbel_m) + (!gumbel && lbk > 1 ? lbk : 0);
        }
        E.nodes_per_tree = npt;
        E.ring_cap = cfg.ring_capacity; E.single_tree = cfg.single_tree;
        E.tau = norm_tau(cfg.tau); E.no_gumbel_noise = cfg.no_gumbel_noise; E.first_game_seq = cfg.first_game_seq;
        E.move_time_ticks = cfg.move_time_limit > 0.0 ? (uint64_t)(cfg.move_time_limit * 1e8) + 1 : 0;
        E.fast_iterations = cfg.fast_iterations; E.full_search_prob = cfg.full_search_prob;
        E.forced_playouts_k = cfg.forced_playouts_k;
        E.games_budget = cfg.games_budget;
        E.n_opening = cfg.n_opening;
        for (int i = 0; i < cfg.n_opening; ++i) { E.opening_actions[i] = cfg.opening_actions[i]; E.opening_weights[i] = cfg.opening_weights[i]; }
        // measured: 32 -> 4 cuts the kernel tail 0.167 -> 0.067 ms; with the evaluation cache a hit is such a simulation too and 8 pays
        // (small boards; a Gomoku simulation is ten times as long and 8 only stretches the launch)
        // (round 2) with the fused tree + trunk launch the tail of the tree step hides behind the trunk: 12 pays there (69.6 k vs 67.9 k)
        // (round 3) with the completion queue and games that yield inside the phase loop, the tree step's tail no longer holds the trunk back, so more
        // evaluation-free simulations per launch only mean fewer rows without a request: Connect4 PUCT 4: 57.5 k, 8: 59.1 - 60.1 k, 12: 58.7 k;
        // Gumbel 4: 317 k, 8: 331 k, 16: 337 k; Gomoku 4: 2096, 16: 2177, 32: 2192 positions/s (tools/sweep_mts.sh, one box each)
        const bool resnet = cfg.evaluator == GAZ_EVAL_RESNET;
        const bool fusable = G::ID == GAME_C4 && cfg.search == GAZ_SEARCH_PUCT && resnet;
        const int fused_default = !resnet ? 0 : (G::ID == GAME_C4 ? (gumbel ? (cfg.eval_cache_log2 > 0 ? 0 : 16) : (cfg.eval_cache_log2 > 0 ? 12 : 8))
                                                                  : (G::ID == GAME_GMK && !gumbel && cfg.eval_cache_log2 == 0 ? 32 : 0));
        E.max_tree_sims = cfg.max_tree_sims_per_wave > 0 ? cfg.max_tree_sims_per_wave
                        : (fused_default ? fused_default : ((cfg.eval_cache_log2 > 0 && G::A <= 64) ? (fusable ? 12 : 8) : 4));
        E.c_init = cfg.c_puct_init; E.c_base = cfg.c_puct_base;
        E.alpha = (double)(float)cfg.dirichlet_alpha;     // alpha * np.ones_like(float32 policy) is float32 (MCTS.py:244-245)
        E.eps = cfg.dirichlet_epsilon; E.one_minus_eps = (float)(1.0 - cfg.dirichlet_epsilon);
        E.key0 = (uint32_t)cfg.seed; E.key1 = (uint32_t)(cfg.seed >> 32); E.slot_offset = cfg.slot_offset;
        const size_t arena_bytes = (size_t)n * 2 * (E.compact ? 2 : 1) * (size_t)npt * (size_t)E.node_bytes;
        void* a = nullptr;
        HIP_OK(hipMalloc(&a, arena_bytes));               // not zeroed: every record is written before it is read
        allocs.push_back(a); E.arena = (uint8_t*)a;
        if (dalloc(&E.trees, (size_t)n * 2)) return 1;
        if (dalloc(&E.games, (size_t)n)) return 1;
        if (dalloc(&E.paths, rows * PathCap<G>::V)) return 1;
        if (lbk > 1 && gbk <= 1) { LB.K = lbk; if (dalloc(&LB.pend, rows)) return 1; }
        if (gbk > 1) { GB.K = gbk; if (dalloc(&GB.rows, rows)) return 1; }
        if (gumbel) { GumbelState<G>* gp = nullptr; if (dalloc(&gp, (size_t)n)) return 1; E.gstate = gp; }
        if (dalloc(&E.recs, (size_t)n * RL::SIZE)) return 1;
        if (dalloc(&E.ring, (size_t)(cfg.ring_capacity > 0 ? cfg.ring_capacity : 1) * RL::SIZE)) return 1;
        if (dalloc(&E.ring_head, 4)) return 1;
        if (dalloc(&E.nn_in, rows * G::HW * G::C + 64)) return 1;
        if (dalloc(&E.nn_policy, rows * G::A + 64)) return 1;
        // behind the value rows, in the same allocation: one symmetry byte per batch row (DevParams::row_sym()), zeroed = the identity
        E.row_sym_off = (uint32_t)((rows + 64) * sizeof(float));
        if (dalloc(&E.nn_value, rows + 64 + (rows + 64 + 3) / 4)) return 1;
        if (cfg.eval_cache_log2 > 0) {
            const size_t slots = (size_t)1 << cfg.eval_cache_log2;
            E.cache_stride = CacheLayout<G>::SIZE; E.cache_mask = (uint32_t)(slots - 1); E.cache_epoch = 1;
            if (dalloc(&E.cache, slots * (size_t)E.cache_stride)) return 1;      // zeroed: tag 0 never matches (tags are odd)
            if (dalloc(&E.cache_lock, slots)) return 1;
        }
        if (env_on("GAZ_TREE_PROF", false)) { if (dalloc(&E.prof, (size_t)n * 8)) return 1; }
        if (!gumbel) {
            double* tb = nullptr;
            if (dalloc(&tb, (size_t)2 * PUCT_TABLE_N)) return 1;
            E.puct_table = tb;
            if (init_puct_table()) return 1;
        }
        if (dalloc(&E.stats, BOOK_STATS_OFFSET + BOOK_STATS_WORDS)) return 1;      // zeroed: resignation off, no opening book
        if (dalloc(&E.error, 4)) return 1;
        if (dalloc(&dN, (size_t)n * G::A) || dalloc(&dW, (size_t)n * G::A) || dalloc(&dP, (size_t)n * G::A) ||
            dalloc(&dPol, (size_t)n * G::A) || dalloc(&dRV, n) || dalloc(&dQ, n) || dalloc(&dChosen, n) ||
            dalloc(&dPhase, n) || dalloc(&dPending, rows) || dalloc(&dCount, 16) || dalloc(&dMoves, (size_t)n + G::MAXT) || dalloc(&dSlots, n)) return 1;
        std::string e2;
        gaz_engine_config ecfg = cfg; ecfg.n_games = (int32_t)rows;           // the evaluator's buffers hold every row of the batch
        eval = make_evaluator(ecfg, G::H, G::W, G::C, G::A, &e2);
        if (!eval && cfg.evaluator != GAZ_EVAL_EXTERNAL) return fail("evaluator: " + e2);
        GAZ_LAUNCH(k_init_games<G>, n, WAVE, stream, E, (int)cfg.first_game_seq);
        HIP_OK(hipGetLastError());
        HIP_OK(hipStreamSynchronize(stream));
        return 0;
    }

    void note_grouped() override { if (eval) eval->set_shared_chip(this->grouped > 1); }

    int check_device_error() {
        int32_t code = 0;
        HIP_OK(hipMemcpy(&code, E.error, sizeof(code), hipMemcpyDeviceToHost));
        if (code) {
            const char* names[] = {"", "tree arena full (raise nodes_per_tree)", "root not fully expanded at move end",
                                   "selection path longer than the game can last", "state-machine loop guard", "PUCT picked an un-poppable child"};
            return fail(std::string("device error: ") + (code > 0 && code < 6 ? names[code] : "unknown"));
        }
        return 0;
    }

    int load_weights(const gaz_tensor* t, int n) override {
        if (!eval) return fail("no evaluator to load weights into");
        std::string m;
        if (eval->load(t, n, stream, &m)) return fail("load_weights: " + m);
        if (E.cache) {                              // cached outputs belong to the previous weights
            HIP_OK(hipMemsetAsync(E.cache, 0, ((size_t)E.cache_mask + 1) * (size_t)E.cache_stride, stream));
            HIP_OK(hipStreamSynchronize(stream));
        }
        return 0;
    }

    int reset_games(const int32_t* slots, int n) override {
        if (slots && n_eff != E.n_games) return fail("reset_games(slots): not after gaz_engine_repack (a physical slot no longer identifies a game; reset all games instead)");
        if (!slots) n_eff = E.n_games;               // every slot restarts: the launches cover all of them again
        if (slots) {
            if (n > E.n_games) return fail("reset_games: too many slots");
            HIP_OK(hipMemcpyAsync(dSlots, slots, sizeof(int32_t) * n, hipMemcpyHostToDevice, stream));
            GAZ_LAUNCH(k_reset_games<G>, n, WAVE, stream, E, (const int32_t*)dSlots, n);
        } else {
            GAZ_LAUNCH(k_reset_games<G>, E.n_games, WAVE, stream, E, (const int32_t*)nullptr, E.n_games);
        }
        HIP_OK(hipGetLastError());
        return 0;
    }

    int new_event(hipEvent_t* e) { HIP_OK(hipEventCreate(e)); ev.push_back(*e); return 0; }
    static constexpr size_t MAX_TIMING_EVENTS = 1 << 16;            // a timed run of any length holds at most this many events

    // every tree launch carries the wave's epoch, and the marks of the previous wave's evaluator pass if that pass made any (a fused launch, or
    // the test hook): DevParams::eval_done
    bool prev_marked = false;                        // the wave before this one wrote eval_done
    DevParams<G> wave_params() {
        DevParams<G> P = E; P.wave_epoch = ++fuse_epoch; P.eval_done = prev_marked ? d_evaldone : nullptr;
        if (book_entries > 0 && !E.sync_moves) P.games_budget = 1;      // opening book (book.hpp): a finished game parks in PH_HALT until k_book_start starts the next one
        return P;
    }
    void launch_wave(hipStream_t st, int g0, int g1) { const DevParams<G> P = wave_params(); prev_marked = false; launch_wave(st, g0, g1, P); }   // (callers follow with a full evaluator pass)
    void launch_wave(hipStream_t st, int g0, int g1, const DevParams<G>& E) {
        book_start(st, g0, g1, E);
        if (E.solver) { if (E.eval_symmetry) launch_wave_v<true, true>(st, g0, g1, E); else launch_wave_v<false, true>(st, g0, g1, E); return; }
        if (E.eval_symmetry) launch_wave_v<true>(st, g0, g1, E); else launch_wave_v<false>(st, g0, g1, E);
    }
    // SYM: the instantiations with the code of the random evaluation symmetry (games.hpp WithSym; same layouts, so the parameters are reinterpreted)
    // SOLVE: those with the solver's code (games.hpp WithSolve) — the plain PUCT step only: set_solver refuses every other search
    template <bool SYM, bool SOLVE = false> void launch_wave_v(hipStream_t st, int g0, int g1, const DevParams<G>& E) {
        // the small boards run four games per wavefront (PuctVariant: same records, 16-lane teams); GAZ_TREE_TEAMS=0 -> one per wave
        typedef typename SolveSel<SOLVE, typename SymSel<SYM, typename PuctVariant<G>::type>::type>::type GP;
        typedef typename SolveSel<SOLVE, typename SymSel<SYM, G>::type>::type GS;
        if constexpr (!SOLVE) {
        if (gbk > 1) {                                // (Gumbel only, no evaluation cache: gaz_engine_create refuses the rest; the register budget of k_wave_lb)
            constexpr int PER = WAVE / GP::TEAM;
            GAZ_LAUNCH(k_wave_gb<GP>, (g1 - g0 + PER - 1) / PER, WAVE, st, *reinterpret_cast<const DevParams<GP>*>(&E), GB, g0, g1);
            return;
        }
        if (lbk > 1) {                                // (PUCT only, no evaluation cache: gaz_engine_create refuses the rest)
            // one register budget for all three games (the four-games-per-wavefront one): the K-leaf step serves few games, occupancy is
            // not what limits it, and with it the step needs no scratch (Gomoku under k_wave's budget: 156 spilled VGPRs)
            constexpr int PER = WAVE / GP::TEAM;
            GAZ_LAUNCH(k_wave_lb<GP>, (g1 - g0 + PER - 1) / PER, WAVE, st, *reinterpret_cast<const DevParams<GP>*>(&E), LB, g0, g1);
            return;
        }
        if (cfg.search == GAZ_SEARCH_GUMBEL) {
            static const int gteams_env = env_int("GAZ_TREE_TEAMS", -1);
            constexpr int GPER = WAVE / GP::TEAM;
            // measured (8192 Connect4 games, n = 32, m = 7): the team build is bit-exact but SLOWER, 225 vs 185 us per launch (sequential
            // halving keeps the four games of a wave in different phases) — opt-in only (GAZ_TREE_TEAMS=1)
            if (GPER > 1 && gteams_env == 1) GAZ_LAUNCH(k_wave_gumbel_teams<GP>, (g1 - g0 + GPER - 1) / GPER, WAVE, st, *reinterpret_cast<const DevParams<GP>*>(&E), g0, g1);
            else GAZ_LAUNCH(k_wave_gumbel<GS>, g1 - g0, WAVE, st, *reinterpret_cast<const DevParams<GS>*>(&E), g0, g1);
            return;
        }
        }
        // measured (4096 Connect4 games): 66 vs 71 us per launch; with the evaluation cache (up to 8 evaluation-free simulations per
        // game and launch, and a wave is as slow as its slowest team) one game per wave stays faster: 60.1 k vs 56.2 k positions/s
        static const int teams_env = env_int("GAZ_TREE_TEAMS", -1);
        const bool teams = teams_env >= 0 ? teams_env != 0 : E.cache == nullptr;
        constexpr int PER = WAVE / GP::TEAM;
        if (PER > 1 && teams) GAZ_LAUNCH(k_wave_teams<GP>, (g1 - g0 + PER - 1) / PER, WAVE, st, *reinterpret_cast<const DevParams<GP>*>(&E), g0, g1);
        else GAZ_LAUNCH(k_wave<GS>, g1 - g0, WAVE, st, *reinterpret_cast<const DevParams<GS>*>(&E), g0, g1);
    }
    void launch_wave() { launch_wave(stream, 0, n_eff); }

    // ---- opening book (book.hpp).  While a book is set, k_book_start runs in front of every tree step — separate or fused — and starts the
    // games that wait (PH_NEW_GAME, or parked in PH_HALT under the budget of 1 that wave_params hands the tree steps); an engine without a
    // book launches nothing here, and the tree kernels are the same with and without one.  The table, the lengths and the per-entry counters are
    // one set of device arrays per book; the block behind the game_stats counters points at them.
    uint8_t* book_act = nullptr; int32_t* book_len = nullptr; unsigned long long* book_cnt = nullptr;
    static void free_book(uint8_t* a, int32_t* l, unsigned long long* c) { if (a) hipFree(a); if (l) hipFree(l); if (c) hipFree(c); }
    void book_start(hipStream_t st, int g0, int g1, const DevParams<G>& P, bool release = false) {
        if ((book_entries <= 0 && !release) || g1 <= g0) return;
        typedef typename PuctVariant<G>::type GP;
        constexpr int PER = WAVE / GP::TEAM;
        DevParams<G> B = P; B.games_budget = E.games_budget;               // the true budget: which parked slots have a next game (book_start.hpp)
        GAZ_LAUNCH(k_book_start<GP>, (g1 - g0 + PER - 1) / PER, WAVE, st, *reinterpret_cast<const DevParams<GP>*>(&B), g0, g1);
    }
    int set_opening_book(int n, int stride, int mode, const uint8_t* actions, const int32_t* lengths) override {
        typedef typename PuctVariant<G>::type GP;
        constexpr int PER = WAVE / GP::TEAM;
        uint8_t* a = nullptr; int32_t* l = nullptr; unsigned long long* c = nullptr;
        if (n > 0) {
            int32_t* d_status = nullptr;
            const size_t bytes = (size_t)n * (size_t)stride;
            if (hipMalloc((void**)&a, bytes) != hipSuccess || hipMalloc((void**)&l, sizeof(int32_t) * (size_t)n) != hipSuccess ||
                hipMalloc((void**)&c, sizeof(unsigned long long) * (size_t)n) != hipSuccess || hipMalloc((void**)&d_status, sizeof(int32_t) * (size_t)n) != hipSuccess) {
                free_book(a, l, c); if (d_status) hipFree(d_status);
                return fail("set_opening_book: out of device memory");
            }
            std::vector<int32_t> status((size_t)n, 0);
            bool ok = hipMemcpyAsync(a, actions, bytes, hipMemcpyHostToDevice, stream) == hipSuccess &&
                      hipMemcpyAsync(l, lengths, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, stream) == hipSuccess &&
                      hipMemsetAsync(c, 0, sizeof(unsigned long long) * (size_t)n, stream) == hipSuccess;
            if (ok) {
                GAZ_LAUNCH(k_book_validate<GP>, (n + PER - 1) / PER, WAVE, stream, (const uint8_t*)a, (const int32_t*)l, n, stride, (int)E.max_actions, d_status);
                ok = hipGetLastError() == hipSuccess && hipMemcpyAsync(status.data(), d_status, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, stream) == hipSuccess &&
                     hipStreamSynchronize(stream) == hipSuccess;
            }
            hipFree(d_status);
            if (!ok) { free_book(a, l, c); return fail("set_opening_book: the validation of the table failed on the device"); }
            for (int i = 0; i < n; ++i) {
                if (status[i] == BOOK_OK) continue;
                const int ply = status[i] >> 8, why = status[i] & 0xff;
                free_book(a, l, c);
                const std::string e = "set_opening_book: entry " + std::to_string(i) + ": ";
                if (why == BOOK_BAD_ILLEGAL) return fail(e + "illegal move " + std::to_string((int)actions[(size_t)i * stride + ply]) + " at ply " + std::to_string(ply));
                if (why == BOOK_BAD_OVER) return fail(e + "the game is over after ply " + std::to_string(ply) + " (a win, or a draw on a full board): a book position must have a move to search");
                return fail(e + "a length of " + std::to_string(ply) + " plies leaves no move below max_actions = " + std::to_string(E.max_actions));
            }
        }
        if (quiesce()) { free_book(a, l, c); return 1; }          // (no launch in flight reads the block or the old table while they change)
        BookBlock b{};
        b.n_entries = n; b.stride = n ? stride : 0; b.mode = n ? mode : 0; b.actions = a; b.lengths = l; b.counts = c;
        if (hipMemcpy(book_block(E.stats), &b, offsetof(BookBlock, started), hipMemcpyHostToDevice) != hipSuccess) { free_book(a, l, c); return fail("set_opening_book: hipMemcpy failed"); }
        if (n == 0 && book_entries > 0) {                           // removed: the slots parked for k_book_start go on to PH_NEW_GAME
            book_start(stream, 0, E.n_games, E, true);
            if (hipGetLastError() != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) return fail("set_opening_book: releasing the waiting games failed");
        }
        free_book(book_act, book_len, book_cnt);
        book_act = a; book_len = l; book_cnt = c; book_entries = n; book_mode = n ? mode : 0;
        return 0;
    }
    int read_book_counts(uint64_t* counts, uint64_t out[8]) override {
        for (int i = 0; i < 8; ++i) out[i] = 0;
        if (quiesce()) return 1;
        BookBlock b;
        HIP_OK(hipMemcpy(&b, book_block(E.stats), sizeof(b), hipMemcpyDeviceToHost));
        out[0] = b.started; out[1] = b.plies;
        static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the counters are copied as they are");
        if (book_entries > 0 && counts) HIP_OK(hipMemcpy(counts, book_cnt, sizeof(uint64_t) * (size_t)book_entries, hipMemcpyDeviceToHost));
        return check_device_error();
    }

    // ---- fused tree + trunk launch (resnet.hip k_wave_trunk): Connect4 PUCT with the whole-trunk ResNet evaluator, no evaluation
    // cache (its probe reads rows other teams are writing).  GAZ_FUSE_WAVE=0 -> separate launches.
    // The hand-over inside the launch is BOUNDED (trunk.hpp TrunkArgs::spin_ticks): HIP promises no dispatch order, so a trunk workgroup whose
    // games' tree block is not resident may not wait forever.  A workgroup that gives up counts itself in d_fault and — unlike the others —
    // does not mark its boards in d_evaldone; their games keep their requests pending (no result changes), and poll_fuse_fault() — at every host
    // synchronisation point — switches this engine to separate launches for good.
    uint32_t* d_done = nullptr; uint32_t* d_evaldone = nullptr; int32_t* d_fault = nullptr;
    unsigned long long* d_queue = nullptr;           // completion queue of the fused launch (DevParams::done_queue); GAZ_FUSE_QUEUE=0 -> a flag per board
    uint32_t fuse_epoch = 0; int fuse_state = -1;     // -1 not decided, 0 off, 1 on
    uint64_t fuse_faults = 0;                        // trunk workgroups that gave up waiting, over the engine's life (get_stats [13])
    unsigned debug_fault_mod = 0;                    // test hook: gaz_engine_debug_fused_fault
    static constexpr unsigned SPIN_TICKS = 2000000;  // 20 ms of the 100-MHz wall clock; a tree step takes ~0.1 ms
    int poll_fuse_fault() {                          // stream must be idle
        if (!d_fault) return 0;
        int32_t n = 0;
        HIP_OK(hipMemcpy(&n, d_fault, sizeof(n), hipMemcpyDeviceToHost));
        if (n) {
            fuse_faults += (uint64_t)n; n = 0; fuse_state = 0; debug_fault_mod = 0;      // (the test hook injects until the fault has been seen)
            fault_wave = waves_launched; fault_strikes++;
            HIP_OK(hipMemcpy(d_fault, &n, sizeof(n), hipMemcpyHostToDevice));
            fprintf(stderr, "[gaz_engine] fused tree + trunk launch: %llu trunk workgroup(s) gave up waiting for their games (dispatch order not as assumed); "
                            "falling back to separate launches%s\n", (unsigned long long)fuse_faults,
                    fault_strikes <= REARM_STRIKES ? " (the one-launch form is tried again after 20000 waves)" : " for good");
        }
        return 0;
    }
    // A give-up can be a transient — with two game groups, two launches in flight can for once hold each other's slots — and separate launches cost a
    // grouped engine a fifth of its rate: after REARM_WAVES waves without the one-launch form it is tried again, at most REARM_STRIKES times.
    int64_t waves_launched = 0, fault_wave = 0; int fault_strikes = 0;
    static constexpr int64_t REARM_WAVES = 20000; static constexpr int REARM_STRIKES = 2;
    bool can_fuse() {
        if (fuse_state == 0 && fault_strikes > 0 && fault_strikes <= REARM_STRIKES && d_queue_or_done() && waves_launched - fault_wave >= REARM_WAVES) fuse_state = 1;
        if (fuse_state >= 0) return fuse_state == 1;
        fuse_state = 0;
        if (lbk > 1) return false;                   // K rows per game: the one-launch form hands over one row per game
        static const bool off = !env_on("GAZ_FUSE_WAVE", true);
        typedef typename PuctVariant<G>::type GP;
        // with the evaluation cache too (measured 67.5 k vs 64.3 k positions/s): a team's probe reads its OWN row, and the table is
        // written by k_cache_insert between launches as before.  GAZ_FUSE_CACHE=0 -> separate launches when the cache is on
        static const bool with_cache = env_on("GAZ_FUSE_CACHE", true);
        const bool gumbel = cfg.search == GAZ_SEARCH_GUMBEL;
        // round 3: Gomoku's PUCT search as well (one game per wavefront; compacting trees are fine: a game's state lives in HBM either way).  GAZ_FUSE_GOMOKU=0 -> separate
        const bool gmk = G::ID == GAME_GMK && !gumbel && !E.cache && env_on("GAZ_FUSE_GOMOKU", true);
        const bool c4 = G::ID == GAME_C4 && WAVE / GP::TEAM >= 4 && !E.compact && !(E.cache && !with_cache);
        if (off || !(c4 || gmk) || !eval || !eval->supports_split()) return false;
        // round 3: the Gumbel search too (BASELINE configs[4]; its tree step is 17 % of a wave when launched separately).  GAZ_FUSE_GUMBEL=0 -> separate
        if (gumbel && (!env_on("GAZ_FUSE_GUMBEL", true) || E.cache)) return false;
        if (!gumbel && !env_on("GAZ_TREE_TEAMS", true)) return false;
        if (dalloc(&d_done, (size_t)E.n_games) || !ensure_skip_buffers()) return false;
        if (env_on("GAZ_FUSE_QUEUE", true) && dalloc(&d_queue, (size_t)E.n_games + 64)) return false;
        fuse_state = 1;
        return true;
    }

    bool d_queue_or_done() const { return d_done != nullptr; }      // the fused launch's buffers exist: it had been running before the fault
    bool fuse_enabled = true;
    int set_fused_wave(int on) override { fuse_enabled = on != 0; return 0; }
    bool ensure_skip_buffers() {
        if (d_evaldone) return true;
        if (dalloc(&d_evaldone, (size_t)E.n_games) || dalloc(&d_fault, 4)) return false;
        return true;
    }
    int debug_fused_fault(int mod) override {
        if (match_mode) return fail("debug_fused_fault: not while match play is on (gaz_engine_set_match runs separate launches only)");
        if (lbk > 1 && mod > 0) return fail(std::string("debug_fused_fault: ") + (gbk > 1 ? "gumbel_batch" : "leaf_batch") + " > 1 runs separate launches only");
        if (mod > 0 && !ensure_skip_buffers()) return 1;
        debug_fault_mod = mod > 0 ? (unsigned)mod : 0u;
        return 0;
    }

    // ---- repack (continuous self-play with a games_budget): towards the end of a generation more and more slots have played their
    // last game and halted, but every wave still steps and EVALUATES all n_games rows.  repack() moves the games that still run into
    // the lowest slots and shrinks every later launch (tree step, evaluator, cache insert) to them: the tail of a generation costs
    // what its live games cost.  Results do not change: a game carries its identity (slot_id) and all its state with it.
    int n_eff = 0;                                   // launches cover physical slots [0, n_eff)
    int32_t* dMoveList = nullptr;
    int repack(int32_t* n_active_out, int32_t* n_eff_out) override {
        if (E.sync_moves) return fail("repack needs continuous self-play (sync_moves = 0)");
        if (match_mode) return fail("repack: not while match play is on (gaz_engine_set_match; the routing stage covers every slot)");
        if (gbk > 1) return fail("repack: not with gumbel_batch > 1 (a game owns gumbel_batch rows of the batch)");
        if (lbk > 1) return fail("repack: not with leaf_batch > 1 (a game owns leaf_batch rows of the batch)");
        if (quiesce()) return 1;
        book_start(stream, 0, n_eff, E);             // opening book: a slot parked for its next game is no hole — start that game first
        GAZ_LAUNCH(k_gather_root<G>, E.n_games, WAVE, stream, E, dN, dW, dP, dPol, dRV, dQ, dChosen, dPhase, dPending);
        std::vector<int32_t> ph(E.n_games);
        HIP_OK(hipMemcpyAsync(ph.data(), dPhase, (size_t)E.n_games * 4, hipMemcpyDeviceToHost, stream));
        HIP_OK(hipStreamSynchronize(stream));
        int n_active = 0;
        for (int g = 0; g < n_eff; ++g) n_active += ph[g] != PH_HALT;
        for (int g = n_eff; g < E.n_games; ++g) if (ph[g] != PH_HALT) return fail("repack: a slot beyond the live range is running");
        if (n_active_out) *n_active_out = n_active;
        const int n_new = n_active > 0 ? n_active : 1;
        std::vector<int32_t> mv;
        int hole = 0;
        for (int g = n_eff - 1; g >= n_new; --g) {
            if (ph[g] == PH_HALT) continue;
            while (hole < n_new && ph[hole] != PH_HALT) ++hole;
            if (hole >= n_new) return fail("repack: internal error (no hole left)");
            mv.push_back(g); mv.push_back(hole); ph[hole] = ph[g]; ph[g] = PH_HALT;
        }
        if (!mv.empty()) {
            if (!dMoveList && dalloc(&dMoveList, (size_t)2 * E.n_games)) return 1;
            HIP_OK(hipMemcpyAsync(dMoveList, mv.data(), mv.size() * 4, hipMemcpyHostToDevice, stream));
            const size_t slot_bytes = (size_t)2 * (E.compact ? 2 : 1) * (size_t)E.nodes_per_tree * (size_t)E.node_bytes;
            const size_t gbytes = cfg.search == GAZ_SEARCH_GUMBEL ? sizeof(GumbelState<G>) : 0;
            DevParams<G> Em = E; Em.eval_done = d_evaldone;              // a game's "evaluated last wave" mark travels with it
            GAZ_LAUNCH(k_move_slots<G>, (int)(mv.size() / 2), 256, stream, Em, (const int32_t*)dMoveList, (int)(mv.size() / 2), slot_bytes, gbytes);   // one block per move
            HIP_OK(hipGetLastError());
            HIP_OK(hipStreamSynchronize(stream));
        }
        n_eff = n_new;
        if (n_eff_out) *n_eff_out = n_eff;
        return 0;
    }

    // the wave as ONE launch, tree blocks and trunk workgroups together; -1: not this wave (no plan or no kernel for this trunk variant), nothing was launched
    int fused_wave(bool timing, hipEvent_t e0, hipEvent_t e1, hipEvent_t e2) {
        // diagnostic: GAZ_FUSED_STAMPS=<file>[:n] -> wall-clock stamps of every block of the n-th fused launch (tools/fused_timeline.py)
        static const char* stamp_spec = getenv("GAZ_FUSED_STAMPS");
        static const long stamp_at = stamp_spec && strchr(stamp_spec, ':') ? atol(strchr(stamp_spec, ':') + 1) : 3000;
        unsigned long long* d_stamps = nullptr;
        const size_t stamp_blocks = (size_t)n_eff + 4096;              // >= tree blocks + trunk workgroups
        if (stamp_spec && n_waves_total == stamp_at && hipMalloc((void**)&d_stamps, stamp_blocks * 128 * 8) == hipSuccess) hipMemsetAsync(d_stamps, 0, stamp_blocks * 128 * 8, stream);
        const FuseHandoff ho{d_done, fuse_epoch + 1, d_evaldone, d_fault, SPIN_TICKS, debug_fault_mod, d_stamps, d_queue};
        const void* plan = eval->trunk_plan(E.nn_in, n_eff, 0, ho);
        if (!plan) return -1;
        if (timing) hipEventRecord(e0, stream);
        DevParams<G> Ef = wave_params(); Ef.done_flag = d_done;
        book_start(stream, 0, n_eff, Ef);
        if (eval->plan_uses_queue(plan)) {   // the trunk workgroups take queue entries: the tree blocks rank their games as they finish
            typedef typename PuctVariant<G>::type GPq;
            static const bool gumbel_teams = env_on("GAZ_FUSE_GUMBEL_TEAMS", true);
            // games per tree block = rounds x (4 waves x games per wavefront); rounds: measured, see DESIGN (GAZ_FUSE_TREE_ROUNDS overrides)
            static const int rounds_env = env_int("GAZ_FUSE_TREE_ROUNDS", 0);
            // measured on one box (tools/sweep_rounds.sh): PUCT 1 round 56.6 k positions/s, 2 rounds 54.6 k, 4: 53.8 k; Gumbel (8192 games: every slot
            // starts as a tree block) 1: 314 k, 2: 319 k, 4: 321 k, 8: 317 k
            // Gomoku as one of two game groups (tools/sweep_groups5.sh): 2: 2372, 3: 2372, 4: 2384, 6: 2357, 8: 2330 positions/s
            // Gumbel as one of two game groups of 4096 (tools/sweep_groups6.sh, sweep_groups7.sh, one box): 1: 341.3 k, 2: 344.2 k, 4: 321.4 k, 8: 247.5 k (one batch: 323.9 k)
            const int rounds = rounds_env > 0 ? rounds_env : (G::ID == GAME_GMK ? (this->grouped > 1 ? 4 : 8) : (cfg.search == GAZ_SEARCH_GUMBEL ? (this->grouped > 1 ? 2 : 4) : 1));
            const int gpb = G::ID == GAME_GMK ? rounds * 8 : rounds * 4 * ((cfg.search == GAZ_SEARCH_GUMBEL && !gumbel_teams) ? 1 : WAVE / GPq::TEAM);
            Ef.done_queue = d_queue; Ef.queue_gpb = gpb; Ef.queue_nfull = n_eff / gpb; Ef.queue_rem = n_eff % gpb;
        }
        Ef.handoff_release = G::ID == GAME_GMK;
        const bool launched = G::ID == GAME_GMK ? launch_wave_trunk_gmk(stream, &Ef, 0, n_eff, plan)
                            : cfg.search == GAZ_SEARCH_GUMBEL ? launch_wave_trunk_c4_gumbel(stream, &Ef, 0, n_eff, plan) : launch_wave_trunk_c4(stream, &Ef, 0, n_eff, plan);
        if (!launched) { fuse_state = 0; --fuse_epoch; return -1; }      // no fused kernel for this trunk variant: separate launches, for good
        prev_marked = true;                  // the trunk workgroups of this launch mark the boards they evaluate
        if (d_stamps) {
            std::vector<unsigned long long> hst(stamp_blocks * 128);
            hipStreamSynchronize(stream);
            hipMemcpy(hst.data(), d_stamps, hst.size() * 8, hipMemcpyDeviceToHost); hipFree(d_stamps);
            std::string path(stamp_spec); if (path.find(':') != std::string::npos) path = path.substr(0, path.find(':'));
            if (FILE* f = fopen(path.c_str(), "wb")) { fwrite(hst.data(), 8, hst.size(), f); fclose(f); }
        }
        if (timing) hipEventRecord(e1, stream);
        eval->forward_heads(stream, E.nn_policy, E.nn_value, n_eff, 0);
        if (E.cache) { Ef.eval_done = d_evaldone; GAZ_LAUNCH(k_cache_insert<G>, n_eff, WAVE, stream, Ef, 0, n_eff); E.cache_epoch++; }
        if (timing) {       // the fused kernel is booked as evaluator time; tree time is what it hides
            hipEventRecord(e2, stream); ev_eval.push_back({e0, e2}); n_waves_timed++;
            ev_fused.push_back({e0, e1});
        }
        n_waves_total++;
        return 0;
    }

    int one_wave(bool with_eval) {
        ++waves_launched;
        // timing brackets on every TIMING_STRIDE-th wave only: an event record is a barrier packet of its own (~5 us between two
        // kernels; five of them per wave were 4 % of the wave they measured)
        const bool timing = this->timing && n_waves_total % TIMING_STRIDE == 0 && ev.size() + 4 <= MAX_TIMING_EVENTS;
        hipEvent_t e0 = 0, e1 = 0, e2 = 0;
        if (timing && (new_event(&e0) || new_event(&e1) || new_event(&e2))) return 1;
        if (with_eval && eval && fuse_enabled && !match_mode && can_fuse()) { const int rc = fused_wave(timing, e0, e1, e2); if (rc >= 0) return rc; }
        if (timing) hipEventRecord(e0, stream);
        DevParams<G> P = wave_params();
        launch_wave(stream, 0, n_eff, P);
        prev_marked = false;                         // the separately launched evaluator pass covers every row
        if (timing) hipEventRecord(e1, stream);
        if (with_eval && eval) { if (match_mode) { if (match_forward(timing)) return 1; } else eval->forward(stream, E.nn_in, E.nn_policy, E.nn_value, n_eff * lbk, timing); }
        if (timing) { hipEventRecord(e2, stream); ev_tree.push_back({e0, e1}); ev_eval.push_back({e1, e2}); n_waves_timed++; }
        P.eval_done = nullptr;
        if (with_eval && eval && debug_fault_mod && d_evaldone) {      // test hook: this wave behaves as a fused launch with workgroups that gave up
            GAZ_LAUNCH(k_debug_skip<G>, n_eff, WAVE, stream, P, d_evaldone, n_eff, debug_fault_mod, d_fault);
            prev_marked = true; P.eval_done = d_evaldone;
        }
        if (with_eval && eval && E.cache) { GAZ_LAUNCH(k_cache_insert<G>, n_eff, WAVE, stream, P, 0, n_eff); E.cache_epoch++; }
        n_waves_total++;
        return 0;
    }

    // ---- group pipeline (free-running self-play only).  The games are split into K groups; stream `stream` carries nothing but the
    // trunk kernels trunk(g0, k), trunk(g1, k), ..., trunk(g0, k + 1) back to back — the MFMA kernel is the only thing on the critical
    // path — while the latency-bound rest runs behind it on two other streams: heads(g, k) (Dense-1 + tail, `hstream`) and the next
    // tree step tree(g, k + 1) (`tstream`) of a group overlap the trunk launches of the OTHER groups.  Group sizes are whole rounds
    // of the trunk kernel's tiles (2 workgroups x CUs x 3 boards = 1536 Connect4 boards; the last group may be the cheaper 2-board
    // tiles), so splitting costs no MFMA round.  Per-game results do not depend on the grouping: rows of a batch are independent.
    hipStream_t tstream = 0, hstream = 0;
    static constexpr int MAXGRP = 8;
    int n_grp = 0, grp0[MAXGRP + 1] = {};
    hipEvent_t ev_tree_done[2][MAXGRP] = {}, ev_trunk_done[2][MAXGRP] = {}, ev_heads_done[2][MAXGRP] = {}, ev_join = 0;
    bool pipeline_ready = false;
    // nothing of this engine is running or queued when this returns 0
    int quiesce() { HIP_OK(hipStreamSynchronize(stream)); if (pipeline_ready) { HIP_OK(hipStreamSynchronize(tstream)); HIP_OK(hipStreamSynchronize(hstream)); } return 0; }
    bool can_pipeline() {
        static const char* spec = getenv("GAZ_PIPELINE");
        if (!spec || !*spec || atoi(spec) == 0 || match_mode) return false;      // (match play: one batch, separate launches)
        // (the evaluation cache is read by tree kernels and written by k_cache_insert: they must not run concurrently)
        if (lbk > 1 || E.sync_moves || !eval || !eval->supports_split() || E.n_games < 1024 || E.cache || n_eff != E.n_games) return false;
        if (!pipeline_ready) {
            // GAZ_PIPELINE=1: groups of one full trunk round (1536 boards), remainder last; GAZ_PIPELINE=a,b,c: explicit sizes
            std::vector<int> sizes;
            if (strchr(spec, ',')) { for (const char* p = spec; *p;) { sizes.push_back(atoi(p)); p = strchr(p, ','); if (!p) break; ++p; } }
            else { const int round = eval->round_rows(); for (int left = E.n_games; left > 0; left -= round) sizes.push_back(left < round ? left : round); }
            int sum = 0; for (int v : sizes) sum += v;
            if (sizes.size() < 2 || sizes.size() > (size_t)MAXGRP || sum != E.n_games) return false;
            for (int v : sizes) if (v <= 0) return false;
            n_grp = (int)sizes.size(); grp0[0] = 0;
            for (int i = 0; i < n_grp; ++i) grp0[i + 1] = grp0[i] + sizes[i];
            int lo = 0, hi = 0;
            hipDeviceGetStreamPriorityRange(&lo, &hi);                   // the small kernels should be dispatched ahead of queued trunk tiles
            if (hipStreamCreateWithPriority(&tstream, hipStreamNonBlocking, hi) != hipSuccess) return false;
            if (hipStreamCreateWithPriority(&hstream, hipStreamNonBlocking, hi) != hipSuccess) return false;
            for (int p = 0; p < 2; ++p) for (int i = 0; i < n_grp; ++i) {
                hipEventCreateWithFlags(&ev_tree_done[p][i], hipEventDisableTiming); hipEventCreateWithFlags(&ev_trunk_done[p][i], hipEventDisableTiming);
                hipEventCreateWithFlags(&ev_heads_done[p][i], hipEventDisableTiming);
            }
            hipEventCreateWithFlags(&ev_join, hipEventDisableTiming);
            pipeline_ready = true;
        }
        return true;
    }
    int run_waves_pipelined(int n) {
        const int in_row = G::HW * G::C;
        hipEventRecord(ev_join, stream);                                 // the side streams start after everything queued on `stream`
        hipStreamWaitEvent(tstream, ev_join, 0); hipStreamWaitEvent(hstream, ev_join, 0);
        for (int k = 0; k < n; ++k) {
            const int cur = k & 1, prev = cur ^ 1;
            const bool timed = timing && n_waves_total % TIMING_STRIDE == 0 && ev.size() + 2 * (size_t)n_grp <= MAX_TIMING_EVENTS;
            const DevParams<G> P = wave_params(); prev_marked = false;    // one epoch per wave, whatever the number of groups
            for (int g = 0; g < n_grp; ++g) {
                const int g0 = grp0[g], g1 = grp0[g + 1];
                if (k > 0) hipStreamWaitEvent(tstream, ev_heads_done[prev][g], 0);      // this group's previous evaluation
                hipEvent_t t0 = 0, t1 = 0;
                if (timed) { if (new_event(&t0) || new_event(&t1)) return 1; hipEventRecord(t0, tstream); }
                launch_wave(tstream, g0, g1, P);
                if (timed) { hipEventRecord(t1, tstream); ev_tree.push_back({t0, t1}); }
                hipEventRecord(ev_tree_done[cur][g], tstream);
                hipStreamWaitEvent(stream, ev_tree_done[cur][g], 0);
                eval->forward_trunk(stream, E.nn_in + (size_t)g0 * in_row, g1 - g0, timed, g0);
                hipEventRecord(ev_trunk_done[cur][g], stream);
                hipStreamWaitEvent(hstream, ev_trunk_done[cur][g], 0);
                eval->forward_heads(hstream, E.nn_policy + (size_t)g0 * G::A, E.nn_value + g0, g1 - g0, g0);
                hipEventRecord(ev_heads_done[cur][g], hstream);
            }
            n_waves_total++; if (timed) n_waves_timed++;
        }
        // join: `stream` ends after every side-stream kernel, so synchronize() / stats reads on it see a quiescent engine
        hipEventRecord(ev_join, tstream); hipStreamWaitEvent(stream, ev_join, 0);
        for (int g = 0; g < n_grp; ++g) hipStreamWaitEvent(stream, ev_heads_done[(n - 1) & 1][g], 0);
        HIP_OK(hipGetLastError());
        return 0;
    }

    int counts(int32_t out[10]) {
        HIP_OK(hipMemsetAsync(dCount, 0, 10 * sizeof(int32_t), stream));
        GAZ_LAUNCH(k_count<G>, E.n_games, WAVE, stream, E, dCount);
        HIP_OK(hipMemcpyAsync(out, dCount, 10 * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
        HIP_OK(hipStreamSynchronize(stream));
        return 0;
    }

    int run_move(int32_t* n_waiting) override {
        if (!E.sync_moves) return fail("run_move needs sync_moves = 1");
        if (!eval) return fail("run_move needs a built-in evaluator (use wave_begin/wave_end with GAZ_EVAL_EXTERNAL)");
        if (!eval->ready()) return fail("run_move: evaluator weights not loaded (gaz_engine_load_weights)");
        if (match_mode && !(eval_b && eval_b->ready())) return fail("run_move: weights of network B not loaded (gaz_engine_load_weights_b)");
        // a move needs at most iter_limit + 2 evaluations (both roots); poll the device every 16 waves (4 with leaf batching)
        // PUCT: a move needs at most iter_limit + 2 evaluations; Gumbel can overshoot its budget (vpc >= 1 per survivor)
        const int max_waves = cfg.search == GAZ_SEARCH_GUMBEL ? 4 * (E.run_iterations + 3 * G::A) + 64
                                                             : (E.run_iterations < 3 * G::A ? 3 * G::A : E.run_iterations) + 8;
        int32_t c[10];
        const int poll = lbk > 1 ? 4 : 16;           // a K-leaf move is a few dozen launches: look more often, every launch evaluates all rows
        for (int w = 0; w < max_waves + 16; w += poll) {
            for (int i = 0; i < poll; ++i) if (one_wave(true)) return 1;
            if (counts(c)) return 1;
            if (check_device_error()) return 1;
            if (c[0] == 0) break;
        }
        if (c[0] != 0) return fail("run_move: games still searching after the wave budget");
        if (n_waiting) *n_waiting = E.n_games;
        return 0;
    }

    int get_root_stats(uint32_t* oN, float* oW, float* oP, float* oPol, uint32_t* oRV, float* oQ, int32_t* oChosen,
                       int32_t* oPhase) override {
        GAZ_LAUNCH(k_gather_root<G>, E.n_games, WAVE, stream, E, dN, dW, dP, dPol, dRV, dQ, dChosen, dPhase, dPending);
        HIP_OK(hipGetLastError());
        const size_t na = (size_t)E.n_games * G::A, n = E.n_games;
        if (oN) HIP_OK(hipMemcpyAsync(oN, dN, na * 4, hipMemcpyDeviceToHost, stream));
        if (oW) HIP_OK(hipMemcpyAsync(oW, dW, na * 4, hipMemcpyDeviceToHost, stream));
        if (oP) HIP_OK(hipMemcpyAsync(oP, dP, na * 4, hipMemcpyDeviceToHost, stream));
        if (oPol) HIP_OK(hipMemcpyAsync(oPol, dPol, na * 4, hipMemcpyDeviceToHost, stream));
        if (oRV) HIP_OK(hipMemcpyAsync(oRV, dRV, n * 4, hipMemcpyDeviceToHost, stream));
        if (oQ) HIP_OK(hipMemcpyAsync(oQ, dQ, n * 4, hipMemcpyDeviceToHost, stream));
        if (oChosen) HIP_OK(hipMemcpyAsync(oChosen, dChosen, n * 4, hipMemcpyDeviceToHost, stream));
        if (oPhase) HIP_OK(hipMemcpyAsync(oPhase, dPhase, n * 4, hipMemcpyDeviceToHost, stream));
        HIP_OK(hipStreamSynchronize(stream));
        return 0;
    }

    int apply_moves(const int32_t* moves) override {
        if (!E.sync_moves) return fail("apply_moves needs sync_moves = 1");
        if (moves) HIP_OK(hipMemcpyAsync(dMoves, moves, sizeof(int32_t) * E.n_games, hipMemcpyHostToDevice, stream));
        GAZ_LAUNCH(k_release<G>, E.n_games, WAVE, stream, E, moves ? (const int32_t*)dMoves : (const int32_t*)nullptr);
        HIP_OK(hipGetLastError());
        // run the APPLY phase (do_action, win check, prune) up to the next evaluation request
        launch_wave();
        if (eval) { if (match_mode) { if (match_forward(false)) return 1; } else eval->forward(stream, E.nn_in, E.nn_policy, E.nn_value, (int)rows, false); }
        if (eval && E.cache) { GAZ_LAUNCH(k_cache_insert<G>, E.n_games, WAVE, stream, E, 0, E.n_games); E.cache_epoch++; }
        HIP_OK(hipGetLastError());
        return check_device_error();
    }

    int run_waves(int n) override {
        if (!eval) return fail("run_waves needs a built-in evaluator");
        if (!eval->ready()) return fail("run_waves: evaluator weights not loaded (gaz_engine_load_weights)");
        if (match_mode && !(eval_b && eval_b->ready())) return fail("run_waves: weights of network B not loaded (gaz_engine_load_weights_b)");
        if (can_pipeline()) return run_waves_pipelined(n);
        for (int i = 0; i < n; ++i) if (one_wave(true)) return 1;
        HIP_OK(hipGetLastError());
        return 0;
    }

    int wave_begin() override { if (one_wave(false)) return 1; HIP_OK(hipGetLastError()); return 0; }
    int wave_end() override { return 0; }   // the next wave_begin consumes the outputs; nothing to do here

    int batch_ptrs(void** a, void** b, void** c) override {
        if (a) *a = E.nn_in; if (b) *b = E.nn_policy; if (c) *c = E.nn_value; return 0;
    }
    int batch_rows(int32_t* out) override { if (!out) return fail("batch_rows: null argument"); *out = (int32_t)rows; return 0; }
    int read_batch(int8_t* inputs, int32_t* pending) override {
        if (inputs) HIP_OK(hipMemcpyAsync(inputs, E.nn_in, rows * G::HW * G::C, hipMemcpyDeviceToHost, stream));
        if (pending) {
            if (gbk > 1) GAZ_LAUNCH(k_gather_pending_gb<G>, E.n_games, WAVE, stream, E, GB, dPending);
            else if (lbk > 1) GAZ_LAUNCH(k_gather_pending_lb<G>, E.n_games, WAVE, stream, E, lbk, dPending);
            else GAZ_LAUNCH(k_gather_root<G>, E.n_games, WAVE, stream, E, dN, dW, dP, dPol, dRV, dQ, dChosen, dPhase, dPending);
            HIP_OK(hipMemcpyAsync(pending, dPending, rows * 4, hipMemcpyDeviceToHost, stream));
        }
        HIP_OK(hipStreamSynchronize(stream));
        return check_device_error();
    }
    int read_batch_symmetry(uint8_t* sym) override {
        HIP_OK(hipMemcpyAsync(sym, E.row_sym(), rows, hipMemcpyDeviceToHost, stream));
        HIP_OK(hipStreamSynchronize(stream));
        return check_device_error();
    }
    int write_outputs(const float* policy, const float* value) override {
        HIP_OK(hipMemcpyAsync(E.nn_policy, policy, rows * G::A * 4, hipMemcpyHostToDevice, stream));
        HIP_OK(hipMemcpyAsync(E.nn_value, value, rows * 4, hipMemcpyHostToDevice, stream));
        if (E.cache) { GAZ_LAUNCH(k_cache_insert<G>, E.n_games, WAVE, stream, E, 0, E.n_games); E.cache_epoch++; }
        HIP_OK(hipStreamSynchronize(stream));
        return 0;
    }

    int evaluate(const int8_t* in, int n, float* pol, float* val, int repeats, double* ms) override {
        if (!eval) return fail("evaluate: no built-in evaluator");
        if (!eval->ready()) return fail("evaluate: evaluator weights not loaded");
        if (n <= 0 || (size_t)n > rows) return fail("evaluate: n must be in [1, " + std::to_string(rows) + "] (the rows of the evaluator batch: n_games, or n_games * leaf_batch / gumbel_batch)");
        HIP_OK(hipMemcpyAsync(E.nn_in, in, (size_t)n * G::HW * G::C, hipMemcpyHostToDevice, stream));
        CallEvent e0, e1;
        if (!e0.ok || !e1.ok) return fail("evaluate: hipEventCreate failed");
        eval->forward(stream, E.nn_in, E.nn_policy, E.nn_value, n, false);      // warm-up / the measured result
        hipEventRecord(e0.e, stream);
        for (int r = 0; r < repeats; ++r) eval->forward(stream, E.nn_in, E.nn_policy, E.nn_value, n, false);
        hipEventRecord(e1.e, stream);
        HIP_OK(hipMemcpyAsync(pol, E.nn_policy, (size_t)n * G::A * 4, hipMemcpyDeviceToHost, stream));
        HIP_OK(hipMemcpyAsync(val, E.nn_value, (size_t)n * 4, hipMemcpyDeviceToHost, stream));
        HIP_OK(hipStreamSynchronize(stream));
        float t = 0; hipEventElapsedTime(&t, e0.e, e1.e);
        if (ms) *ms = repeats > 0 ? (double)t / repeats : 0.0;
        HIP_OK(hipGetLastError());
        return 0;
    }

    // the built-in evaluator (network A) on the window's current plan: per batch a gather on the window's stream, the forward pass and
    // k_score_rows on the engine's, handed over by events; one host synchronisation at the end (ScoreState::finish)
    int score_replay(gaz_replay* w, int batch, int augment, gaz_score_totals* t, double* row_ce, double* row_ent, double* row_se, uint8_t* row_flags, double* ms) override {
        if (wave_open) return fail("score_replay: called between wave_begin and wave_end: the evaluator batch is in the caller's hands, call wave_end first");
        if (!eval) return fail("score_replay: no built-in evaluator (GAZ_EVAL_EXTERNAL): score its outputs with gaz_engine_score_outputs");
        if (!eval->ready()) return fail("score_replay: evaluator weights not loaded (gaz_engine_load_weights)");
        if (!w) return fail("score_replay: null window");
        if (w->cfg.game != cfg.game) return fail("score_replay: the window holds rows of game " + std::to_string(w->cfg.game) + ", this engine plays game " + std::to_string(cfg.game));
        if (w->cfg.device != cfg.device) return fail("score_replay: the window is on device " + std::to_string(w->cfg.device) + ", this engine on device " + std::to_string(cfg.device));
        if (!w->plan_valid) return fail("score_replay: no plan: call gaz_replay_begin_epoch (append and evict drop the plan)");
        if (batch < 1 || (size_t)batch > rows) return fail("score_replay: batch_rows must be in [1, " + std::to_string(rows) + "] (the rows of the evaluator batch), not " + std::to_string(batch));
        ScoreState* S = score_state();
        const long long M = w->plan_M;
        if (S->init() || S->ensure(batch, 0, M)) return fail(S->err);
        if (M > 0 && w->grow_outputs(batch + 8)) return fail(w->err);      // (spare rows behind a full batch, as the engine's own input buffer has spare bytes)
        const int act = ScoreState::act_of(score_mode());
        HIP_OK(hipEventRecord(S->ev_t0, stream));
        for (long long first = 0; first < M; first += batch) {
            const int n = M - first < batch ? (int)(M - first) : batch;
            if (first > 0) HIP_OK(hipStreamWaitEvent(w->stream, S->ev_scored, 0));      // the gather reuses the buffers the last batch was scored from
            if (w->sample(first, n, augment)) return fail(w->err);
            HIP_OK(hipEventRecord(S->ev_gather, w->stream));
            HIP_OK(hipStreamWaitEvent(stream, S->ev_gather, 0));
            eval->forward(stream, w->o_boards, S->d_pp, S->d_pv, n, false);
            S->launch_rows(stream, S->d_pp, S->d_pv, w->o_pol, w->o_val, n, first, act);
            HIP_OK(hipEventRecord(S->ev_scored, stream));
        }
        HIP_OK(hipGetLastError());
        if (S->finish(stream, M, score_mode(), t, row_ce, row_ent, row_se, row_flags, true, ms)) return fail(S->err);
        return check_device_error();
    }

    int read_head_features(int n, float* p, float* v, int32_t* p_row, int32_t* v_row) override {
        const float *dp = nullptr, *dv = nullptr; int pr = 0, vr = 0;
        if (!eval || !eval->head_features(&dp, &dv, &pr, &vr)) return fail("read_head_features: this evaluator keeps no head features");
        if (n < 0 || n > E.n_games) return fail("read_head_features: n must be in [0, n_games]");
        if (p_row) *p_row = pr; if (v_row) *v_row = vr;
        HIP_OK(hipStreamSynchronize(stream));
        if (p && n) HIP_OK(hipMemcpy(p, dp, (size_t)n * pr * 4, hipMemcpyDeviceToHost));
        if (v && n) HIP_OK(hipMemcpy(v, dv, (size_t)n * vr * 4, hipMemcpyDeviceToHost));
        return 0;
    }

    int record_layout(gaz_record_layout* o) override {
        o->record_bytes = RL::SIZE; o->max_T = G::MAXT; o->A = G::A; o->t_pad = G::TPAD;
        o->off_hdr = RL::OFF_HDR; o->off_actions = RL::OFF_ACT; o->off_q = RL::OFF_Q; o->off_root_visits = RL::OFF_RV;
        o->off_evals = RL::OFF_EV; o->off_policy = RL::OFF_POL; o->off_N = RL::OFF_N; o->off_W = RL::OFF_W; o->off_P = RL::OFF_P;
        o->off_move_kind = RL::OFF_MK;
        return 0;
    }

    // the two ends of a drain: the finished games waiting in the ring (the caller clamps the number to what it takes), then the n taken
    int ring_begin(uint32_t* avail) {
        HIP_OK(hipStreamSynchronize(stream));
        if (poll_fuse_fault()) return 1;            // a host synchronisation point like the others: a caller that only ever drains must still get the fallback
        uint32_t head[2];
        HIP_OK(hipMemcpy(head, E.ring_head, sizeof(head), hipMemcpyDeviceToHost));
        *avail = head[0] - ring_consumed;
        return 0;
    }
    int ring_commit(uint32_t n) { ring_consumed += n; HIP_OK(hipMemcpy(E.ring_head + 1, &ring_consumed, sizeof(uint32_t), hipMemcpyHostToDevice)); return 0; }
    int drain(void* out, int max_records, int32_t* n_out) override {
        *n_out = 0;
        if (E.ring_cap <= 0) return 0;
        uint32_t avail = 0;
        if (ring_begin(&avail)) return 1;
        if ((int)avail > max_records) avail = (uint32_t)max_records;
        for (uint32_t i = 0; i < avail; ++i) {
            const uint32_t slot = (ring_consumed + i) % (uint32_t)E.ring_cap;
            HIP_OK(hipMemcpy((uint8_t*)out + (size_t)i * RL::SIZE, E.ring + (size_t)slot * RL::SIZE, RL::SIZE, hipMemcpyDeviceToHost));
        }
        if (ring_commit(avail)) return 1;
        *n_out = (int32_t)avail;
        return check_device_error();
    }

    // ---- gaz_engine_drain_samples (samples.hpp): one staging buffer on the device [boards | policies | values] and its pinned twin on the
    // host, both grown on demand; per call one header gather, one build launch and ONE device-to-host copy, then the augmentation planes
    // are copied apart into the caller's arrays
    int32_t* dPlan = nullptr;                        // [ring_cap][SAMPLE_HDR_INTS] gathered headers + kept rows | [2][ring_cap] ring slots, row0
    uint8_t* dSamples = nullptr; uint8_t* hSamples = nullptr; size_t samples_cap = 0;
    static size_t al256(size_t n) { return (n + 255) / 256 * 256; }
    int sample_layout(gaz_sample_layout* o) override {
        o->n_aug = SampleAug<G>::N; o->state_bytes = G::HW * G::C; o->A = G::A; o->max_T = G::MAXT;
        return 0;
    }
    // the R rows of the n games of `plan` (ring slots, then row0) -> the caller's arrays.  weighted: k_build_samples_w with the counts of
    // k_sample_weights (dCounts), and the ply of every row behind the values
    int build_samples(const std::vector<int32_t>& plan, int n, int64_t R, int64_t plane_rows, int8_t* boards, float* policies, float* values,
                      bool weighted = false, uint8_t* row_ply = nullptr) {
        constexpr int SB = G::HW * G::C, NA = SampleAug<G>::N;
        const size_t off_p = al256((size_t)NA * R * SB), off_v = off_p + al256((size_t)NA * R * G::A * 4), off_rp = off_v + al256((size_t)R * 4),
                     total = off_rp + (weighted ? al256((size_t)R) : 0);
        if (total > samples_cap) {
            if (dSamples) HIP_OK(hipFree(dSamples));
            if (hSamples) HIP_OK(hipHostFree(hSamples));
            dSamples = nullptr; hSamples = nullptr;
            const size_t want = total > 2 * samples_cap ? total : 2 * samples_cap;
            samples_cap = 0;
            void* d = nullptr; void* hp = nullptr;
            HIP_OK(hipMalloc(&d, want));
            dSamples = (uint8_t*)d;
            HIP_OK(hipHostMalloc(&hp, want, 0));
            hSamples = (uint8_t*)hp; samples_cap = want;
        }
        int32_t* d_plan = dPlan + (size_t)SAMPLE_HDR_W_INTS * E.ring_cap;
        HIP_OK(hipMemcpyAsync(d_plan, plan.data(), plan.size() * 4, hipMemcpyHostToDevice, stream));
        if (weighted)
            GAZ_LAUNCH(k_build_samples_w<G>, n, SAMPLES_THREADS, stream, (const uint8_t*)E.ring, E.ring_cap, (const int32_t*)d_plan, n, (long long)R, (const uint8_t*)dCounts,
                       reinterpret_cast<int8_t*>(dSamples), reinterpret_cast<float*>(dSamples + off_p), reinterpret_cast<float*>(dSamples + off_v), dSamples + off_rp);
        else
            GAZ_LAUNCH(k_build_samples<G>, n, SAMPLES_THREADS, stream, (const uint8_t*)E.ring, E.ring_cap, (const int32_t*)d_plan, n, (long long)R,
                       reinterpret_cast<int8_t*>(dSamples), reinterpret_cast<float*>(dSamples + off_p), reinterpret_cast<float*>(dSamples + off_v));
        HIP_OK(hipGetLastError());
        HIP_OK(hipMemcpyAsync(hSamples, dSamples, weighted ? off_rp + (size_t)R : off_v + (size_t)R * 4, hipMemcpyDeviceToHost, stream));
        HIP_OK(hipStreamSynchronize(stream));
        for (int k = 0; k < NA; ++k) {
            memcpy(boards + (size_t)k * plane_rows * SB, hSamples + (size_t)k * R * SB, (size_t)R * SB);
            memcpy(policies + (size_t)k * plane_rows * G::A, hSamples + off_p + (size_t)k * R * G::A * 4, (size_t)R * G::A * 4);
        }
        memcpy(values, hSamples + off_v, (size_t)R * 4);
        if (weighted && row_ply) memcpy(row_ply, hSamples + off_rp, (size_t)R);
        return 0;
    }
    uint8_t* dCounts = nullptr; int32_t* dRows = nullptr;      // k_sample_weights: u8 [ring_cap][TPAD] rows per ply | [ring_cap][2] rows, plies without a row
    int drain_samples(int max_games, int64_t max_rows, int64_t plane_rows, int64_t row_base, int32_t* games, int8_t* boards, float* policies,
                      float* values, uint8_t* row_ply, int32_t* n_games, int64_t* n_rows, int32_t* blocked_T) override {
        *n_games = 0; *n_rows = 0; *blocked_T = 0;
        if (E.ring_cap <= 0) return 0;
        uint32_t avail = 0;
        if (ring_begin(&avail)) return 1;
        if (avail > (uint32_t)E.ring_cap) avail = (uint32_t)E.ring_cap;
        if ((int64_t)avail > (int64_t)max_games) avail = (uint32_t)(max_games > 0 ? max_games : 0);
        if (!avail) return check_device_error();
        if (!dPlan && dalloc(&dPlan, (size_t)(SAMPLE_HDR_W_INTS + 2) * E.ring_cap)) return 1;
        // weighted: the rows of a ply are a count (k_sample_weights).  Off (lambda = 0), a caller that wants the ply of every row is served by the
        // same kernels: at lambda = 0 the counts are 1 for the plies kept today and 0 for the fast ones
        const bool weighted = sw_lambda > 0.0 || row_ply != nullptr;
        const int HI = weighted ? SAMPLE_HDR_W_INTS : SAMPLE_HDR_INTS;
        if (weighted) {
            if (!dCounts && dalloc(&dCounts, (size_t)E.ring_cap * G::TPAD)) return 1;
            if (!dRows && dalloc(&dRows, (size_t)2 * E.ring_cap)) return 1;
            GAZ_LAUNCH(k_sample_weights<G>, (int)avail, SAMPLES_THREADS, stream, (const uint8_t*)E.ring, E.ring_cap, ring_consumed, (int)avail, E.key0, E.key1,
                       sw_lambda, sw_fast_factor, dCounts, dRows);
            GAZ_LAUNCH_FLAT(k_sample_headers_w<G>, (int)avail, SAMPLES_THREADS, stream, (const uint8_t*)E.ring, E.ring_cap, ring_consumed, (int)avail, (const int32_t*)dRows, dPlan);
        } else {
            GAZ_LAUNCH_FLAT(k_sample_headers<G>, (int)avail, SAMPLES_THREADS, stream, (const uint8_t*)E.ring, E.ring_cap, ring_consumed, (int)avail, dPlan);
        }
        HIP_OK(hipGetLastError());
        std::vector<int32_t> hdr((size_t)HI * avail);
        HIP_OK(hipMemcpyAsync(hdr.data(), dPlan, hdr.size() * 4, hipMemcpyDeviceToHost, stream));
        HIP_OK(hipStreamSynchronize(stream));
        int n = 0; int64_t R = 0;                    // whole games, oldest first, while their rows (the plies that were not fast searches; weighted: the counts' total) fit
        std::vector<int32_t> plan;
        for (; n < (int)avail; ++n) {
            const int32_t* h = &hdr[(size_t)HI * n];
            const int T = sample_plies<G>(h[0]), most = weighted ? sample_rows_cap<G>() : T, rows = h[4] < 0 ? 0 : (h[4] > most ? most : h[4]);
            if (R + rows > max_rows) { if (n == 0) *blocked_T = rows; break; }
            plan.push_back((int32_t)((ring_consumed + (uint32_t)n) % (uint32_t)E.ring_cap));
            games[6 * n] = T; games[6 * n + 1] = h[1]; games[6 * n + 2] = h[2]; games[6 * n + 3] = h[3];
            games[6 * n + 4] = (int32_t)(row_base + R); games[6 * n + 5] = weighted ? h[5] : T - rows;
            R += rows;
        }
        if (!n) return check_device_error();
        if (row_base + R > 0x7fffffffLL) return fail("drain_samples: more than 2^31 rows in one call");
        for (int i = 0; i < n; ++i) plan.push_back(games[6 * i + 4] - (int32_t)row_base);
        if (R > 0 && build_samples(plan, n, R, plane_rows, boards, policies, values, weighted, row_ply)) return 1;
        if (ring_commit((uint32_t)n)) return 1;
        *n_games = n; *n_rows = R;
        return check_device_error();
    }

    int get_stats(uint64_t out[16]) override {
        for (int i = 0; i < 16; ++i) out[i] = 0;
        int32_t c[10];
        if (counts(c)) return 1;
        unsigned long long s[8];
        HIP_OK(hipMemcpy(s, E.stats, sizeof(s), hipMemcpyDeviceToHost));
        for (int i = 0; i < 6; ++i) out[i] = s[i];
        memcpy(&out[6], c + 2, 8); memcpy(&out[7], c + 4, 8); memcpy(&out[8], c + 6, 8);
        out[9] = (uint64_t)n_waves_total; memcpy(&out[10], c + 8, 8);
        out[11] = pipeline_ready ? (uint64_t)n_grp : 0;
        if (poll_fuse_fault()) return 1;             // counts() synchronised the stream
        out[12] = (fuse_state == 1 && fuse_enabled && !match_mode) ? 1 : 0;
        out[13] = fuse_faults;
        if (lbk > 1 && gbk <= 1) {
            unsigned long long* d = reinterpret_cast<unsigned long long*>(dCount);
            HIP_OK(hipMemsetAsync(d, 0, sizeof(*d), stream));
            GAZ_LAUNCH(k_count_reserved<G>, E.n_games, WAVE, stream, E, d);
            HIP_OK(hipMemcpyAsync(&out[15], d, sizeof(*d), hipMemcpyDeviceToHost, stream));
            HIP_OK(hipStreamSynchronize(stream));
        }
        return check_device_error();
    }

    int synchronize() override { HIP_OK(hipStreamSynchronize(stream)); if (poll_fuse_fault()) return 1; return check_device_error(); }

    int timing_reset(int enable) override {
        HIP_OK(hipStreamSynchronize(stream));
        for (hipEvent_t e : ev) hipEventDestroy(e);
        ev.clear(); ev_tree.clear(); ev_eval.clear(); ev_fused.clear(); ev_match_pre.clear(); ev_match_gap.clear(); ev_match_post.clear(); match_sync_ms = 0; match_waves_timed = 0; n_waves_total = 0; n_waves_timed = 0; timing = enable != 0;
        if (eval) eval->timing_reset();
        return 0;
    }
    int set_position(int slot, const int32_t* actions, int n) override {
        if (n_eff != E.n_games) return fail("set_position: not after gaz_engine_repack (a physical slot no longer identifies a game)");
        if (slot < 0 || slot >= E.n_games || n < 0 || n > G::MAXT) return fail("set_position: bad slot / history length");
        // the game ends at ply max_actions (absolute plies, Self_Play.py:155-157): a longer history would never reach that cap and play on past
        // what the record and the tree arena were sized for
        if (n >= E.max_actions) return fail("set_position: a history of " + std::to_string(n) + " actions leaves no move below max_actions = " + std::to_string(E.max_actions));
        if (n > 0) HIP_OK(hipMemcpyAsync(dMoves, actions, sizeof(int32_t) * n, hipMemcpyHostToDevice, stream));   // dMoves holds >= MAXT? n_games ints
        GAZ_LAUNCH(k_set_position<G>, 1, WAVE, stream, E, slot, (const int32_t*)dMoves, n);
        HIP_OK(hipGetLastError());
        return 0;
    }
    uint8_t* dHist = nullptr; std::vector<uint8_t> hHist;
    int read_positions(int32_t* n_hist, uint8_t* hist, int stride) override {
        if (!n_hist || !hist || stride < G::MAXT) return fail("read_positions: hist must hold at least max_T actions per slot");
        if (!dHist && dalloc(&dHist, (size_t)E.n_games * G::TPAD)) return 1;
        // the device rows are TPAD apart; the caller's rows `stride` apart (bytes past TPAD are zero: no history is longer than MAXT)
        GAZ_LAUNCH(k_read_positions<G>, E.n_games, WAVE, stream, E, dPhase, dHist, G::TPAD);
        HIP_OK(hipGetLastError());
        HIP_OK(hipMemcpyAsync(n_hist, dPhase, (size_t)E.n_games * 4, hipMemcpyDeviceToHost, stream));
        if (stride == G::TPAD) HIP_OK(hipMemcpyAsync(hist, dHist, (size_t)E.n_games * stride, hipMemcpyDeviceToHost, stream));
        else {
            hHist.resize((size_t)E.n_games * G::TPAD);
            HIP_OK(hipMemcpyAsync(hHist.data(), dHist, hHist.size(), hipMemcpyDeviceToHost, stream));
        }
        HIP_OK(hipStreamSynchronize(stream));
        if (stride != G::TPAD) {
            const int row = stride < G::TPAD ? stride : G::TPAD;
            for (int g = 0; g < E.n_games; ++g) {
                memcpy(hist + (size_t)g * stride, hHist.data() + (size_t)g * G::TPAD, row);
                memset(hist + (size_t)g * stride + row, 0, (size_t)(stride - row));
            }
        }
        return 0;
    }
    // ---- gaz_engine_read_trees / gaz_engine_read_pv (tree_export.hpp).  Scratch and staging are allocated per call, from the sizes of the
    // requested trees (the queue: their TreeState::n_nodes) and of the export itself — nothing scales with n_games x nodes_per_tree.
    int read_trees(const int32_t* slots, int n, int tree, int max_depth, uint32_t min_visits, int64_t* node_first, int64_t* edge_first,
                   bool want_records, const TreePlace& place) override {
        typedef typename PuctVariant<G>::type GP;
        constexpr int PER = WAVE / GP::TEAM;
        node_first[0] = 0; edge_first[0] = 0;
        if (n == 0) { HIP_OK(hipStreamSynchronize(stream)); return 0; }
        const DevParams<GP>& EP = *reinterpret_cast<const DevParams<GP>*>(&E);
        CallScratch cs;
        int32_t* d_slots = cs.get<int32_t>(n); int32_t* d_cap = cs.get<int32_t>(n);
        long long* d_qfirst = cs.get<long long>((size_t)n + 1); long long* d_counts = cs.get<long long>((size_t)2 * n);
        if (!d_slots || !d_cap || !d_qfirst || !d_counts) return fail("read_trees: out of device memory");
        HIP_OK(hipMemcpyAsync(d_slots, slots, sizeof(int32_t) * n, hipMemcpyHostToDevice, stream));
        GAZ_LAUNCH_FLAT(k_tree_caps<G>, n, 256, stream, E, (const int32_t*)d_slots, n, tree, d_cap);
        HIP_OK(hipGetLastError());
        std::vector<int32_t> cap(n);
        HIP_OK(hipMemcpyAsync(cap.data(), d_cap, sizeof(int32_t) * n, hipMemcpyDeviceToHost, stream));
        HIP_OK(hipStreamSynchronize(stream));
        std::vector<long long> first((size_t)n + 1, 0);
        for (int i = 0; i < n; ++i) first[i + 1] = first[i] + cap[i];
        ExportQ* d_queue = cs.get<ExportQ>((size_t)first[n]);
        if (!d_queue) return fail("read_trees: out of device memory");
        HIP_OK(hipMemcpyAsync(d_qfirst, first.data(), sizeof(long long) * ((size_t)n + 1), hipMemcpyHostToDevice, stream));
        TreeExportArgs X; memset(&X, 0, sizeof(X));
        X.slots = d_slots; X.n_slots = n; X.tree = tree; X.max_depth = max_depth; X.min_visits = min_visits;
        X.queue = d_queue; X.q_first = d_qfirst; X.counts = d_counts;
        GAZ_LAUNCH((k_tree_export<GP, false>), (n + PER - 1) / PER, WAVE, stream, EP, X);
        HIP_OK(hipGetLastError());
        std::vector<long long> counts((size_t)2 * n);
        HIP_OK(hipMemcpyAsync(counts.data(), d_counts, sizeof(long long) * 2 * (size_t)n, hipMemcpyDeviceToHost, stream));
        HIP_OK(hipStreamSynchronize(stream));
        std::vector<long long> nf((size_t)n + 1, 0), ef((size_t)n + 1, 0);
        for (int i = 0; i < n; ++i) { nf[i + 1] = nf[i] + counts[2 * i]; ef[i + 1] = ef[i] + counts[2 * i + 1]; }
        for (int i = 0; i <= n; ++i) { node_first[i] = nf[i]; edge_first[i] = ef[i]; }
        if (!want_records) return 0;
        gaz_tree_node* nodes = nullptr; gaz_tree_edge* edges = nullptr;
        if (place(nf[n], ef[n], &nodes, &edges)) return 1;
        if (nf[n] == 0) return 0;
        long long* d_nf = cs.get<long long>((size_t)n + 1); long long* d_ef = cs.get<long long>((size_t)n + 1);
        gaz_tree_node* d_nodes = cs.get<gaz_tree_node>((size_t)nf[n]); gaz_tree_edge* d_edges = cs.get<gaz_tree_edge>((size_t)ef[n]);
        if (!d_nf || !d_ef || !d_nodes || !d_edges) return fail("read_trees: out of device memory");
        HIP_OK(hipMemcpyAsync(d_nf, nf.data(), sizeof(long long) * ((size_t)n + 1), hipMemcpyHostToDevice, stream));
        HIP_OK(hipMemcpyAsync(d_ef, ef.data(), sizeof(long long) * ((size_t)n + 1), hipMemcpyHostToDevice, stream));
        X.node_first = d_nf; X.edge_first = d_ef; X.nodes = d_nodes; X.edges = d_edges;
        GAZ_LAUNCH((k_tree_export<GP, true>), (n + PER - 1) / PER, WAVE, stream, EP, X);
        HIP_OK(hipGetLastError());
        HIP_OK(hipMemcpyAsync(nodes, d_nodes, sizeof(gaz_tree_node) * (size_t)nf[n], hipMemcpyDeviceToHost, stream));
        if (ef[n]) HIP_OK(hipMemcpyAsync(edges, d_edges, sizeof(gaz_tree_edge) * (size_t)ef[n], hipMemcpyDeviceToHost, stream));
        HIP_OK(hipStreamSynchronize(stream));
        return 0;
    }
    int read_pv(int tree, const int32_t* first_action, int max_len, uint8_t* actions, uint32_t* N, float* W, int32_t* len) override {
        typedef typename PuctVariant<G>::type GP;
        constexpr int PER = WAVE / GP::TEAM;
        const size_t n = (size_t)E.n_games, cells = n * (size_t)max_len;
        CallScratch cs;
        int32_t* d_first = first_action ? cs.get<int32_t>(n) : nullptr;
        uint8_t* d_act = cs.get<uint8_t>(cells); uint32_t* d_N = cs.get<uint32_t>(cells); float* d_W = cs.get<float>(cells); int32_t* d_len = cs.get<int32_t>(n);
        if ((first_action && !d_first) || !d_act || !d_N || !d_W || !d_len) return fail("read_pv: out of device memory");
        if (first_action) HIP_OK(hipMemcpyAsync(d_first, first_action, sizeof(int32_t) * n, hipMemcpyHostToDevice, stream));
        HIP_OK(hipMemsetAsync(d_act, 0, cells, stream)); HIP_OK(hipMemsetAsync(d_N, 0, cells * 4, stream)); HIP_OK(hipMemsetAsync(d_W, 0, cells * 4, stream));
        GAZ_LAUNCH(k_tree_pv<GP>, (E.n_games + PER - 1) / PER, WAVE, stream, *reinterpret_cast<const DevParams<GP>*>(&E), tree, (const int32_t*)d_first, max_len,
                   d_act, d_N, d_W, d_len);
        HIP_OK(hipGetLastError());
        HIP_OK(hipMemcpyAsync(actions, d_act, cells, hipMemcpyDeviceToHost, stream));
        HIP_OK(hipMemcpyAsync(N, d_N, cells * 4, hipMemcpyDeviceToHost, stream));
        HIP_OK(hipMemcpyAsync(W, d_W, cells * 4, hipMemcpyDeviceToHost, stream));
        HIP_OK(hipMemcpyAsync(len, d_len, n * 4, hipMemcpyDeviceToHost, stream));
        HIP_OK(hipStreamSynchronize(stream));
        return 0;
    }
    int start_search() override { GAZ_LAUNCH(k_start_search<G>, E.n_games, WAVE, stream, E); HIP_OK(hipGetLastError()); return 0; }
    int stop_search(int stop) override { E.stop_search = stop != 0; return 0; }
    // tau != 0 and tau <= 5e-3 -> 0 (MCTS.py:116-120,163-168); negative = Self_Play's schedule
    static double norm_tau(double tau) { return tau < 0.0 ? -1.0 : ((tau != 0.0 && tau <= 5e-3) ? 0.0 : tau); }
    int set_search_params(int run_iterations, int tau_mode) override {
        if (run_iterations > 0) E.run_iterations = run_iterations;
        E.tau = tau_mode < 0 ? -1.0 : (double)tau_mode;
        return 0;
    }
    int init_puct_table() {
        double* tb = const_cast<double*>(E.puct_table);
        GAZ_LAUNCH_FLAT(k_init_puct_table<0>, PUCT_TABLE_N, 256, stream, tb, E.c_init, E.c_base, PUCT_TABLE_N);
        HIP_OK(hipGetLastError());
        return 0;
    }
    // MCTS.update_hyperparams (MCTS.py:134-168: invalid values are ignored with a warning there, rejected here) and
    // MCTS_Gumbel.update_hyperparams (MCTS_Gumbel.py:186-210); kernels read DevParams per launch, so the next wave sees them
    int set_hyperparams(const gaz_search_hyperparams* hp) override {
        if (!hp || hp->struct_size != sizeof(gaz_search_hyperparams)) return fail("set_hyperparams: struct_size does not match this library's gaz_search_hyperparams");
        auto given = [](double v) { return v == v; };
        if (given(hp->c_puct_init) && hp->c_puct_init < 0.0) return fail("c_puct_init cannot be negative");
        if (given(hp->c_puct_base) && hp->c_puct_base <= 0.0) return fail("c_puct_base must be positive");
        if (given(hp->dirichlet_alpha) && hp->dirichlet_alpha <= 0.0) return fail("dirichlet_alpha must be positive");
        if (given(hp->dirichlet_epsilon) && (hp->dirichlet_epsilon < 0.0 || hp->dirichlet_epsilon >= 1.0)) return fail("dirichlet_epsilon must be in [0, 1)");
        if (hp->gumbel_m >= 0 && cfg.search == GAZ_SEARCH_GUMBEL && hp->gumbel_m < 2) return fail("Gumbel search needs m >= 2");
        // the node arena was sized at create time from run_iterations (and gumbel_m): a larger value now could only end in ERR_ARENA_FULL in
        // the middle of a search, so it is refused here with the remedy
        if (cfg.nodes_per_tree <= 0) {
            const int it = hp->run_iterations > 0 ? hp->run_iterations : E.run_iterations, m = hp->gumbel_m >= 0 ? hp->gumbel_m : E.gumbel_m;
            const long long need = nodes_needed(it, m);
            if (need > E.nodes_per_tree)
                return fail("set_hyperparams: run_iterations / gumbel_m beyond what the tree arena was sized for at create time (" + std::to_string(E.nodes_per_tree) +
                            " nodes per tree, " + std::to_string(need) + " needed): create the engine with the largest values, or give nodes_per_tree");
        }
        bool table = false;
        if (given(hp->c_puct_init)) { E.c_init = hp->c_puct_init; table = true; }
        if (given(hp->c_puct_base)) { E.c_base = hp->c_puct_base; table = true; }
        if (given(hp->dirichlet_alpha)) E.alpha = (double)(float)hp->dirichlet_alpha;
        if (given(hp->dirichlet_epsilon)) { E.eps = hp->dirichlet_epsilon; E.one_minus_eps = (float)(1.0 - hp->dirichlet_epsilon); }
        if (hp->use_dirichlet >= 0) E.use_dirichlet = hp->use_dirichlet != 0;
        if (given(hp->tau)) E.tau = norm_tau(hp->tau);
        if (hp->gumbel_m >= 0) E.gumbel_m = hp->gumbel_m;
        if (given(hp->c_visit)) E.c_visit = hp->c_visit;
        if (given(hp->c_scale)) E.c_scale = hp->c_scale;
        if (hp->run_iterations > 0) E.run_iterations = hp->run_iterations;
        if (table && E.puct_table) return init_puct_table();
        return 0;
    }
    // resignation (resign.hpp): the parameters go to the block behind the game_stats counters, which PH_APPLY reads once per move, so the
    // next wave sees them.  The block's counters live as long as the engine, through off and on again
    ResignBlock* resign_block() { return reinterpret_cast<ResignBlock*>(E.stats + RESIGN_STATS_OFFSET); }
    int set_resignation(const gaz_resign_params* p) override {
        ResignBlock b{};                             // (threshold 0 = off: the other fields are then not looked at, on the device either)
        if (p->threshold > 0.0) { b.threshold = p->threshold; b.no_resign_prob = p->no_resign_prob; b.consecutive = p->consecutive; b.min_ply = p->min_ply; }
        if (quiesce()) return 1;                     // (no launch in flight reads the block while it changes)
        HIP_OK(hipMemcpy(resign_block(), &b, offsetof(ResignBlock, stats), hipMemcpyHostToDevice));
        return 0;
    }
    int get_resign_stats(uint64_t out[8]) override {
        for (int i = 0; i < 8; ++i) out[i] = 0;
        if (quiesce()) return 1;
        unsigned long long s[8];
        HIP_OK(hipMemcpy(s, resign_block()->stats, sizeof(s), hipMemcpyDeviceToHost));
        for (int i = 0; i < 7; ++i) out[i] = s[i];
        return check_device_error();
    }
    // random board symmetry per evaluator request (puct_core.hpp eval_sym_draw): kernels take DevParams by value per launch, so rows encoded
    // from the next launch on follow the mode; rows in flight are answered under the byte they were encoded with (DevParams::row_sym)
    // The kernels with the symmetry code (games.hpp WithSym) are launched from the first time the mode is 1, and from then on for good: rows encoded
    // under a symmetry may be in flight when the mode goes back to 0, and only those kernels read a row's byte
    // (DevParams::eval_symmetry: bit 0 = the mode, bit 1 = those kernels are in use)
    int set_eval_symmetry(int32_t mode) override { E.eval_symmetry = (mode ? 1 : 0) | ((mode || E.eval_symmetry) ? 2 : 0); return 0; }
    int get_eval_symmetry(int32_t* mode) override { *mode = E.eval_symmetry & 1; return 0; }
    // solver (puct_core.hpp "MCTS-Solver"): like the symmetry, the kernels with its code (games.hpp WithSolve) are launched from the first time the
    // mode is 1 and from then on for good — the tag bits they wrote into child words stay in the trees, and only those kernels take an index through
    // child_index().  (DevParams::solver: bit 0 = the mode, bit 1 = those kernels are in use.)  Switching on tags the edges into the terminal parents
    // made while it was off (k_solver_retag): a terminal parent's status is derived from its record, whenever it was made.
    unsigned long long* d_solver_ctr = nullptr;
    int set_solver(int32_t mode) override {
        if (cfg.search == GAZ_SEARCH_GUMBEL && gbk > 1) return fail("set_solver: not with gumbel_batch > 1 (the solver proves in the PUCT tree; the Gumbel search is the follow-up)");
        if (cfg.search == GAZ_SEARCH_GUMBEL) return fail("set_solver: not with the Gumbel search (the solver proves in the PUCT tree)");
        if (lbk > 1) return fail("set_solver: not with leaf_batch > 1 (a proof may not stand on leaves in flight)");
        if (E.nodes_per_tree > CHILD_INDEX_MASK) return fail("set_solver: nodes_per_tree must be below 2^29 (two bits of a child word carry the proof)");
        if (mode && !(E.solver & 1)) {
            if (quiesce()) return 1;
            if (!d_solver_ctr) {
                if (dalloc(&d_solver_ctr, 8)) return 1;
                E.solver_ctr_lo = (uint32_t)(uintptr_t)d_solver_ctr; E.solver_ctr_hi = (uint32_t)((uint64_t)(uintptr_t)d_solver_ctr >> 32);
            }
            GAZ_LAUNCH(k_solver_retag<G>, E.n_games, WAVE, stream, E);
            HIP_OK(hipGetLastError());
            HIP_OK(hipStreamSynchronize(stream));
        }
        E.solver = (mode ? 1 : 0) | ((mode || E.solver) ? 2 : 0);
        return 0;
    }
    int get_solver(int32_t* mode) override { *mode = E.solver & 1; return 0; }
    int get_solver_stats(uint64_t out[8]) override {
        for (int i = 0; i < 8; ++i) out[i] = 0;
        if (quiesce()) return 1;
        if (d_solver_ctr) {
            unsigned long long s[8];
            HIP_OK(hipMemcpy(s, d_solver_ctr, sizeof(s), hipMemcpyDeviceToHost));
            for (int i = 0; i < 8; ++i) out[i] = s[i];
        }
        return check_device_error();
    }
    // ---- match play (match.hpp): the games of this engine are played by two networks.  Network A = eval, network B =
    // eval_b, a second instance of the same evaluator; the network of a row is a function of the game state (match_network), so the mode takes
    // effect at the next evaluator pass and needs no migration.  With the mode on, the evaluator pass of one_wave / apply_moves is match_forward:
    // launches are separate (no fused launch, no group pipeline) and the host waits once per wave for the two row counts.
    int match_mode = 0; uint32_t match_salt_b = 0;
    Evaluator* eval_b = nullptr;
    uint8_t* m_net = nullptr; unsigned long long* m_blk = nullptr; uint32_t* m_cnt = nullptr; uint32_t* h_match_cnt = nullptr;
    int32_t* m_idx_a = nullptr; int32_t* m_idx_b = nullptr;
    int8_t* m_in_a = nullptr; int8_t* m_in_b = nullptr; float* m_pol_a = nullptr; float* m_pol_b = nullptr; float* m_val_a = nullptr; float* m_val_b = nullptr;
    // timing (gaz_engine_timing_reset(1)), on the waves the other brackets are taken on: route + partition + copy; the stream's idle gap from the
    // end of the copy to the first launch after the host's wait; the scatter; and the host's time inside that wait
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_match_pre, ev_match_gap, ev_match_post;
    double match_sync_ms = 0; int64_t match_waves_timed = 0;
    uint64_t match_stats[5] = {0, 0, 0, 0, 0};       // rows of A, rows of B, waves without a row for A, for B, evaluator passes with the mode on
    // why this engine cannot play a match ("" = it can): the routing stage owns one row per game and one batch
    std::string match_fault(const char* fn) const {
        const std::string f = std::string(fn) + ": ";
        if (cfg.single_tree) return f + "not with single_tree = 1 (one tree searches for both players: a request has no owner)";
        if (cfg.leaf_batch > 1) return f + "not with leaf_batch > 1 (a game owns leaf_batch rows of the batch; match play routes one row per game)";
        if (cfg.gumbel_batch > 1) return f + "not with gumbel_batch > 1 (a game owns gumbel_batch rows of the batch; match play routes one row per game)";
        if (cfg.eval_cache_log2 > 0) return f + "not with eval_cache_log2 > 0 (the evaluation cache does not know which network answered an entry)";
        return "";
    }
    int ensure_match_buffers() {
        if (m_net) return 0;
        const size_t n = (size_t)E.n_games, nblk = (n + WAVE - 1) / WAVE;
        if (dalloc(&m_blk, nblk) || dalloc(&m_cnt, 2) || dalloc(&m_idx_a, n) || dalloc(&m_idx_b, n) ||
            dalloc(&m_in_a, n * G::HW * G::C + 64) || dalloc(&m_in_b, n * G::HW * G::C + 64) || dalloc(&m_pol_a, n * G::A + 64) || dalloc(&m_pol_b, n * G::A + 64) ||
            dalloc(&m_val_a, n + 64) || dalloc(&m_val_b, n + 64)) return 1;
        void* h = nullptr;
        HIP_OK(hipHostMalloc(&h, 2 * sizeof(uint32_t)));
        h_match_cnt = (uint32_t*)h;
        return dalloc(&m_net, n);                    // (last: its pointer says that all of them exist)
    }
    int ensure_eval_b() {
        if (eval_b || cfg.evaluator == GAZ_EVAL_EXTERNAL) return 0;
        std::string e2;
        gaz_engine_config ecfg = cfg; ecfg.n_games = (int32_t)rows; ecfg.hash_salt = match_salt_b;
        eval_b = make_evaluator(ecfg, G::H, G::W, G::C, G::A, &e2);
        return eval_b ? 0 : fail("evaluator of network B: " + e2);
    }
    void match_route() {
        const int nblk = (E.n_games + WAVE - 1) / WAVE;
        GAZ_LAUNCH(k_match_route<G>, nblk, WAVE, stream, (const GameState<G>*)E.games, E.n_games, cfg.search == GAZ_SEARCH_GUMBEL ? 1 : 0, m_net, m_blk);
    }
    // the evaluator pass of a wave with the mode on, over all rows (n_eff == n_games: repack is refused)
    int match_forward(bool timing) {
        const int n = E.n_games, nblk = (n + WAVE - 1) / WAVE;
        hipEvent_t m[5] = {0, 0, 0, 0, 0};
        const bool timed = timing && ev.size() + 5 <= MAX_TIMING_EVENTS;
        if (timed) { for (hipEvent_t& e : m) if (new_event(&e)) return 1; hipEventRecord(m[0], stream); }
        match_route();
        GAZ_LAUNCH(k_match_pack<G>, nblk, WAVE, stream, (const uint8_t*)m_net, (const unsigned long long*)m_blk, n, m_idx_a, m_idx_b, m_cnt);
        HIP_OK(hipMemcpyAsync(h_match_cnt, m_cnt, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        GAZ_LAUNCH_FLAT(k_match_copy<G>, n * MatchRow<G>::UNITS, 256, stream, (const int8_t*)E.nn_in, (const int32_t*)m_idx_a, (const int32_t*)m_idx_b,
                        (const uint32_t*)m_cnt, n, m_in_a, m_in_b);
        if (timed) hipEventRecord(m[1], stream);
        const auto t0 = std::chrono::steady_clock::now();
        HIP_OK(hipStreamSynchronize(stream));        // the host must know the two grid sizes
        if (timed) { match_sync_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); hipEventRecord(m[2], stream); }
        const int na = (int)h_match_cnt[0], nb = (int)h_match_cnt[1];
        if (na < 0 || nb < 0 || na + nb > n) return fail("match play: internal error (row counts " + std::to_string(na) + " + " + std::to_string(nb) + " of " + std::to_string(n) + " rows)");
        match_stats[0] += (uint64_t)na; match_stats[1] += (uint64_t)nb; match_stats[2] += na == 0; match_stats[3] += nb == 0; match_stats[4] += 1;
        if (na) eval->forward(stream, m_in_a, m_pol_a, m_val_a, na, timing);
        if (nb) eval_b->forward(stream, m_in_b, m_pol_b, m_val_b, nb, timing);
        if (timed) hipEventRecord(m[3], stream);
        if (na + nb) GAZ_LAUNCH_FLAT(k_match_scatter<G>, (na + nb) * (G::A + 1), 256, stream, (const int32_t*)m_idx_a, (const int32_t*)m_idx_b, na, nb,
                                     (const float*)m_pol_a, (const float*)m_val_a, (const float*)m_pol_b, (const float*)m_val_b, E.nn_policy, E.nn_value);
        if (timed) { hipEventRecord(m[4], stream); ev_match_pre.push_back({m[0], m[1]}); ev_match_gap.push_back({m[1], m[2]}); ev_match_post.push_back({m[3], m[4]}); match_waves_timed++; }
        HIP_OK(hipGetLastError());
        return 0;
    }
    int get_match_timing(double out[8]) override {
        for (int i = 0; i < 8; ++i) out[i] = 0;
        HIP_OK(hipStreamSynchronize(stream));
        const std::vector<std::pair<hipEvent_t, hipEvent_t>>* v[3] = {&ev_match_pre, &ev_match_gap, &ev_match_post};
        for (int k = 0; k < 3; ++k) for (auto& pr : *v[k]) { float a = 0; hipEventElapsedTime(&a, pr.first, pr.second); out[k] += a; }
        out[3] = match_sync_ms; out[4] = (double)match_waves_timed;
        return 0;
    }
    int set_match(int32_t mode, uint32_t hash_salt_b) override {
        if (!mode) { match_mode = 0; return 0; }
        if (const std::string f = match_fault("set_match"); !f.empty()) return fail(f);
        if (n_eff != E.n_games) return fail("set_match: not after gaz_engine_repack (the routing stage covers every slot; reset all games first)");
        if (debug_fault_mod) return fail("set_match: not while gaz_engine_debug_fused_fault is armed");
        if (quiesce()) return 1;
        if (cfg.evaluator == GAZ_EVAL_HASH && eval_b && hash_salt_b != match_salt_b) { delete eval_b; eval_b = nullptr; }
        match_salt_b = hash_salt_b;
        if (ensure_match_buffers() || ensure_eval_b()) return 1;
        match_mode = 1;
        return 0;
    }
    int get_match(int32_t* mode) override { *mode = match_mode; return 0; }
    int load_weights_b(const gaz_tensor* t, int n) override {
        if (const std::string f = match_fault("load_weights_b"); !f.empty()) return fail(f);
        if (!eval) return fail("load_weights_b: no evaluator to load weights into");
        if (quiesce() || ensure_eval_b()) return 1;
        std::string m;
        if (eval_b->load(t, n, stream, &m)) return fail("load_weights_b: " + m);
        return 0;
    }
    int read_batch_network(uint8_t* net) override {
        if (const std::string f = match_fault("read_batch_network"); !f.empty()) return fail(f);
        if (ensure_match_buffers()) return 1;
        match_route();
        HIP_OK(hipMemcpyAsync(net, m_net, (size_t)E.n_games, hipMemcpyDeviceToHost, stream));
        HIP_OK(hipStreamSynchronize(stream));
        return check_device_error();
    }
    int get_match_stats(uint64_t out[8]) override {
        for (int i = 0; i < 8; ++i) out[i] = i < 5 ? match_stats[i] : 0;
        return 0;
    }

    int8_t* pr_board = nullptr; uint8_t* pr_legal = nullptr; int32_t* pr_winner = nullptr; int8_t* pr_input = nullptr; int32_t* pr_term = nullptr;
    int32_t* pr_actions = nullptr; int32_t* pr_n = nullptr; float* pr_pin = nullptr; float* pr_pout = nullptr; int pr_cap = 0, pr_stride = 0;
    int probe_rules(const int32_t* actions, const int32_t* n_actions, int n_pos, int stride, int8_t* o_board, uint8_t* o_legal,
                    int32_t* o_winner, int8_t* o_input, int32_t* o_term, const float* policy_in, float* o_policy) override {
        if (n_pos <= 0 || stride <= 0 || stride > G::MAXT || !actions || !n_actions) return fail("probe_rules: bad arguments");
        for (int p = 0; p < n_pos; ++p) {
            if (n_actions[p] < 0 || n_actions[p] > stride) return fail("probe_rules: history longer than stride");
            for (int i = 0; i < n_actions[p]; ++i) { const int a = actions[(size_t)p * stride + i]; if (a < 0 || a >= G::A) return fail("probe_rules: action out of range"); }
        }
        if (n_pos > pr_cap || stride > pr_stride) {                      // scratch grows, never shrinks (freed with the engine)
            const size_t n = (size_t)n_pos, st = (size_t)G::MAXT;
            if (dalloc(&pr_board, n * G::HW) || dalloc(&pr_legal, n * G::A) || dalloc(&pr_winner, n) || dalloc(&pr_input, n * G::HW * G::C) ||
                dalloc(&pr_term, n * G::A) || dalloc(&pr_actions, n * st) || dalloc(&pr_n, n) || dalloc(&pr_pin, n * G::A) || dalloc(&pr_pout, n * G::A)) return 1;
            pr_cap = n_pos; pr_stride = G::MAXT;
        }
        const size_t n = (size_t)n_pos;
        HIP_OK(hipMemcpyAsync(pr_actions, actions, n * stride * 4, hipMemcpyHostToDevice, stream));
        HIP_OK(hipMemcpyAsync(pr_n, n_actions, n * 4, hipMemcpyHostToDevice, stream));
        const bool pol = policy_in && o_policy;
        if (pol) HIP_OK(hipMemcpyAsync(pr_pin, policy_in, n * G::A * 4, hipMemcpyHostToDevice, stream));
        GAZ_LAUNCH(k_probe_rules<G>, n_pos, WAVE, stream, E, (const int32_t*)pr_actions, (const int32_t*)pr_n, n_pos, stride, pr_board, pr_legal,
                   pr_winner, pr_input, pr_term, pol ? (const float*)pr_pin : (const float*)nullptr, pol ? pr_pout : (float*)nullptr);
        HIP_OK(hipGetLastError());
        if (o_board) HIP_OK(hipMemcpyAsync(o_board, pr_board, n * G::HW, hipMemcpyDeviceToHost, stream));
        if (o_legal) HIP_OK(hipMemcpyAsync(o_legal, pr_legal, n * G::A, hipMemcpyDeviceToHost, stream));
        if (o_winner) HIP_OK(hipMemcpyAsync(o_winner, pr_winner, n * 4, hipMemcpyDeviceToHost, stream));
        if (o_input) HIP_OK(hipMemcpyAsync(o_input, pr_input, n * G::HW * G::C, hipMemcpyDeviceToHost, stream));
        if (o_term) HIP_OK(hipMemcpyAsync(o_term, pr_term, n * G::A * 4, hipMemcpyDeviceToHost, stream));
        if (pol) HIP_OK(hipMemcpyAsync(o_policy, pr_pout, n * G::A * 4, hipMemcpyDeviceToHost, stream));
        HIP_OK(hipStreamSynchronize(stream));
        return 0;
    }
    // gaz_engine_probe_det (det_probe.hpp): every count an item carries is checked here, so that no kernel indexes past its arrays
    uint64_t* pd_in = nullptr; uint64_t* pd_out = nullptr; size_t pd_in_cap = 0, pd_out_cap = 0;
    int probe_det(int op, int n, const uint64_t* in, int in_words, uint64_t* out, int out_words) override {
        const bool whole = (op & DP_WHOLE_WAVE) != 0;
        const int code = op & ~DP_WHOLE_WAVE;
        DetProbeOp d;
        if (!det_probe_op(code, &d)) return fail("probe_det: unknown op " + std::to_string(op));
        if (n <= 0 || n > (1 << 22) || in_words <= 0 || out_words <= 0 || in_words > 4096 || out_words > 4096 || !in || !out) return fail("probe_det: bad arguments");
        if (!d.team) {
            if (whole) return fail("probe_det: DP_WHOLE_WAVE goes with the team ops only");
            if (in_words != d.in || out_words != d.out) return fail("probe_det: op " + std::to_string(code) + " takes " + std::to_string(d.in) + " words per item and gives " + std::to_string(d.out));
        } else {
            const uint64_t limit = (code == DP_SUM_F32 || code == DP_SUM_F64) ? (uint64_t)DP_SUM_MAX : (uint64_t)G::A;
            for (int i = 0; i < n; ++i) {
                const uint64_t ni = in[(size_t)i * in_words];
                if (ni < 1 || ni > limit) return fail("probe_det: item " + std::to_string(i) + " has n outside 1.." + std::to_string(limit));
                const int nf = ni < 8 ? 8 : (int)ni;
                if (in_words < d.in + d.in_per * nf || out_words < d.out + d.out_per * (int)ni) return fail("probe_det: item " + std::to_string(i) + " does not fit its words");
            }
        }
        const size_t bi = (size_t)n * in_words, bo = (size_t)n * out_words;
        if (bi > pd_in_cap) { if (dalloc(&pd_in, bi)) return 1; pd_in_cap = bi; }        // scratch grows, never shrinks (freed with the engine)
        if (bo > pd_out_cap) { if (dalloc(&pd_out, bo)) return 1; pd_out_cap = bo; }
        HIP_OK(hipMemcpyAsync(pd_in, in, bi * 8, hipMemcpyHostToDevice, stream));
        HIP_OK(hipMemsetAsync(pd_out, 0, bo * 8, stream));
        typedef typename PuctVariant<G>::type GP;
        constexpr int PER = WAVE / GP::TEAM;
        if (!d.team) GAZ_LAUNCH(k_probe_det<G>, (n + WAVE - 1) / WAVE, WAVE, stream, E, code, n, (const uint64_t*)pd_in, in_words, pd_out, out_words);
        else if (PER > 1 && !whole) GAZ_LAUNCH(k_probe_det_teams<GP>, (n + PER - 1) / PER, WAVE, stream, *reinterpret_cast<const DevParams<GP>*>(&E), code, n, (const uint64_t*)pd_in, in_words, pd_out, out_words);
        else GAZ_LAUNCH(k_probe_det_wave<G>, n, WAVE, stream, E, code, n, (const uint64_t*)pd_in, in_words, pd_out, out_words);
        HIP_OK(hipGetLastError());
        HIP_OK(hipMemcpyAsync(out, pd_out, bo * 8, hipMemcpyDeviceToHost, stream));
        HIP_OK(hipStreamSynchronize(stream));
        return 0;
    }
    int dominant(char* name, int cap, double* flops) override {
        // positions per evaluator launch; the pipelined run launches the trunk kernel once per group: price the MEAN launch (the
        // timing sums all launches, so FLOPs per launch x launches = FLOPs of the waves either way)
        const int n_launch = can_pipeline() ? E.n_games / n_grp : E.n_games;
        double f = 0; const char* k = eval ? eval->dominant_kernel(n_launch, &f) : "";
        if (eval && can_pipeline()) { double fa = 0; eval->dominant_kernel(E.n_games, &fa); f = fa / n_grp; }
        std::string label = k;
        if (fuse_state == 1 && fuse_enabled && !match_mode) label = "k_wave_trunk = " + label + " FUSED with the " + std::string(cfg.search == GAZ_SEARCH_GUMBEL ? "Gumbel" : "PUCT") + " tree step of the same wave (one launch: tree blocks first, trunk workgroups start on the "
                                     "boards whose games are done; the launch duration therefore includes the part of the tree step it could not hide)";
        if (name && cap > 0) { strncpy(name, label.c_str(), cap - 1); name[cap - 1] = 0; }
        if (flops) *flops = f;
        return 0;
    }
    int timing_get(double* ms_tree, double* ms_eval, double* ms_dom, int64_t* n_dom, int64_t* n_waves) override {
        HIP_OK(hipStreamSynchronize(stream));
        double t = 0, e = 0;
        for (auto& pr : ev_tree) { float a = 0; hipEventElapsedTime(&a, pr.first, pr.second); t += a; }
        for (auto& pr : ev_eval) { float b = 0; hipEventElapsedTime(&b, pr.first, pr.second); e += b; }
        if (ms_tree) *ms_tree = t; if (ms_eval) *ms_eval = e;
        double d = 0; int64_t nd = 0;
        if (eval) eval->timing_get(&d, &nd);
        for (auto& pr : ev_fused) { float a = 0; hipEventElapsedTime(&a, pr.first, pr.second); d += a; nd++; }
        if (ms_dom) *ms_dom = d; if (n_dom) *n_dom = nd; if (n_waves) *n_waves = n_waves_timed;
        return 0;
    }
};

// ------------------------------------------------------------------------------------------ game groups
// gaz_engine_config::game_groups: the games of ONE engine handle as K independent engines (groups of consecutive slots), each with its own
// stream, batch and fused tree + trunk launch, stepped alternately by run_waves.  Nothing of a game depends on how games are grouped — RNG streams
// and records are keyed by the GLOBAL slot (slot_offset + slot), rows of an evaluator batch are independent bit for bit — so every game is the one
// a single engine plays (tests: records equal by (slot, game_seq)); only the order in which finished games reach the ring differs.
// Why: a wave of one engine is tree step -> trunk -> heads in sequence; in the one-launch form the trunk workgroups still wait ~60 us for their
// first boards, the last round of tiles leaves slots idle and the heads (Dense-1 + tail, ~27 us) run on a nearly empty chip.  With TWO launches
// of half the games in flight, the other group's trunk tiles fill all of that: Connect4 headline config, steady state, one box: 7.84 M -> 8.60 M
// evaluations/s with 2048 | 2048 (2560 | 1536: 8.14 M; 3072 | 1024: 7.19 M; three groups 7.73 M; four 7.1 M;
// 8-lane teams = half the tree blocks: +0.5 %, within noise, not kept).  Gomoku 2048 games -> 2 x 1024: +6 % (+8.6 % with four tree rounds per block).
// Gumbel 8192 -> 2 x 4096 with two tree rounds per block: +6 %.  auto = 2 for Connect4 PUCT + ResNet from 3072 games, Gomoku PUCT + ResNet from
// 2048 games, Connect4 Gumbel + ResNet from 6144 games.
static gaz_engine* make_single_engine(const gaz_engine_config& cfg, std::string* err) {
    if (*err = config_fault(cfg, 1); !err->empty()) return nullptr;
    gaz_engine* h = nullptr;
    switch (cfg.game) {
        case GAZ_GAME_TICTACTOE: h = new EngineT<Game<GAME_TTT>>(); break;
        case GAZ_GAME_CONNECT4: h = new EngineT<Game<GAME_C4>>(); break;
        default: h = new EngineT<Game<GAME_GMK>>(); break;
    }
    h->cfg = cfg; h->cfg.game_groups = 1;
    if (h->init()) { *err = h->err; delete h; return nullptr; }
    return h;
}

struct GroupEngine : gaz_engine {
    std::vector<gaz_engine*> kid;
    std::vector<int> first;                          // first[c] = first slot of group c, first[K] = n_games
    gaz_record_layout lay{};
    gaz_sample_layout slay{};
    int drain_from = 0;
    ~GroupEngine() override { for (gaz_engine* k : kid) delete k; }
    int K() const { return (int)kid.size(); }
    int size_of(int c) const { return first[c + 1] - first[c]; }
    int rows_of(int c, int n) const { return n - first[c] < 0 ? 0 : (n - first[c] > size_of(c) ? size_of(c) : n - first[c]); }      // of the first n rows, group c's
    int up(gaz_engine* k, int rc) { if (rc) err = k->err; return rc; }
    template <class F> int each(F f) { for (int c = 0; c < K(); ++c) if (up(kid[c], f(kid[c], c))) return 1; return 0; }
    // the three plain ways a call reaches the groups: the same call on every group, on the first only (what all groups share), eight counters summed
    template <class... P, class... A> int all(int (gaz_engine::*f)(P...), A... a) { return each([&](gaz_engine* k, int) { return (k->*f)(a...); }); }
    template <class... P, class... A> int lead(int (gaz_engine::*f)(P...), A... a) { return up(kid[0], (kid[0]->*f)(a...)); }
    int sum8(int (gaz_engine::*f)(uint64_t*), uint64_t out[8]) {
        for (int i = 0; i < 8; ++i) out[i] = 0;
        return each([&](gaz_engine* k, int) { uint64_t s[8]; if ((k->*f)(s)) return 1; for (int i = 0; i < 8; ++i) out[i] += s[i]; return 0; });
    }
    int group_of(int slot) const { int c = 0; while (c + 1 < K() && slot >= first[c + 1]) ++c; return c; }

    int init() override {
        const int n = cfg.n_games, k = cfg.game_groups;
        if (const std::string fault = config_fault(cfg, k); !fault.empty()) return fail(fault);
        first.assign(1, 0);
        for (int c = 0; c < k; ++c) first.push_back(first.back() + n / k + (c < n % k ? 1 : 0));
        for (int c = 0; c < k; ++c) {
            gaz_engine_config cc = cfg;
            cc.n_games = size_of(c); cc.slot_offset = cfg.slot_offset + (uint32_t)first[c];
            if (cfg.ring_capacity > 0) cc.ring_capacity = (int32_t)(((int64_t)cfg.ring_capacity * cc.n_games + n - 1) / n);
            // with another group's trunk tiles filling the chip, the tail of a group's tree step costs less than the rows that carry no request:
            // two groups, headline config, one box (tools/sweep_groups.sh): 8: 66.8 k, 12: 67.5 k, 16: 67.4 k positions/s (one batch: 8, see EngineT::init)
            if (cfg.max_tree_sims_per_wave == 0 && cfg.game == GAZ_GAME_CONNECT4 && cfg.search == GAZ_SEARCH_PUCT && cfg.evaluator == GAZ_EVAL_RESNET) cc.max_tree_sims_per_wave = 12;
            if (cfg.games_budget > 0) {
                // one engine: slot g plays its k-th game iff k n + g < budget, i.e. floor(budget / n) games and one more in the first budget % n slots;
                // the group's own rule (k n_c + g_c < budget_c) gives exactly those games with this budget
                const int64_t whole = cfg.games_budget / n, extra = cfg.games_budget % n - first[c];
                cc.games_budget = whole * cc.n_games + (extra < 0 ? 0 : (extra > cc.n_games ? cc.n_games : extra));
            }
            std::string e;
            gaz_engine* h = make_single_engine(cc, &e);
            if (!h) return fail("game group " + std::to_string(c) + ": " + e);
            h->grouped = k; h->note_grouped();
            kid.push_back(h);
        }
        return lead(&gaz_engine::record_layout, &lay) || lead(&gaz_engine::sample_layout, &slay);
    }
    int load_weights(const gaz_tensor* t, int n) override { return all(&gaz_engine::load_weights, t, n); }
    int reset_games(const int32_t* slots, int n) override {
        if (!slots) return all(&gaz_engine::reset_games, nullptr, 0);
        std::vector<std::vector<int32_t>> per(K());
        for (int i = 0; i < n; ++i) {
            if (slots[i] < 0 || slots[i] >= cfg.n_games) return fail("reset_games: slot out of range");
            const int c = group_of(slots[i]); per[c].push_back(slots[i] - first[c]);
        }
        return each([&](gaz_engine* k, int c) { return per[c].empty() ? 0 : k->reset_games(per[c].data(), (int)per[c].size()); });
    }
    int run_move(int32_t* w) override { return lead(&gaz_engine::run_move, w); }             // (sync_moves = 0: the group's own refusal)
    int apply_moves(const int32_t* m) override { return lead(&gaz_engine::apply_moves, m); }
    int get_root_stats(uint32_t* N, float* W, float* P, float* pol, uint32_t* rv, float* q, int32_t* chosen, int32_t* phase) override {
        return each([&](gaz_engine* k, int c) {
            const size_t a = (size_t)first[c] * lay.A, g = (size_t)first[c];
            return k->get_root_stats(N ? N + a : N, W ? W + a : W, P ? P + a : P, pol ? pol + a : pol, rv ? rv + g : rv, q ? q + g : q, chosen ? chosen + g : chosen, phase ? phase + g : phase);
        });
    }
    int run_waves(int n) override {                  // wave by wave, group by group: every group's stream always holds work
        for (int i = 0; i < n; ++i) if (all(&gaz_engine::run_waves, 1)) return 1;
        return 0;
    }
    int no_batch() { return fail("game groups hold one evaluator batch each: the wave_begin / batch API needs game_groups = 1"); }
    int wave_begin() override { return no_batch(); }
    int wave_end() override { return no_batch(); }
    int batch_ptrs(void**, void**, void**) override { return no_batch(); }
    int read_batch(int8_t*, int32_t*) override { return no_batch(); }
    int read_batch_symmetry(uint8_t*) override { return fail("read_batch_symmetry: game groups hold one evaluator batch each, like read_batch it needs game_groups = 1"); }
    int batch_rows(int32_t*) override { return no_batch(); }
    int write_outputs(const float*, const float*) override { return no_batch(); }
    // rows [first[c], first[c + 1]) go through group c's evaluator (and stay in ITS head-feature buffers: read_head_features below); ms: the sum
    int evaluate(const int8_t* in, int n, float* p, float* v, int rep, double* ms) override {
        if (n < 1 || n > cfg.n_games) return fail("evaluate: n must be in [1, n_games]");
        const size_t row = (size_t)slay.state_bytes;
        double total = 0;
        if (each([&](gaz_engine* k, int c) {
                const int nc = rows_of(c, n);
                double m = 0;
                if (nc && k->evaluate(in + (size_t)first[c] * row, nc, p ? p + (size_t)first[c] * lay.A : p, v ? v + first[c] : v, rep, &m)) return 1;
                total += m; return 0;
            })) return 1;
        if (ms) *ms = total;
        return 0;
    }
    int record_layout(gaz_record_layout* o) override { *o = lay; return 0; }
    int drain(void* out, int max_records, int32_t* n_out) override {
        int total = 0;
        for (int i = 0; i < K() && total < max_records; ++i) {       // start with another group every call: no ring starves behind a small max_records
            gaz_engine* k = kid[(drain_from + i) % K()];
            int32_t got = 0;
            if (up(k, k->drain((uint8_t*)out + (size_t)total * lay.record_bytes, max_records - total, &got))) return 1;
            total += got;
        }
        drain_from = (drain_from + 1) % K();
        *n_out = total;
        return 0;
    }
    int sample_layout(gaz_sample_layout* o) override { *o = slay; return 0; }
    int drain_samples(int max_games, int64_t max_rows, int64_t plane_rows, int64_t row_base, int32_t* games, int8_t* boards, float* policies,
                      float* values, uint8_t* row_ply, int32_t* n_games, int64_t* n_rows, int32_t* blocked_T) override {
        const gaz_sample_layout& sl = slay;
        int total = 0, blocked = 0; int64_t rows = 0;
        for (int i = 0; i < K() && total < max_games; ++i) {         // children append at the running game / row offset
            gaz_engine* k = kid[(drain_from + i) % K()];
            int32_t got = 0, b = 0; int64_t r = 0;
            if (up(k, k->drain_samples(max_games - total, max_rows - rows, plane_rows, row_base + rows, games + (size_t)6 * total, boards + (size_t)rows * sl.state_bytes,
                                       policies + (size_t)rows * sl.A, values + rows, row_ply ? row_ply + rows : row_ply, &got, &r, &b))) return 1;
            if (b && !blocked) blocked = b;
            total += got; rows += r;
        }
        drain_from = (drain_from + 1) % K();
        *n_games = total; *n_rows = rows; *blocked_T = total ? 0 : blocked;
        return 0;
    }
    int set_sample_weighting(double lambda, double fast_factor) override {
        sw_lambda = lambda; sw_fast_factor = fast_factor;
        return all(&gaz_engine::set_sample_weighting, lambda, fast_factor);
    }
    int get_stats(uint64_t out[16]) override {
        for (int i = 0; i < 16; ++i) out[i] = 0;
        out[12] = 1;
        for (int c = 0; c < K(); ++c) {
            uint64_t s[16];
            if (up(kid[c], kid[c]->get_stats(s))) return 1;
            if (s[0] > out[0]) out[0] = s[0];        // game_stats[0] = the LONGEST game (atomic_max on the device), as parallel.reduce_stats
            for (int i = 1; i < 9; ++i) out[i] += s[i];
            out[10] += s[10]; out[13] += s[13];
            if (s[9] > out[9]) out[9] = s[9];        // waves: every group has run the same number
            if (!s[12]) out[12] = 0;                 // one launch per wave: only if every group runs it
        }
        out[14] = (uint64_t)K();
        return 0;
    }
    int synchronize() override { return all(&gaz_engine::synchronize); }
    int timing_reset(int en) override { return all(&gaz_engine::timing_reset, en); }
    // sums over the groups: per wave (of all groups) the kernel time of every group's launches — they overlap in time, so the sum is NOT wall clock
    int timing_get(double* ms_tree, double* ms_eval, double* ms_dom, int64_t* n_dom, int64_t* n_waves) override {
        double t = 0, e = 0, d = 0; int64_t nd = 0, nw = 0;
        for (int c = 0; c < K(); ++c) {
            double a = 0, b = 0, x = 0; int64_t y = 0, z = 0;
            if (up(kid[c], kid[c]->timing_get(&a, &b, &x, &y, &z))) return 1;
            t += a; e += b; d += x; nd += y; if (z > nw) nw = z;
        }
        if (ms_tree) *ms_tree = t; if (ms_eval) *ms_eval = e; if (ms_dom) *ms_dom = d; if (n_dom) *n_dom = nd; if (n_waves) *n_waves = nw;
        return 0;
    }
    int dominant(char* name, int cap, double* flops) override { return lead(&gaz_engine::dominant, name, cap, flops); }      // per launch of one group
    int set_position(int slot, const int32_t* a, int n) override {
        if (slot < 0 || slot >= cfg.n_games) return fail("set_position: bad slot / history length");
        const int c = group_of(slot);
        return up(kid[c], kid[c]->set_position(slot - first[c], a, n));
    }
    int set_search_params(int it, int tau) override { return all(&gaz_engine::set_search_params, it, tau); }
    int stop_search(int s) override { return all(&gaz_engine::stop_search, s); }
    int start_search() override { return all(&gaz_engine::start_search); }
    int set_hyperparams(const gaz_search_hyperparams* hp) override { return all(&gaz_engine::set_hyperparams, hp); }
    int set_resignation(const gaz_resign_params* p) override { return all(&gaz_engine::set_resignation, p); }
    int set_eval_symmetry(int32_t mode) override { return all(&gaz_engine::set_eval_symmetry, mode); }
    int get_eval_symmetry(int32_t* mode) override { return lead(&gaz_engine::get_eval_symmetry, mode); }
    int set_solver(int32_t mode) override { return all(&gaz_engine::set_solver, mode); }
    int get_solver(int32_t* mode) override { return lead(&gaz_engine::get_solver, mode); }
    int get_solver_stats(uint64_t out[8]) override { return sum8(&gaz_engine::get_solver_stats, out); }
    int get_resign_stats(uint64_t out[8]) override { return sum8(&gaz_engine::get_resign_stats, out); }
    // every group keeps a copy of the book (and validates it: the same table, the same verdict); the per-entry counters are summed
    int set_opening_book(int n, int stride, int mode, const uint8_t* actions, const int32_t* lengths) override {
        if (all(&gaz_engine::set_opening_book, n, stride, mode, actions, lengths)) return 1;
        book_entries = n; book_mode = n ? mode : 0;
        return 0;
    }
    int read_book_counts(uint64_t* counts, uint64_t out[8]) override {
        for (int i = 0; i < 8; ++i) out[i] = 0;
        for (int i = 0; i < book_entries && counts; ++i) counts[i] = 0;
        std::vector<uint64_t> part((size_t)(book_entries > 0 ? book_entries : 1));
        return each([&](gaz_engine* k, int) {
            uint64_t s[8];
            if (k->read_book_counts(counts ? part.data() : nullptr, s)) return 1;
            for (int i = 0; i < 8; ++i) out[i] += s[i];
            for (int i = 0; i < book_entries && counts; ++i) counts[i] += part[i];
            return 0;
        });
    }
    int read_head_features(int n, float* p, float* v, int32_t* p_row, int32_t* v_row) override {
        if (n < 0 || n > cfg.n_games) return fail("read_head_features: n must be in [0, n_games]");
        int32_t pr = 0, vr = 0;
        if (lead(&gaz_engine::read_head_features, 0, nullptr, nullptr, &pr, &vr)) return 1;
        if (p_row) *p_row = pr; if (v_row) *v_row = vr;
        return each([&](gaz_engine* k, int c) {
            const int nc = rows_of(c, n);
            return nc ? k->read_head_features(nc, p ? p + (size_t)first[c] * pr : p, v ? v + (size_t)first[c] * vr : v, nullptr, nullptr) : 0;
        });
    }
    int set_fused_wave(int on) override { return all(&gaz_engine::set_fused_wave, on); }
    int debug_fused_fault(int mod) override { return all(&gaz_engine::debug_fused_fault, mod); }
    int read_positions(int32_t* n_hist, uint8_t* hist, int stride) override {
        if (!n_hist || !hist || stride < lay.max_T) return fail("read_positions: hist must hold at least max_T actions per slot");
        return each([&](gaz_engine* k, int c) { return k->read_positions(n_hist + first[c], hist + (size_t)first[c] * stride, stride); });
    }
    // the slots of every group in ONE call of that group, into staging arrays of the group's own size; the trees are then placed at the caller's positions
    int read_trees(const int32_t* slots, int n, int tree, int max_depth, uint32_t min_visits, int64_t* node_first, int64_t* edge_first,
                   bool want_records, const TreePlace& place) override {
        std::vector<std::vector<int32_t>> local(K()), pos(K());
        for (int i = 0; i < n; ++i) { const int c = group_of(slots[i]); local[c].push_back(slots[i] - first[c]); pos[c].push_back(i); }
        std::vector<std::vector<int64_t>> nf(K()), ef(K());
        std::vector<std::vector<gaz_tree_node>> tn(K()); std::vector<std::vector<gaz_tree_edge>> te(K());
        std::vector<int64_t> cn((size_t)n, 0), ce((size_t)n, 0);
        for (int c = 0; c < K(); ++c) {
            const int m = (int)local[c].size();
            nf[c].assign((size_t)m + 1, 0); ef[c].assign((size_t)m + 1, 0);
            const TreePlace stage = [&, c](int64_t nn, int64_t ne, gaz_tree_node** pn, gaz_tree_edge** pe) {
                tn[c].resize((size_t)nn + 1); te[c].resize((size_t)ne + 1); *pn = tn[c].data(); *pe = te[c].data(); return 0;
            };
            if (up(kid[c], kid[c]->read_trees(local[c].data(), m, tree, max_depth, min_visits, nf[c].data(), ef[c].data(), want_records, stage))) return 1;
            for (int j = 0; j < m; ++j) { cn[pos[c][j]] = nf[c][j + 1] - nf[c][j]; ce[pos[c][j]] = ef[c][j + 1] - ef[c][j]; }
        }
        node_first[0] = 0; edge_first[0] = 0;
        for (int i = 0; i < n; ++i) { node_first[i + 1] = node_first[i] + cn[i]; edge_first[i + 1] = edge_first[i] + ce[i]; }
        if (!want_records) return 0;
        gaz_tree_node* nodes = nullptr; gaz_tree_edge* edges = nullptr;
        if (place(node_first[n], edge_first[n], &nodes, &edges)) return 1;
        for (int c = 0; c < K(); ++c)
            for (size_t j = 0; j < pos[c].size(); ++j) {
                const int i = pos[c][j];
                if (cn[i]) memcpy(nodes + node_first[i], tn[c].data() + nf[c][j], sizeof(gaz_tree_node) * (size_t)cn[i]);
                if (ce[i]) memcpy(edges + edge_first[i], te[c].data() + ef[c][j], sizeof(gaz_tree_edge) * (size_t)ce[i]);
            }
        return 0;
    }
    int read_pv(int tree, const int32_t* fa, int max_len, uint8_t* actions, uint32_t* N, float* W, int32_t* len) override {
        return each([&](gaz_engine* k, int c) {
            const size_t o = (size_t)first[c] * (size_t)max_len;
            return k->read_pv(tree, fa ? fa + first[c] : fa, max_len, actions + o, N + o, W + o, len + first[c]);
        });
    }
    int repack(int32_t* n_active, int32_t* n_launch) override {      // every group packs its own live games; the sums are reported
        int32_t a = 0, l = 0;
        if (each([&](gaz_engine* k, int) { int32_t x = 0, y = 0; if (k->repack(&x, &y)) return 1; a += x; l += y; return 0; })) return 1;
        if (n_active) *n_active = a; if (n_launch) *n_launch = l;
        return 0;
    }
    // match play routes the rows of ONE batch to two evaluators: an engine that resolved to game groups refuses it
    int no_match(const char* fn) { return fail(std::string(fn) + ": this engine runs " + std::to_string(K()) + " game groups; match play needs one batch: create the engine with game_groups = 1"); }
    int set_match(int32_t mode, uint32_t) override { return mode ? no_match("set_match") : 0; }
    int get_match(int32_t* mode) override { *mode = 0; return 0; }
    int load_weights_b(const gaz_tensor*, int) override { return no_match("load_weights_b"); }
    int read_batch_network(uint8_t*) override { return no_match("read_batch_network"); }
    int get_match_stats(uint64_t out[8]) override { for (int i = 0; i < 8; ++i) out[i] = 0; return 0; }
    int get_match_timing(double out[8]) override { for (int i = 0; i < 8; ++i) out[i] = 0; return 0; }
    int probe_rules(const int32_t* actions, const int32_t* n_actions, int n_pos, int stride, int8_t* b, uint8_t* l, int32_t* w, int8_t* in, int32_t* t,
                    const float* pin, float* pout) override { return lead(&gaz_engine::probe_rules, actions, n_actions, n_pos, stride, b, l, w, in, t, pin, pout); }
    int probe_det(int op, int n, const uint64_t* in, int iw, uint64_t* out, int ow) override { return lead(&gaz_engine::probe_det, op, n, in, iw, out, ow); }
};

// auto (game_groups = 0): two groups where that was measured to pay (see above; measured at num_filters = 128 only, so other widths run one group); GAZ_GAME_GROUPS overrides the automatic choice only
static int choose_game_groups(const gaz_engine_config& c) {
    if (c.game_groups != 0) return c.game_groups;
    if (c.leaf_batch > 1 || c.gumbel_batch > 1) return 1;   // K rows per game: one batch
    static const int env = env_int("GAZ_GAME_GROUPS", 0);
    if (env > 0) return group_fault(c, env) ? 1 : env;
    // (with the evaluation cache every group has a table of its own — nothing is shared between groups: 108.2 k -> 110.2 k positions/s)
    const bool pays = c.game == GAZ_GAME_CONNECT4 && c.search == GAZ_SEARCH_PUCT && c.evaluator == GAZ_EVAL_RESNET && c.net_blocks > 0 && c.net_filters == 128 && c.n_games >= 3072;
    // Gomoku (2048 games, 10 blocks; the one-launch wave needs the cache off): 2195 -> 2330 positions/s, 2384 with four tree rounds per block
    // (EngineT::one_wave); from empty boards 1706 -> 1855.  Three groups 2225.  Its heads are a chain of small kernels (~300 us of a 3000-us wave)
    // that one batch runs on an idle chip
    const bool pays_gmk = c.game == GAZ_GAME_GOMOKU && c.search == GAZ_SEARCH_PUCT && c.evaluator == GAZ_EVAL_RESNET && c.net_blocks > 0 && c.net_filters == 128 && c.eval_cache_log2 == 0 && c.n_games >= 2048;
    // Gumbel (8192 games -> 2 x 4096, two tree rounds per block instead of four): 323.9 k -> 344.1 k positions/s same box (with four rounds: -1 %)
    const bool pays_gumbel = c.game == GAZ_GAME_CONNECT4 && c.search == GAZ_SEARCH_GUMBEL && c.evaluator == GAZ_EVAL_RESNET && c.net_blocks > 0 && c.net_filters == 128 && c.eval_cache_log2 == 0 && c.n_games >= 6144;
    return (pays || pays_gmk || pays_gumbel) && !group_fault(c, 2) ? 2 : 1;
}

// ------------------------------------------------------------------------------------------ C ABI
extern "C" {

int gaz_engine_abi_version(void) { return GAZ_ENGINE_ABI_VERSION; }
int gaz_engine_config_size(void) { return (int)sizeof(gaz_engine_config); }

int gaz_engine_create(const gaz_engine_config* cfg, gaz_engine** out) {
    if (!cfg || !out) { g_create_error = "null argument"; return 1; }
    *out = nullptr;
    if (cfg->struct_size != sizeof(gaz_engine_config)) {
        g_create_error = "gaz_engine_config.struct_size is " + std::to_string(cfg->struct_size) + ", this library's gaz_engine_config has " +
                         std::to_string(sizeof(gaz_engine_config)) + " bytes (ABI version " + std::to_string(GAZ_ENGINE_ABI_VERSION) +
                         "): rebuild the binding from include/gaz_engine.h";
        return 1;
    }
    const int groups = choose_game_groups(*cfg);
    if (groups <= 1) {
        gaz_engine* h = make_single_engine(*cfg, &g_create_error);
        if (!h) return 1;
        *out = h;
        return 0;
    }
    GroupEngine* h = new GroupEngine();
    h->cfg = *cfg; h->cfg.game_groups = groups;
    if (h->init()) { g_create_error = h->err; delete h; return 1; }
    *out = h;
    return 0;
}
void gaz_engine_destroy(gaz_engine* h) { delete h; }
const char* gaz_engine_last_error(gaz_engine* h) { return h ? h->err.c_str() : g_create_error.c_str(); }
int gaz_engine_load_weights(gaz_engine* h, const gaz_tensor* t, int32_t n) { return h->load_weights(t, n); }
int gaz_engine_reset_games(gaz_engine* h, const int32_t* slots, int32_t n) { return h->reset_games(slots, n); }
int gaz_engine_run_move(gaz_engine* h, int32_t* n_waiting) { return h->run_move(n_waiting); }
int gaz_engine_get_root_stats(gaz_engine* h, uint32_t* N, float* W, float* P, float* pol, uint32_t* rv, float* q, int32_t* chosen,
                              int32_t* phase) { return h->get_root_stats(N, W, P, pol, rv, q, chosen, phase); }
int gaz_engine_apply_moves(gaz_engine* h, const int32_t* moves) { return h->apply_moves(moves); }
int gaz_engine_run_waves(gaz_engine* h, int32_t n) { return h->run_waves(n); }
int gaz_engine_wave_begin(gaz_engine* h) { const int rc = h->wave_begin(); if (!rc) h->wave_open = true; return rc; }
int gaz_engine_wave_end(gaz_engine* h) { h->wave_open = false; return h->wave_end(); }
int gaz_engine_batch_ptrs(gaz_engine* h, void** a, void** b, void** c) { return h->batch_ptrs(a, b, c); }
int gaz_engine_read_batch(gaz_engine* h, int8_t* in, int32_t* pending) { return h->read_batch(in, pending); }
int gaz_engine_batch_rows(gaz_engine* h, int32_t* rows) { return h->batch_rows(rows); }
int gaz_engine_write_outputs(gaz_engine* h, const float* p, const float* v) { return h->write_outputs(p, v); }
int gaz_engine_evaluate(gaz_engine* h, const int8_t* in, int32_t n, float* p, float* v, int32_t repeats, double* ms) { return h->evaluate(in, n, p, v, repeats, ms); }
int gaz_engine_record_layout(gaz_engine* h, gaz_record_layout* o) { return h->record_layout(o); }
int gaz_engine_drain_finished(gaz_engine* h, void* out, int32_t max_records, int32_t* n_out) { return h->drain(out, max_records, n_out); }
int gaz_engine_sample_layout(gaz_engine* h, gaz_sample_layout* o) { return o ? h->sample_layout(o) : h->fail("sample_layout: null argument"); }
int gaz_engine_drain_samples2(gaz_engine* h, int32_t max_games, int64_t max_rows, int32_t* games, int8_t* boards, float* policies, float* values,
                              uint8_t* row_ply, int32_t* n_games, int64_t* n_rows) {
    if (!games || !boards || !policies || !values || !n_games || !n_rows) return h->fail("drain_samples: null argument");
    if (max_games < 0 || max_rows < 0) return h->fail("drain_samples: max_games and max_rows must be >= 0");
    int32_t blocked = 0;
    if (h->drain_samples(max_games, max_rows, max_rows, 0, games, boards, policies, values, row_ply, n_games, n_rows, &blocked)) return 1;
    if (*n_games == 0 && blocked)
        return h->fail("drain_samples: the oldest finished game has " + std::to_string(blocked) + " rows, max_rows is " + std::to_string(max_rows) +
                       (h->sw_lambda > 0.0 ? " (no game was taken: call again with room for at least 2 * max_T rows)"
                                           : " (no game was taken: call again with room for at least max_T rows)"));
    return 0;
}
int gaz_engine_drain_samples(gaz_engine* h, int32_t max_games, int64_t max_rows, int32_t* games, int8_t* boards, float* policies, float* values,
                             int32_t* n_games, int64_t* n_rows) {
    return gaz_engine_drain_samples2(h, max_games, max_rows, games, boards, policies, values, nullptr, n_games, n_rows);
}
// policy surprise weighting of the training rows (samples.hpp): lambda = 0 is off (a new engine), legal at any time, read by the next drain
int gaz_engine_set_sample_weighting(gaz_engine* h, double lambda, double fast_factor) {
    if (h->cfg.search == GAZ_SEARCH_GUMBEL)
        return h->fail("set_sample_weighting: not with the Gumbel search (the surprise is taken against the priors of a PUCT root; a Gumbel record's policy is not a visit distribution over them)");
    if (!(lambda >= 0.0 && lambda <= 1.0)) return h->fail("set_sample_weighting: lambda must be in [0, 1] (0 = off), not " + std::to_string(lambda));
    if (!(fast_factor > 0.0) || fast_factor > 1.7976931348623157e308)
        return h->fail("set_sample_weighting: fast_factor must be a finite number above 0, not " + std::to_string(fast_factor));
    return h->set_sample_weighting(lambda, fast_factor);
}
int gaz_engine_get_sample_weighting(gaz_engine* h, double* lambda, double* fast_factor) {
    if (!lambda || !fast_factor) return h->fail("get_sample_weighting: null argument");
    *lambda = h->sw_lambda; *fast_factor = h->sw_fast_factor;
    return 0;
}
int gaz_engine_get_stats(gaz_engine* h, uint64_t out[16]) { return h->get_stats(out); }
int gaz_engine_synchronize(gaz_engine* h) { return h->synchronize(); }
int gaz_engine_timing_reset(gaz_engine* h, int32_t enable) { return h->timing_reset(enable); }
int gaz_engine_set_position(gaz_engine* h, int32_t slot, const int32_t* actions, int32_t n) { return h->set_position(slot, actions, n); }
int gaz_engine_set_search_params(gaz_engine* h, int32_t run_iterations, int32_t tau_mode) { return h->set_search_params(run_iterations, tau_mode); }
int gaz_engine_stop_search(gaz_engine* h, int32_t stop) { return h->stop_search(stop); }
int gaz_engine_start_search(gaz_engine* h) { return h->start_search(); }
int gaz_engine_set_hyperparams(gaz_engine* h, const gaz_search_hyperparams* hp) { return h->set_hyperparams(hp); }
// resignation: threshold = 0 is off (and then nothing else is looked at); else threshold in (0, 1), consecutive in [1, 8], min_ply >= 0, no_resign_prob in [0, 1]
int gaz_engine_set_resignation(gaz_engine* h, const gaz_resign_params* p) {
    if (!p) return h->fail("set_resignation: null argument");
    if (p->struct_size != sizeof(gaz_resign_params))
        return h->fail("set_resignation: struct_size is " + std::to_string(p->struct_size) + ", this library's gaz_resign_params has " + std::to_string(sizeof(gaz_resign_params)) + " bytes");
    if (p->threshold != p->threshold) return h->fail("set_resignation: threshold must be a number (0 = no resignation), not NaN");
    if (p->threshold > 1.7976931348623157e308 || p->threshold < -1.7976931348623157e308) return h->fail("set_resignation: threshold must be finite, not infinity");
    if (p->threshold < 0.0) return h->fail("set_resignation: threshold must be >= 0 (0 = no resignation), not " + std::to_string(p->threshold));
    if (p->threshold >= 1.0) return h->fail("set_resignation: threshold must be below 1 (q lies in [-1, 1], so no ply could trigger), not " + std::to_string(p->threshold));
    if (p->threshold == 0.0) return h->set_resignation(p);
    if (p->consecutive < 1 || p->consecutive > RESIGN_MAX_CONSECUTIVE)
        return h->fail("set_resignation: consecutive must be in [1, " + std::to_string(RESIGN_MAX_CONSECUTIVE) + "], not " + std::to_string(p->consecutive));
    if (p->min_ply < 0) return h->fail("set_resignation: min_ply must be >= 0, not " + std::to_string(p->min_ply));
    if (!(p->no_resign_prob >= 0.0 && p->no_resign_prob <= 1.0)) return h->fail("set_resignation: no_resign_prob must be in [0, 1], not " + std::to_string(p->no_resign_prob));
    return h->set_resignation(p);
}
// opening book: every refusal that needs no device state, then the engine validates the entries on the device (book_start.hpp)
int gaz_engine_set_opening_book(gaz_engine* h, const gaz_book_params* p, const uint8_t* actions, const int32_t* lengths) {
    if (!p) return h->fail("set_opening_book: null argument");
    if (p->struct_size != sizeof(gaz_book_params))
        return h->fail("set_opening_book: struct_size is " + std::to_string(p->struct_size) + ", this library's gaz_book_params has " + std::to_string(sizeof(gaz_book_params)) + " bytes");
    if (p->mode < 0 || p->mode > 2) return h->fail("set_opening_book: mode must be 0 (no book), 1 (an entry per game) or 2 (an entry per pair of games), not " + std::to_string(p->mode));
    if (p->n_entries < 0 || p->n_entries > BOOK_MAX_ENTRIES)
        return h->fail("set_opening_book: n_entries must be in [0, " + std::to_string(BOOK_MAX_ENTRIES) + "], not " + std::to_string(p->n_entries));
    if (p->mode == 0 || p->n_entries == 0) return h->set_opening_book(0, 0, 0, nullptr, nullptr);
    const int max_t = h->cfg.game == GAZ_GAME_TICTACTOE ? Game<GAME_TTT>::MAXT : (h->cfg.game == GAZ_GAME_CONNECT4 ? Game<GAME_C4>::MAXT : Game<GAME_GMK>::MAXT);
    if (p->stride < 1 || p->stride > max_t) return h->fail("set_opening_book: stride must be in [1, " + std::to_string(max_t) + "] (the longest game), not " + std::to_string(p->stride));
    if (!actions || !lengths) return h->fail("set_opening_book: actions and lengths must not be null with n_entries > 0");
    for (int32_t i = 0; i < p->n_entries; ++i)
        if (lengths[i] < 0 || lengths[i] > p->stride)
            return h->fail("set_opening_book: entry " + std::to_string(i) + ": a length of " + std::to_string(lengths[i]) + " is outside [0, stride = " + std::to_string(p->stride) + "]");
    return h->set_opening_book(p->n_entries, p->stride, p->mode, actions, lengths);
}
int gaz_engine_get_opening_book(gaz_engine* h, int32_t* n_entries, int32_t* mode) {
    if (!n_entries || !mode) return h->fail("get_opening_book: null argument");
    *n_entries = h->book_entries; *mode = h->book_mode;
    return 0;
}
int gaz_engine_read_book_counts(gaz_engine* h, uint64_t* counts, uint64_t out[8]) {
    if (!out || (h->book_entries > 0 && !counts)) return h->fail("read_book_counts: null argument");
    return h->read_book_counts(counts, out);
}
int gaz_engine_get_resign_stats(gaz_engine* h, uint64_t out[8]) { return out ? h->get_resign_stats(out) : h->fail("get_resign_stats: null argument"); }
// random board symmetry per evaluator request: 0 = off (a new engine), 1 = on
int gaz_engine_set_eval_symmetry(gaz_engine* h, int32_t mode) {
    if (mode != 0 && mode != 1) return h->fail("set_eval_symmetry: mode must be 0 (off) or 1 (a random board symmetry per evaluator request), not " + std::to_string(mode));
    return h->set_eval_symmetry(mode);
}
int gaz_engine_set_solver(gaz_engine* h, int32_t mode) {
    if (mode != 0 && mode != 1) return h->fail("set_solver: mode must be 0 (off) or 1 (prove wins, draws and losses in the PUCT tree), not " + std::to_string(mode));
    return h->set_solver(mode);
}
int gaz_engine_get_solver(gaz_engine* h, int32_t* mode) { return mode ? h->get_solver(mode) : h->fail("get_solver: null argument"); }
int gaz_engine_get_solver_stats(gaz_engine* h, uint64_t out[8]) { return out ? h->get_solver_stats(out) : h->fail("get_solver_stats: null argument"); }
int gaz_engine_get_eval_symmetry(gaz_engine* h, int32_t* mode) { return mode ? h->get_eval_symmetry(mode) : h->fail("get_eval_symmetry: null argument"); }
int gaz_engine_read_batch_symmetry(gaz_engine* h, uint8_t* sym) { return sym ? h->read_batch_symmetry(sym) : h->fail("read_batch_symmetry: null argument"); }
// match play: two networks in one engine
int gaz_engine_set_match(gaz_engine* h, const gaz_match_params* p) {
    if (!p) return h->fail("set_match: null argument");
    if (p->struct_size != sizeof(gaz_match_params))
        return h->fail("set_match: struct_size is " + std::to_string(p->struct_size) + ", this library's gaz_match_params has " + std::to_string(sizeof(gaz_match_params)) + " bytes");
    if (p->mode != 0 && p->mode != 1) return h->fail("set_match: mode must be 0 (off) or 1 (network A against network B), not " + std::to_string(p->mode));
    return h->set_match(p->mode, p->hash_salt_b);
}
int gaz_engine_get_match(gaz_engine* h, int32_t* mode) { return mode ? h->get_match(mode) : h->fail("get_match: null argument"); }
int gaz_engine_load_weights_b(gaz_engine* h, const gaz_tensor* t, int32_t n) { return h->load_weights_b(t, n); }
int gaz_engine_read_batch_network(gaz_engine* h, uint8_t* net) { return net ? h->read_batch_network(net) : h->fail("read_batch_network: null argument"); }
int gaz_engine_get_match_stats(gaz_engine* h, uint64_t out[8]) { return out ? h->get_match_stats(out) : h->fail("get_match_stats: null argument"); }
int gaz_engine_get_match_timing(gaz_engine* h, double out[8]) { return out ? h->get_match_timing(out) : h->fail("get_match_timing: null argument"); }
int gaz_engine_set_fused_wave(gaz_engine* h, int32_t on) { return h->set_fused_wave(on); }
int gaz_engine_debug_fused_fault(gaz_engine* h, int32_t mod) { return h->debug_fused_fault(mod); }
int gaz_engine_read_positions(gaz_engine* h, int32_t* n_hist, uint8_t* hist, int32_t stride) { return h->read_positions(n_hist, hist, stride); }
// a tree id this engine has: 0 / 1, or -1 = the tree running the move; single_tree and Gumbel engines keep one tree per game
static int check_tree_arg(gaz_engine* h, const char* fn, int32_t tree) {
    if (tree < -1 || tree > 1) return h->fail(std::string(fn) + ": tree must be 0, 1 or -1 (the tree running the game's move), not " + std::to_string(tree));
    if (tree == 1 && (h->cfg.single_tree || h->cfg.search == GAZ_SEARCH_GUMBEL))
        return h->fail(std::string(fn) + ": tree = 1 on an engine with one tree per game (single_tree or the Gumbel search); use tree = 0 or -1");
    return 0;
}
int gaz_engine_read_trees(gaz_engine* h, const int32_t* slots, int32_t n_slots, int32_t tree, int32_t max_depth, uint32_t min_visits, int64_t max_nodes,
                          int64_t max_edges, gaz_tree_node* nodes, gaz_tree_edge* edges, int64_t* node_first, int64_t* edge_first) {
    if (n_slots < 0) return h->fail("read_trees: n_slots must be >= 0, not " + std::to_string(n_slots));
    if (!node_first || !edge_first || (n_slots > 0 && !slots)) return h->fail("read_trees: slots, node_first and edge_first must not be null");
    if (check_tree_arg(h, "read_trees", tree)) return 1;
    if ((nodes == nullptr) != (edges == nullptr)) return h->fail("read_trees: nodes and edges must both be given, or both be null (counting call)");
    if (nodes && (max_nodes < 0 || max_edges < 0)) return h->fail("read_trees: max_nodes and max_edges must be >= 0");
    for (int32_t i = 0; i < n_slots; ++i)
        if (slots[i] < 0 || slots[i] >= h->cfg.n_games)
            return h->fail("read_trees: slots[" + std::to_string(i) + "] = " + std::to_string(slots[i]) + " is out of range [0, " + std::to_string(h->cfg.n_games) + ")");
    // too little capacity: refused before anything is written to the caller's arrays
    const gaz_engine::TreePlace place = [&](int64_t nn, int64_t ne, gaz_tree_node** pn, gaz_tree_edge** pe) {
        if (nn > max_nodes || ne > max_edges) return h->short_capacity(nn, ne, max_nodes, max_edges);
        *pn = nodes; *pe = edges; return 0;
    };
    return h->read_trees(slots, n_slots, tree, max_depth, min_visits, node_first, edge_first, nodes != nullptr, place);
}
int gaz_engine_read_pv(gaz_engine* h, int32_t tree, const int32_t* first_action, int32_t max_len, uint8_t* actions, uint32_t* N, float* W, int32_t* len) {
    if (max_len <= 0) return h->fail("read_pv: max_len must be positive, not " + std::to_string(max_len));
    if (!actions || !N || !W || !len) return h->fail("read_pv: actions, N, W and len must not be null");
    if (check_tree_arg(h, "read_pv", tree)) return 1;
    return h->read_pv(tree, first_action, max_len, actions, N, W, len);
}
int gaz_engine_repack(gaz_engine* h, int32_t* n_active, int32_t* n_launch) { return h->repack(n_active, n_launch); }
int gaz_engine_read_head_features(gaz_engine* h, int32_t n, float* p, float* v, int32_t* p_row, int32_t* v_row) { return h->read_head_features(n, p, v, p_row, v_row); }
int gaz_engine_probe_rules(gaz_engine* h, const int32_t* actions, const int32_t* n_actions, int32_t n_positions, int32_t stride, int8_t* board,
                           uint8_t* legal, int32_t* winner, int8_t* input, int32_t* terminal, const float* policy_in, float* policy_out) {
    return h->probe_rules(actions, n_actions, n_positions, stride, board, legal, winner, input, terminal, policy_in, policy_out);
}
int gaz_engine_probe_det(gaz_engine* h, int32_t op, int32_t n_items, const uint64_t* in, int32_t in_words, uint64_t* out, int32_t out_words) {
    return h->probe_det(op, n_items, in, in_words, out, out_words);
}
int gaz_engine_dominant_kernel(gaz_engine* h, char* name, int32_t cap, double* flops) { return h->dominant(name, cap, flops); }
int gaz_engine_timing_get(gaz_engine* h, double* a, double* b, double* c, int64_t* d, int64_t* e) { return h->timing_get(a, b, c, d, e); }

// ---- held-out loss (score.hpp)
int gaz_score_totals_size(void) { return (int)sizeof(gaz_score_totals); }
static int score_totals_fault(gaz_engine* h, const char* fn, const gaz_score_totals* t) {
    if (!t) return h->fail(std::string(fn) + ": null totals");
    if (t->struct_size != sizeof(gaz_score_totals))
        return h->fail("gaz_score_totals.struct_size is " + std::to_string(t->struct_size) + ", this library's gaz_score_totals has " + std::to_string(sizeof(gaz_score_totals)) +
                       " bytes: rebuild the binding from include/gaz_engine.h");
    return 0;
}
int gaz_engine_score_outputs(gaz_engine* h, const float* pp, const float* pv, const float* tp, const float* tv, int64_t n, int32_t mode, gaz_score_totals* t, double* row_ce,
                             double* row_ent, double* row_se, uint8_t* row_flags) {
    if (score_totals_fault(h, "score_outputs", t)) return 1;
    if (n < 0 || n > 0x7fffffffll) return h->fail("score_outputs: n must be in [0, 2^31 - 1], not " + std::to_string(n));
    if (n > 0 && (!pp || !pv || !tp || !tv)) return h->fail("score_outputs: null arrays");
    if (mode < -1 || mode > 3) return h->fail("score_outputs: policy_mode must be -1 (the engine's own) or 0 .. 3, not " + std::to_string(mode));
    ScoreState* S = h->score_state();
    if (S->outputs(pp, pv, tp, tv, n, mode < 0 ? h->score_mode() : mode, t, row_ce, row_ent, row_se, row_flags)) return h->fail(S->err);
    return 0;
}
int gaz_engine_score_replay(gaz_engine* h, gaz_replay* w, int32_t batch_rows, int32_t augment, gaz_score_totals* t, double* row_ce, double* row_ent, double* row_se,
                            uint8_t* row_flags, double* ms_total) {
    if (score_totals_fault(h, "score_replay", t)) return 1;
    return h->score_replay(w, batch_rows, augment != 0, t, row_ce, row_ent, row_se, row_flags, ms_total);
}
int gaz_engine_score_rows_timed(gaz_engine* h, int32_t repeats, double* ms_per_launch) {
    ScoreState* S = h->score_state();
    return S->rows_timed(repeats, ms_per_launch) ? h->fail(S->err) : 0;
}

}  // extern "C"
