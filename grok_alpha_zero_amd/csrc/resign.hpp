// resign.hpp — resignation in self-play, and the games played out to calibrate it (gaz_engine_set_resignation; no
// reference counterpart: Self_Play.play() plays every game to its end).
//
// The rule is STATELESS: after ply p (0-based, the game going on: no win, no draw, not the max_actions cap) it reads the game's own record —
// q of the played move from the mover's view and move_kind, written per ply by move_end / g_move_end — and triggers iff
//     p >= min_ply  and  p >= 2 (consecutive - 1)  and  for i in 0 .. consecutive-1: kind(p - 2i) != 0  and  q[p - 2i] < -threshold
// i.e. the mover's last `consecutive` searched plies all saw the game as lost (the float32 q widened to double, strict <).  A ply no search
// ran at (a set_position prefix, a move the host played: kind 0) breaks the run; fast plies of the playout cap count like full ones.
// A ply of an opening-book prefix (kind 3, book.hpp MK_BOOK) breaks the run exactly as kind 0 does: its recorded q is the 0 the start wrote
// there, and 0 < -threshold never holds, so the test below needs no case of its own.
// Whether a game is a PLAY-OUT game (resignation disabled, to measure false positives, as AlphaGo Zero does for a tenth of its games) is
// one uniform variate of the game-level stream, keyed by (seed, slot, game_seq) like the opening draw: tree 2, event 0, purpose P_RESIGN,
// u < no_resign_prob.  Nothing is kept in GameState or TreeState, no tree's event counter moves and no search changes, so the record of a
// game with resignation on is a prefix of its record with resignation off.
//   trigger, not a play-out game: the game ends after p with winner = -mover; move_kind[p] |= MK_RESIGNED
//   trigger, play-out game:       move_kind[p] |= MK_WOULD_RESIGN (every such ply) and the game goes on
//   natural end of a play-out game: the first MK_WOULD_RESIGN ply f, if any, is the ply the game would have been resigned at — a false
//                                   positive when the would-be resigner drew or won (winner != -mover(f))
// The parameters and counters live in one small block in HBM behind the game_stats counters (DevParams::stats + RESIGN_STATS_OFFSET), which
// only resign_after_ply touches: once per move, on the team's lane 0.  Nothing is added to the kernel arguments — the fused launches hold
// DevParams in scalar registers across their trunk role — and a block whose threshold is 0 (a new engine) means off.
#pragma once
#include <stddef.h>
#include "det.hpp"
#include "tree.hpp"

namespace gaz {

constexpr int RESIGN_MAX_CONSECUTIVE = 8;
struct ResignBlock {
    double threshold;          // in (0, 1); 0 = off
    double no_resign_prob;     // in [0, 1]
    int32_t consecutive;       // 1 .. RESIGN_MAX_CONSECUTIVE
    int32_t min_ply;           // >= 0
    // gaz_engine_get_resign_stats: [0] games resigned, [1] / [2] of them by player -1 / 1, [3] play-out games finished, [4] of them with a
    // would-have-resigned ply, [5] of those false positives, [6] plies of the resigned games, [7] 0
    unsigned long long stats[8];
};
constexpr int RESIGN_STATS_OFFSET = 8;       // DevParams::stats: [8] counters of the engine, then the ResignBlock
enum : int32_t { RESIGN_NONE = 0, RESIGN_NOW = 1, RESIGN_WOULD = 2 };

GAZ_DEV bool resign_trigger(const ResignBlock* rb, const float* q, const uint8_t* mk, int p) {
    const int c = rb->consecutive;
    if (p < rb->min_ply || p < 2 * (c - 1)) return false;
    const double lim = -rb->threshold;
    // a fixed trip count and no exits: plies beyond the run read ply p again.  With the early-exit loop over `c` the fused Connect4 launches
    // spilled 22 to 29 VGPRs instead of 19 to 25 (profiles/resign_kernel_resources.json)
    bool all = true;
#pragma unroll
    for (int i = 0; i < RESIGN_MAX_CONSECUTIVE; ++i) {
        const int j = i < c ? p - 2 * i : p;
        all = all && (mk[j] & MK_KIND_MASK) != MK_NONE && (double)q[j] < lim;
    }
    return all;
}

GAZ_DEV bool resign_is_playout_game(const ResignBlock* rb, uint32_t key0, uint32_t key1, uint32_t slot, uint32_t game_seq) {
    const double p = rb->no_resign_prob;
    if (!(p > 0.0)) return false;                    // (u >= 0: the draw could not say otherwise)
    det::Event e; e.key0 = key0; e.key1 = key1; e.slot = slot; e.game_seq = game_seq;
    e.event = 0; e.tree = 2; e.purpose = det::P_RESIGN;
    return det::uniform(e) < p;
}

// After ply p of game (slot, game_seq) has been played and recorded, on one lane; q and mk are the record's OFF_Q and OFF_MK arrays.  `over`: the
// game has ended by itself (a win, a draw or the max_actions cap; `winner` is then its result) — natural ends and the cap take precedence over
// the rule.  Returns RESIGN_NOW when the game ends here by resignation (the caller makes -mover the winner), having marked the ply in the
// record and counted what there is to count.
GAZ_DEV int resign_after_ply(unsigned long long* game_stats, uint32_t key0, uint32_t key1, uint32_t slot, uint32_t game_seq, const float* q, uint8_t* mk,
                                 int p, bool over, int winner) {
    ResignBlock* rb = reinterpret_cast<ResignBlock*>(game_stats + RESIGN_STATS_OFFSET);
    if (!(rb->threshold > 0.0)) return RESIGN_NONE;
    if (!over && !resign_trigger(rb, q, mk, p)) return RESIGN_NONE;
    const bool playout = resign_is_playout_game(rb, key0, key1, slot, game_seq);
    if (!over) {
        mk[p] |= playout ? MK_WOULD_RESIGN : MK_RESIGNED;
        if (playout) return RESIGN_WOULD;
        atomic_add(&rb->stats[0], 1ull);
        atomic_add(&rb->stats[(p & 1) ? 2 : 1], 1ull);   // the mover of ply p resigns: -1 moves first (GameState::next_player)
        atomic_add(&rb->stats[6], (unsigned long long)(p + 1));
        return RESIGN_NOW;
    }
    if (!playout) return RESIGN_NONE;
    atomic_add(&rb->stats[3], 1ull);
    for (int f = 0; f <= p; ++f) {
        if (!(mk[f] & MK_WOULD_RESIGN)) continue;
        atomic_add(&rb->stats[4], 1ull);
        const int resigner = (f & 1) ? 1 : -1;
        if (winner != -resigner) atomic_add(&rb->stats[5], 1ull);
        break;
    }
    return RESIGN_NONE;
}

}  // namespace gaz
