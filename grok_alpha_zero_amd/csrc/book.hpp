// book.hpp — opening book: games that start from book positions, paired for matches (gaz_engine_set_opening_book; no
// reference counterpart: Self_Play.play() starts every game on the empty board, and its opening_actions override move 0 only).
//
// The rule is STATELESS, a function of the game's identity: game (slot, game_seq) — slot = GameState::slot_id, the global slot of the record
// header — draws
//     u   = uniform(seed, slot, key_seq, tree 3, event 0, purpose P_OPENING)      key_seq = game_seq (mode 1), game_seq & ~1 (mode 2)
//     idx = min((int)(u * n_entries), n_entries - 1)                               (float64)
// and starts from entry idx: what k_set_position makes of a slot, with move_kind MK_BOOK on the prefix plies.  Tree 3 is the stream of the book
// alone (det.hpp).  In mode 2 the two games (slot, 2k) and (slot, 2k + 1) of a colour-swapped match pair share their entry; their searches stay
// keyed by game_seq.  The rule survives gaz_engine_repack, game groups, slot_offset and first_game_seq because nothing else enters it.
//
// Where it runs.  The tree kernels (puct_core.hpp / gumbel_core.hpp) carry NOTHING of the feature — the fused launches sit at their register
// cap, and even one load and a branch in PH_NEW_GAME moved their spills — and an engine with or without a book launches the very kernels it
// launched before.  Two things make that possible:
//   * k_book_start (book_start.hpp), launched in front of every tree step while a book is set, starts the games that wait: one team per game,
//     the lanes zero the record prefix and place the stones, and the game goes on from PH_ROOT in the tree step that follows;
//   * a game that ends inside a tree step must wait for it instead of starting on the empty board in the same launch.  ring_push already has
//     the state for that: a slot whose next game is beyond DevParams::games_budget goes to PH_HALT.  While a book is set the host hands the
//     tree steps a budget of 1 (EngineT::wave_params) — every finished game then parks in PH_HALT — and k_book_start, which gets the true
//     budget, applies the true rule: a parked slot whose next game is within the budget starts, the others stay halted for good.
// A started game costs one wave of latency, nothing else; results do not depend on the wave a game starts in.  When the book is removed the
// same kernel sends the parked slots on to PH_NEW_GAME.
// The parameters and counters live in one block in HBM behind the ResignBlock (DevParams::stats + BOOK_STATS_OFFSET): nothing is added to the
// kernel arguments.  n_entries = 0 (a new engine) means no book.
#pragma once
#include "det.hpp"
#include "tree.hpp"
#include "resign.hpp"

namespace gaz {

enum : uint8_t { MK_BOOK = 3 };                      // move_kind of a book ply: the free value of the kind's two low bits (tree.hpp MK_*)
constexpr int BOOK_MAX_ENTRIES = 1 << 20;
struct BookBlock {
    int32_t n_entries, stride, mode, pad_;           // mode 1 = per game, 2 = per pair; n_entries = 0 = off
    const uint8_t* actions;                          // [n_entries][stride]
    const int32_t* lengths;                          // [n_entries]
    unsigned long long* counts;                      // [n_entries] games started from every entry
    unsigned long long started, plies;               // games started with a book set, prefix plies placed — over the engine's life
};
constexpr int BOOK_STATS_OFFSET = RESIGN_STATS_OFFSET + (int)((sizeof(ResignBlock) + 7) / 8);
constexpr int BOOK_STATS_WORDS = (int)((sizeof(BookBlock) + 7) / 8);
GAZ_HD BookBlock* book_block(unsigned long long* game_stats) { return reinterpret_cast<BookBlock*>(game_stats + BOOK_STATS_OFFSET); }

GAZ_DEV int book_draw(uint32_t key0, uint32_t key1, uint32_t slot, uint32_t game_seq, int mode, int n_entries) {
    det::Event e; e.key0 = key0; e.key1 = key1; e.slot = slot; e.game_seq = mode == 2 ? (game_seq & ~1u) : game_seq;
    e.event = 0; e.tree = 3; e.purpose = det::P_OPENING;
    const int idx = (int)(det::uniform(e) * (double)n_entries);
    return idx < n_entries - 1 ? idx : n_entries - 1;
}

}  // namespace gaz
