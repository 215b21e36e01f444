// match.hpp — match play (gaz_engine_set_match): the routing stage between the tree step and the evaluator pass of a wave
// whose games are played by TWO networks.  The tree kernels and the evaluators are untouched: after a tree step the owner of every pending row is
// in GameState, so the network of a row is a function of the game state alone,
//   owner = PUCT with two trees: pend_tree (tree 0 searches for player -1)      Gumbel: next_player == -1 ? 0 : 1
//   net   = owner ^ ((slot_id + game_seq) & 1)                                  0 = network A, 1 = network B, 255 = the row carries no request
// and the stage is  route -> stable partition -> copy into two dense batches -> [both evaluators] -> scatter.
//   k_match_route    one lane per row: net[row], and per block of 64 rows the number of A and B rows (two ballots, one 64-bit word per block)
//   k_match_pack     the stable partition: a row's place is (rows of its network in the blocks before) + (those in lower lanes of its block);
//                    rows of A in ascending row order into idx_a, rows of B likewise into idx_b.  No atomics: the order is the row order
//   k_match_copy     input rows idx_a[r] / idx_b[r] -> dense staging row r, in the widest unit the row size divides into
//   k_match_scatter  policy / value row r of each dense batch -> rows idx_a[r] / idx_b[r] of the engine's batch; rows without a request are
//                    not written (no tree kernel reads the outputs of a row whose pend_kind is PEND_NONE)
// Under GAZ_HOST_EMU a wave is one lane and the blocks run in order, as for every kernel of engine.hip.
#pragma once
#include "tree.hpp"
#include "wave.hpp"

namespace gaz {

enum : uint8_t { NET_A = 0, NET_B = 1, NET_NONE = 255 };

template <class G> GAZ_DEV uint8_t match_network(const GameState<G>& gs, int gumbel) {
    if (gs.pend_kind == PEND_NONE) return NET_NONE;
    const uint32_t owner = gumbel ? (gs.next_player == -1 ? 0u : 1u) : (uint32_t)(gs.pend_tree & 1);
    return (uint8_t)(owner ^ ((gs.slot_id + gs.game_seq) & 1u));
}

// blk[b] = (B rows of block b) << 32 | (A rows of block b); grid = ceil(n / WAVE) blocks of one wave
template <class G> GAZ_KERNEL k_match_route(const GameState<G>* games, int n, int gumbel, uint8_t* net, unsigned long long* blk) {
    const int g = block_id() * WAVE + lane_id();
    const uint8_t v = g < n ? match_network<G>(games[g], gumbel) : (uint8_t)NET_NONE;
    if (g < n) net[g] = v;
    const uint64_t a = ballot(v == NET_A), b = ballot(v == NET_B);
    if (lane_id() == 0) blk[block_id()] = ((unsigned long long)popcll(b) << 32) | (unsigned long long)popcll(a);
}

// same grid.  cnt[0] = rows of A, cnt[1] = rows of B (written by the last block)
template <class G> GAZ_KERNEL k_match_pack(const uint8_t* net, const unsigned long long* blk, int n, int32_t* idx_a, int32_t* idx_b, uint32_t* cnt) {
    const int b = block_id(), g = b * WAVE + lane_id();
    uint64_t before = 0;                             // (both halves at once: a batch has far fewer than 2^32 rows, no carry between them)
    for (int i = lane_id(); i < b; i += WAVE) before += blk[i];
    before = wave_sum_u64(before);
    const uint32_t off_a = (uint32_t)before, off_b = (uint32_t)(before >> 32);
    const uint8_t v = g < n ? net[g] : (uint8_t)NET_NONE;
    const uint64_t a = ballot(v == NET_A), bb = ballot(v == NET_B);
    const uint64_t below = (1ull << lane_id()) - 1ull;
    if (v == NET_A) idx_a[off_a + (uint32_t)popcll(a & below)] = g;
    if (v == NET_B) idx_b[off_b + (uint32_t)popcll(bb & below)] = g;
    if (b == (n + WAVE - 1) / WAVE - 1 && lane_id() == 0) { cnt[0] = off_a + (uint32_t)popcll(a); cnt[1] = off_b + (uint32_t)popcll(bb); }
}

// the widest power-of-two unit (<= 16 bytes) that divides a row: rows start at multiples of it in buffers that start at multiples of 256
template <int BYTES> struct CopyUnit { typedef uint8_t type; };
template <> struct CopyUnit<2> { typedef uint16_t type; };
template <> struct CopyUnit<4> { typedef uint32_t type; };
template <> struct CopyUnit<8> { typedef unsigned long long type; };
template <> struct CopyUnit<16> { typedef uint4 type; };
template <class G> struct MatchRow {
    static constexpr int ROWB = G::HW * G::C;        // 168 (Connect4: 8-byte units), 450 (Gomoku: 2), 18 (TicTacToe: 2)
    static constexpr int UNITB = ROWB % 16 == 0 ? 16 : ROWB % 8 == 0 ? 8 : ROWB % 4 == 0 ? 4 : ROWB % 2 == 0 ? 2 : 1;
    static constexpr int UNITS = ROWB / UNITB;
    typedef typename CopyUnit<UNITB>::type unit;
};

// one thread per unit of a dense row, n_max rows launched (the host does not know cnt yet): dense row r < cnt[0] is A's, the next cnt[1] are B's
template <class G> GAZ_KERNEL_WIDE k_match_copy(const int8_t* in, const int32_t* idx_a, const int32_t* idx_b, const uint32_t* cnt, int n_max, int8_t* in_a, int8_t* in_b) {
    typedef typename MatchRow<G>::unit U;
    constexpr int UNITS = MatchRow<G>::UNITS;
#ifdef GAZ_HOST_EMU
    const long long i = block_id();
#else
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
#endif
    const long long r = i / UNITS; const int u = (int)(i % UNITS);
    const long long na = cnt[0], nb = cnt[1];
    if (r >= n_max || r >= na + nb) return;
    const bool is_a = r < na;
    const long long d = is_a ? r : r - na;
    const int src = is_a ? idx_a[d] : idx_b[d];
    const U* s = reinterpret_cast<const U*>(in) + (size_t)src * UNITS;
    U* t = reinterpret_cast<U*>(is_a ? in_a : in_b) + (size_t)d * UNITS;
    t[u] = s[u];
}

// one thread per output float of the na + nb dense rows (A policy floats and the value)
template <class G> GAZ_KERNEL_WIDE k_match_scatter(const int32_t* idx_a, const int32_t* idx_b, int na, int nb, const float* pol_a, const float* val_a,
                                                   const float* pol_b, const float* val_b, float* policy, float* value) {
    constexpr int A = G::A;
#ifdef GAZ_HOST_EMU
    const long long i = block_id();
#else
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
#endif
    const long long r = i / (A + 1); const int a = (int)(i % (A + 1));
    if (r >= (long long)na + nb) return;
    const bool is_a = r < na;
    const long long d = is_a ? r : r - na;
    const int dst = is_a ? idx_a[d] : idx_b[d];
    if (a < A) policy[(size_t)dst * A + a] = (is_a ? pol_a : pol_b)[(size_t)d * A + a];
    else value[dst] = (is_a ? val_a : val_b)[d];
}

}  // namespace gaz
