// samples.hpp — finished games leave the device as TRAINING SAMPLES (gaz_engine_drain_samples): what Self_Play.play() collects per
// game (Self_Play.py:159-175: input states before every move, improved policies, values = 0.5 (z + q)) and what augment_sample makes of
// it (Guide.py:255-283; Connect4.py:442-443, Gomoku.py:265-303, Tictactoe.py:321-358), built from the records in the ring.
//
// The host definition of every byte is self_play._fast_states + games.augment_sample + engine.decode_record; this is a gather of it:
//   * no board is replayed.  fill[cell] = the ply at which the cell was filled (from the action list; Connect4: the row is the number
//     of earlier moves in the column), the stone there is the mover of that ply (even plies: -1), and the board "k moves back" at
//     ply t is  fill[cell] < t - k ? stone : 0.
//   * every output element is then an independent function of (ply, augmentation, cell / action); the symmetry is applied on the
//     READ side (output cell -> source cell), so a game's rows of one augmentation are one contiguous range that is written as
//     whole 16-byte vectors (single elements only at the ragged ends: a row is 18 / 168 / 450 bytes, a range starts anywhere).
// One workgroup per game; fill table and action list in LDS.
//
// Playout cap randomisation (gaz_engine_config::fast_iterations): a ply whose search was a fast one (RecLayout::OFF_MK, MK_FAST) gives no row.
// The workgroup compacts the plies it keeps into a table in LDS (kept row -> ply, a ballot / popcount scan) and every output element is
// indexed through it: the rows of a game stay one contiguous range, and a kept row is what it is without the cap — its state shows every
// move played before it, fast ones included.  With the cap off the table is the identity.
// A ply of an opening-book prefix (move_kind 3, book.hpp MK_BOOK) gives no row either, with or without the surprise weighting, and takes no
// part in the weighting's means and counts: kinds 2 and 3 are left out alike.  (A gaz_engine_set_position prefix, kind 0, keeps its rows.)
#pragma once
#include "tree.hpp"

namespace gaz {

#ifdef GAZ_HOST_EMU
#define GAZ_SAMPLES_BOUNDS
GAZ_DEV void group_sync() {}
#else
#define GAZ_SAMPLES_BOUNDS __launch_bounds__(256)
GAZ_DEV void group_sync() { __syncthreads(); }
#endif
constexpr int SAMPLES_THREADS = 256;

template <class G> struct SampleAug { static constexpr int N = 8; };          // the 8 symmetries of a square board
template <> struct SampleAug<Game<GAME_C4>> { static constexpr int N = 2; };  // [identity, np.fliplr]

// plies of a record as the sample builder counts them (a header is data: never trust it with an index)
template <class G> GAZ_HD int sample_plies(int T) { return T < 0 ? 0 : (T > G::MAXT ? G::MAXT : T); }

// output cell (y, x) of augmentation k -> the cell of the un-augmented board it shows.
// Square boards: games.hpp square_src_cell (the order of games._GridGame.augment_sample).  games.Connect4.augment_sample: np.fliplr of the
// [T,6,7,4] states reverses axis 1 = the board ROWS.
template <class G> GAZ_DEV int board_src_cell(int k, int y, int x) {
    if (G::ID == GAME_C4) return (k ? G::H - 1 - y : y) * G::W + x;
    return square_src_cell(k, y, x, G::W);
}
// the same for a policy index; Connect4's [T,7] policy is mirrored along the COLUMNS (Connect4.py:442-443: kept as the reference has it)
template <class G> GAZ_DEV int policy_src_index(int k, int a) {
    if (G::ID == GAME_C4) return k ? G::A - 1 - a : a;
    return board_src_cell<G>(k, a / G::W, a % G::W);
}

// element r of the input state before ply t, augmentation k (get_input_state_MCTS, [H][W][C] int8)
template <class G> GAZ_DEV int8_t state_element(const int* fill, int t, int k, int r) {
    const int c = r % G::C, cell = r / G::C;
    const int f = fill[board_src_cell<G>(k, cell / G::W, cell % G::W)];
    const int stone = (f & 1) ? 1 : -1;                                   // the first mover is -1
    if (G::ID == GAME_C4) {
        // plane 3 = board, planes 2 / 1 = one / two moves back once 2 / 3 moves were played, plane 0 = minus the next player until four
        // moves were played and the board three moves back after that (Connect4.py:340-345)
        const int back = 3 - c;
        if (back == 0 || t > back) return (int8_t)(f < t - back ? stone : 0);
        return (int8_t)(c == 0 ? ((t & 1) ? -1 : 1) : 0);
    }
    if (c == 0) return (int8_t)((t & 1) ? 1 : -1);                        // the mover, on every cell
    return (int8_t)(f < t ? stone : 0);
}

// dst[start + i] = f(i) for i in [0, count): 16-byte vector stores wherever start + i is a multiple of VEC = 16 / sizeof(T), single
// elements before the first and after the last whole vector.  dst itself is 16-byte aligned (an allocation's base).
template <class T, class F> GAZ_DEV void emit_range(T* dst, size_t start, int count, int t, int nT, F f) {
    constexpr int VEC = 16 / (int)sizeof(T);
    const int head0 = (int)((VEC - start % VEC) % VEC);
    const int head = head0 < count ? head0 : count;
    const int n_vec = (count - head) / VEC;
    for (int i = t; i < head; i += nT) dst[start + i] = f(i);
    for (int v = t; v < n_vec; v += nT) {
        T tmp[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) tmp[j] = f(head + v * VEC + j);
        uint4 u;
        memcpy(&u, tmp, 16);
        *reinterpret_cast<uint4*>(dst + start + head + (size_t)v * VEC) = u;
    }
    for (int i = head + n_vec * VEC + t; i < count; i += nT) dst[start + i] = f(i);
}

// the [T, winner, slot, game_seq] headers of `n` ring slots from `first` on and the rows each game gives (its plies that are neither MK_FAST nor MK_BOOK),
// dense, SAMPLE_HDR_INTS per game: what the host needs to choose the games of a drain
constexpr int SAMPLE_HDR_INTS = 5;
template <class G> GAZ_SAMPLES_BOUNDS GAZ_KERNEL_WIDE k_sample_headers(const uint8_t* ring, int ring_cap, uint32_t first, int n, int32_t* out) {
#ifdef GAZ_HOST_EMU
    const int i = block_id();
#else
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
#endif
    if (i >= n) return;
    const uint8_t* rec = ring + (size_t)((first + (uint32_t)i) % (uint32_t)ring_cap) * RecLayout<G>::SIZE;
    const int32_t* hdr = reinterpret_cast<const int32_t*>(rec + RecLayout<G>::OFF_HDR);
    for (int j = 0; j < 4; ++j) out[SAMPLE_HDR_INTS * i + j] = hdr[j];
    static_assert(RecLayout<G>::OFF_MK % 4 == 0 && G::TPAD % 4 == 0, "move_kind is read in 32-bit words");
    const uint32_t* mk = reinterpret_cast<const uint32_t*>(rec + RecLayout<G>::OFF_MK);
    const int T = sample_plies<G>(hdr[0]);
    int fast = 0;
    for (int w = 0; w * 4 < T; ++w) {
        const uint32_t v = mk[w];
        for (int j = 0; j < 4; ++j) fast += (w * 4 + j < T) && ((v >> (8 * j)) & MK_KIND_MASK) >= MK_FAST;   // fast and book plies (the kind: the bits above it mark resignation)
    }
    out[SAMPLE_HDR_INTS * i + 4] = T - fast;
}

// plan[i] = ring slot of the drain's i-th game, plan[n + i] = row0[i] = the exclusive prefix sum of the games' kept rows.  The drain has R rows;
// augmentation k of an output array starts k * R rows in.
template <class G> GAZ_SAMPLES_BOUNDS GAZ_KERNEL_WIDE k_build_samples(const uint8_t* ring, int ring_cap, const int32_t* plan, int n, long long R,
                                                                       int8_t* boards, float* policies, float* values) {
    using RL = RecLayout<G>;
    constexpr int SB = G::HW * G::C, NA = SampleAug<G>::N, NEVER = 0x7ffffffe;
#ifdef GAZ_HOST_EMU
    const int b = block_id(), nT = 1, t = 0;
#else
    const int b = blockIdx.x, nT = blockDim.x, t = threadIdx.x;
#endif
    GAZ_SHARED int fill[G::HW];
    GAZ_SHARED uint8_t act[G::TPAD];
    GAZ_SHARED uint8_t kept[G::TPAD];                                     // kept row -> ply (MAXT <= 255)
    GAZ_SHARED int wave_kept[SAMPLES_THREADS / 64 + 1];
    static_assert(G::MAXT <= 255, "plies are kept as bytes");
    if (b >= n) return;
    const int slot = plan[b];
    if (slot < 0 || slot >= ring_cap) return;
    const uint8_t* rec = ring + (size_t)slot * RL::SIZE;
    const int32_t* hdr = reinterpret_cast<const int32_t*>(rec + RL::OFF_HDR);
    const int T = sample_plies<G>(hdr[0]), winner = hdr[1];
    const long long row0 = plan[n + b];
    for (int i = t; i < G::HW; i += nT) fill[i] = NEVER;
    for (int i = t; i < T; i += nT) act[i] = rec[RL::OFF_ACT + i];
    // the plies that give a row, in order: per pass of nT plies every wavefront ballots its lanes, the wavefronts' counts meet in LDS, and a
    // kept ply lands at (rows of earlier passes) + (rows of lower wavefronts) + (kept lanes below its own).  (The one-lane emulation: WAVE = 1,
    // one "wavefront", one ply per pass.)
    const int lane = t % WAVE, wv = t / WAVE, n_wv = (nT + WAVE - 1) / WAVE;
    int K = 0;
    for (int base = 0; base < T; base += nT) {
        const int p = base + t;
        const bool keep = p < T && (rec[RL::OFF_MK + p] & MK_KIND_MASK) < MK_FAST;          // neither a fast ply nor a book ply (kind 3)
        const uint64_t m = ballot(keep);
        if (lane == 0) wave_kept[wv] = popcll(m);
        group_sync();
        int below = 0, all = 0;
        for (int w = 0; w < n_wv; ++w) { const int c = wave_kept[w]; below += w < wv ? c : 0; all += c; }
        if (keep) kept[K + below + popcll(m & ((1ull << lane) - 1ull))] = (uint8_t)p;
        K += all;
        group_sync();
    }
    group_sync();                                                         // (T = 0: no pass ran)
    if (row0 < 0 || row0 + K > R) return;                              // (the host built row0 from k_sample_headers' counts of these very records)
    if (G::ID == GAME_C4) {
        for (int p = t; p < T; p += nT) {                                 // row = 5 - the earlier moves in the same column
            const int a = act[p];
            int below = 0;
            for (int e = 0; e < p; ++e) below += act[e] == a;
            if (a < G::W && below < G::H) fill[(G::H - 1 - below) * G::W + a] = p;
        }
    } else {
        for (int p = t; p < T; p += nT) if (act[p] < G::HW) fill[act[p]] = p;
    }
    group_sync();
    const float* q = reinterpret_cast<const float*>(rec + RL::OFF_Q);
    const float* pol = reinterpret_cast<const float*>(rec + RL::OFF_POL);
    // z as engine.py decode_record derives it: z[p] = mover(p) * winner, the mover of ply p being -1 on even plies (Self_Play.py:127).  Without
    // resignation the winner is 0 or the LAST mover, and this is the reference's rule (mover signs, all turned when -1 won and moved last,
    // zeros for a draw: Self_Play.py:165-172) value for value; a resigned game is won by the player who did not move last
    for (int j = t; j < K; j += nT) {
        const int p = kept[j];
        const float z = (float)(((p & 1) ? 1 : -1) * winner);
        values[row0 + j] = 0.5f * (z + q[p]);
    }
    for (int k = 0; k < NA; ++k) {
        const size_t row = (size_t)k * (size_t)R + (size_t)row0;
        emit_range<int8_t>(boards, row * SB, K * SB, t, nT, [&](int i) { return state_element<G>(fill, kept[i / SB], k, i % SB); });
        emit_range<float>(policies, row * G::A, K * G::A, t, nT, [&](int i) { return pol[kept[i / G::A] * G::A + policy_src_index<G>(k, i % G::A)]; });
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// Policy surprise weighting (gaz_engine_set_sample_weighting; DESIGN.md "Policy surprise weighting"; KataGo, Wu 2019, section 3.3): the
// rows a ply gives become a COUNT c_p, a function of the finished record, (lambda, fast_factor) and the engine's seed alone.
//   s_p  = max(0, sum_a pi_p[a] (dlog pi_p[a] - dlog P_p[a])) over pi_p[a] > 0 and P_p[a] > 0, a ascending, sequential float64; NaN / inf = 0
//   w0_p = 1 for a full ply, 0 for a fast one; a ply without a search (set_position prefix) keeps its one row and takes no part; a book
//          ply (kind 3) gives no row and takes no part
//   mean = (sum of s_p over the full plies, in ply order) / n_full;  a fast ply is eligible iff s_p > fast_factor * mean
//   S    = sum of s_p over E = full + eligible fast plies, in ply order
//   w_p  = (1 - lambda) w0_p + lambda n_full s_p / S on E, 0 elsewhere; w0_p if n_full == 0 or S is 0 or not finite
//   c_p  = floor(w_p) + (u_p < w_p - floor(w_p)), u_p = uniform(seed, slot, game_seq, tree 2, event 0x40000000 + p, P_PLAYOUT_CAP)
// (det::draw puts all 32 bits of the event into Philox counter word 2, so the variate shares nothing with the cap's own draw, event p.)
// P_p is the record's P row: the priors the root searched with, Dirichlet noise included — the only prior a record keeps.
constexpr uint32_t SURPRISE_EVENT = 0x40000000u;
// The two clamps of k_sample_weights keep the tables of k_build_samples_w in bounds whatever a record holds; with a record the engine wrote
// they cannot act (the counts would then differ from self_play.sample_row_counts), and the emulation build, which the tests run, aborts if one does.
#ifdef GAZ_HOST_EMU
inline void emu_unreachable() { abort(); }
#else
GAZ_DEV void emu_unreachable() {}
#endif
template <class G> constexpr int sample_rows_cap() { return 2 * G::MAXT; }        // rows of one game: < n_full + |E| + 1 <= 2 T

template <class G> GAZ_DEV double ply_surprise(const float* pi, const float* P) {
    double s = 0.0;
    for (int a = 0; a < G::A; ++a) {
        const float x = pi[a], y = P[a];
        if (x > 0.0f && y > 0.0f) s = s + (double)x * (det::dlog((double)x) - det::dlog((double)y));
    }
    if (!(s == s) || s > 1.7976931348623157e308 || s < -1.7976931348623157e308) return 0.0;
    return s > 0.0 ? s : 0.0;
}

// one workgroup per ring record of the drain window [first, first + n): counts[b][p] = c_p (0 from the record's T on), rows[2 b] = the game's
// rows, rows[2 b + 1] = its plies that give no row.  One lane per ply walks its A actions; the sums over plies are one lane's, in ply order.
template <class G> GAZ_SAMPLES_BOUNDS GAZ_KERNEL_WIDE k_sample_weights(const uint8_t* ring, int ring_cap, uint32_t first, int n, uint32_t key0, uint32_t key1,
                                                                        double lambda, double fast_factor, uint8_t* counts, int32_t* rows) {
    using RL = RecLayout<G>;
#ifdef GAZ_HOST_EMU
    const int b = block_id(), nT = 1, t = 0;
#else
    const int b = blockIdx.x, nT = blockDim.x, t = threadIdx.x;
#endif
    GAZ_SHARED double s[G::TPAD];
    GAZ_SHARED double sums[2];                                            // n_full * lambda (0: w = w0), S
    GAZ_SHARED double mean_cut;                                           // fast_factor * mean
    GAZ_SHARED uint8_t cnt[G::TPAD];
    if (b >= n) return;
    const uint8_t* rec = ring + (size_t)((first + (uint32_t)b) % (uint32_t)ring_cap) * RL::SIZE;
    const int32_t* hdr = reinterpret_cast<const int32_t*>(rec + RL::OFF_HDR);
    const int T = sample_plies<G>(hdr[0]);
    const uint8_t* mk = rec + RL::OFF_MK;
    const float* pol = reinterpret_cast<const float*>(rec + RL::OFF_POL);
    const float* pri = reinterpret_cast<const float*>(rec + RL::OFF_P);
    for (int p = t; p < T; p += nT) s[p] = ((mk[p] & MK_KIND_MASK) == MK_NONE || (mk[p] & MK_KIND_MASK) == MK_KIND_MASK) ? 0.0 : ply_surprise<G>(pol + (size_t)p * G::A, pri + (size_t)p * G::A);
    group_sync();
    if (t == 0) {
        int n_full = 0;
        double sum_full = 0.0, S = 0.0;
        for (int p = 0; p < T; ++p) if ((mk[p] & MK_KIND_MASK) == MK_FULL) { ++n_full; sum_full = sum_full + s[p]; }
        const double cut = n_full ? fast_factor * (sum_full / (double)n_full) : 0.0;
        for (int p = 0; p < T; ++p) {
            const int kind = mk[p] & MK_KIND_MASK;
            if (kind == MK_FULL || (kind == MK_FAST && s[p] > cut)) S = S + s[p];
        }
        const bool plain = n_full == 0 || !(S > 0.0) || S > 1.7976931348623157e308 || lambda == 0.0;
        sums[0] = plain ? 0.0 : lambda * (double)n_full; sums[1] = S; mean_cut = cut;
    }
    group_sync();
    for (int p = t; p < G::TPAD; p += nT) {
        int c = 0;
        if (p < T) {
            const int kind = mk[p] & MK_KIND_MASK;
            const double w0 = kind == MK_FULL ? 1.0 : 0.0;
            double w = w0;
            if (sums[0] != 0.0) w = (kind == MK_FULL || (kind == MK_FAST && s[p] > mean_cut)) ? (1.0 - lambda) * w0 + (sums[0] * s[p]) / sums[1] : 0.0;
            if (kind == MK_NONE) c = 1;
            else if (w > 0.0) {
                const double fl = (double)(long long)w;                   // floor: w > 0, far below 2^63
                det::Event e; e.key0 = key0; e.key1 = key1; e.slot = (uint32_t)hdr[2]; e.game_seq = (uint32_t)hdr[3];
                e.event = SURPRISE_EVENT + (uint32_t)p; e.tree = 2; e.purpose = det::P_PLAYOUT_CAP;
                c = (int)fl + (det::uniform(e) < w - fl ? 1 : 0);
                if (c > 255) { emu_unreachable(); c = 255; }        // (w <= n_full + 1 <= 226)
            }
        }
        cnt[p] = (uint8_t)c;
    }
    group_sync();
    if (t == 0) {                                                         // the total, held to the table of k_build_samples_w (never reached: rows < 2 T + 1)
        int total = 0, none = 0;
        for (int p = 0; p < T; ++p) {
            int c = cnt[p];
            if (total + c > sample_rows_cap<G>()) { emu_unreachable(); c = sample_rows_cap<G>() - total; cnt[p] = (uint8_t)c; }
            total += c; none += c == 0;
        }
        rows[2 * b] = total; rows[2 * b + 1] = none;
    }
    group_sync();
    for (int p = t; p < G::TPAD; p += nT) counts[(size_t)b * G::TPAD + p] = cnt[p];
}

// k_sample_headers with the rows from k_sample_weights: SAMPLE_HDR_W_INTS per game, [T, winner, slot, game_seq, rows, plies without a row]
constexpr int SAMPLE_HDR_W_INTS = 6;
template <class G> GAZ_SAMPLES_BOUNDS GAZ_KERNEL_WIDE k_sample_headers_w(const uint8_t* ring, int ring_cap, uint32_t first, int n, const int32_t* rows, int32_t* out) {
#ifdef GAZ_HOST_EMU
    const int i = block_id();
#else
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
#endif
    if (i >= n) return;
    const uint8_t* rec = ring + (size_t)((first + (uint32_t)i) % (uint32_t)ring_cap) * RecLayout<G>::SIZE;
    const int32_t* hdr = reinterpret_cast<const int32_t*>(rec + RecLayout<G>::OFF_HDR);
    for (int j = 0; j < 4; ++j) out[SAMPLE_HDR_W_INTS * i + j] = hdr[j];
    out[SAMPLE_HDR_W_INTS * i + 4] = rows[2 * i]; out[SAMPLE_HDR_W_INTS * i + 5] = rows[2 * i + 1];
}

// inclusive prefix sum of v over the workgroup's lanes of one pass, on top of `carry` (the sum of the passes before): every wavefront scans its
// lanes by shuffles, the wavefronts' totals meet in LDS.  -> this lane's inclusive sum; carry grows by the pass's total.  (One-lane emulation: WAVE = 1.)
GAZ_DEV int group_scan(int v, int t, int nT, int* wave_sum, int& carry) {
    const int lane = t % WAVE, wv = t / WAVE, n_wv = (nT + WAVE - 1) / WAVE;
    int x = v;
    for (int d = 1; d < WAVE; d <<= 1) { const int y = shfl(x, lane - d < 0 ? lane : lane - d); if (lane >= d) x += y; }
    if (lane == WAVE - 1) wave_sum[wv] = x;
    group_sync();
    int below = 0, all = 0;
    for (int w = 0; w < n_wv; ++w) { const int c = wave_sum[w]; below += w < wv ? c : 0; all += c; }
    const int incl = carry + below + x;
    carry += all;
    group_sync();
    return incl;
}

// k_build_samples with c_p rows per ply: counts = k_sample_weights' table of the drain window, game b of the plan = record b of the window.
// The compaction is a scan over the counts (end[p] = rows of plies 0 .. p), and "output row -> ply" a table of up to 2 MAXT entries that the
// lanes fill by output row, in passes of nT rows: row j belongs to the first ply whose end exceeds j.  row_ply (may be null) receives it.
template <class G> GAZ_SAMPLES_BOUNDS GAZ_KERNEL_WIDE k_build_samples_w(const uint8_t* ring, int ring_cap, const int32_t* plan, int n, long long R, const uint8_t* counts,
                                                                         int8_t* boards, float* policies, float* values, uint8_t* row_ply) {
    using RL = RecLayout<G>;
    constexpr int SB = G::HW * G::C, NA = SampleAug<G>::N, NEVER = 0x7ffffffe, CAP = sample_rows_cap<G>();
#ifdef GAZ_HOST_EMU
    const int b = block_id(), nT = 1, t = 0;
#else
    const int b = blockIdx.x, nT = blockDim.x, t = threadIdx.x;
#endif
    GAZ_SHARED int fill[G::HW];
    GAZ_SHARED uint8_t act[G::TPAD];
    GAZ_SHARED uint16_t end[G::TPAD];                                     // rows of plies 0 .. p
    GAZ_SHARED uint8_t kept[CAP];                                         // output row -> ply (MAXT <= 255)
    GAZ_SHARED int wave_sum[SAMPLES_THREADS / 64 + 1];
    if (b >= n) return;
    const int slot = plan[b];
    if (slot < 0 || slot >= ring_cap) return;
    const uint8_t* rec = ring + (size_t)slot * RL::SIZE;
    const int32_t* hdr = reinterpret_cast<const int32_t*>(rec + RL::OFF_HDR);
    const int T = sample_plies<G>(hdr[0]), winner = hdr[1];
    const long long row0 = plan[n + b];
    for (int i = t; i < G::HW; i += nT) fill[i] = NEVER;
    for (int i = t; i < T; i += nT) act[i] = rec[RL::OFF_ACT + i];
    int K = 0;
    for (int base = 0; base < T; base += nT) {
        const int p = base + t;
        const int incl = group_scan(p < T ? (int)counts[(size_t)b * G::TPAD + p] : 0, t, nT, wave_sum, K);
        if (p < T) end[p] = (uint16_t)(incl < 0xffff ? incl : 0xffff);
    }
    group_sync();                                                         // (T = 0: no pass ran)
    if (K > CAP || row0 < 0 || row0 + K > R) return;                     // (the host built row0 from k_sample_weights' totals of these very counts)
    for (int j = t; j < K; j += nT) {                                     // the first ply with end[p] > j: j < K = end[T - 1], so there is one
        int lo = 0, hi = T - 1;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if ((int)end[mid] > j) hi = mid; else lo = mid + 1; }
        kept[j] = (uint8_t)lo;
    }
    if (G::ID == GAME_C4) {
        for (int p = t; p < T; p += nT) {                                 // row = 5 - the earlier moves in the same column
            const int a = act[p];
            int below = 0;
            for (int e = 0; e < p; ++e) below += act[e] == a;
            if (a < G::W && below < G::H) fill[(G::H - 1 - below) * G::W + a] = p;
        }
    } else {
        for (int p = t; p < T; p += nT) if (act[p] < G::HW) fill[act[p]] = p;
    }
    group_sync();
    const float* q = reinterpret_cast<const float*>(rec + RL::OFF_Q);
    const float* pol = reinterpret_cast<const float*>(rec + RL::OFF_POL);
    for (int j = t; j < K; j += nT) {                                     // z as in k_build_samples
        const int p = kept[j];
        const float z = (float)(((p & 1) ? 1 : -1) * winner);
        values[row0 + j] = 0.5f * (z + q[p]);
        if (row_ply) row_ply[row0 + j] = (uint8_t)p;
    }
    for (int k = 0; k < NA; ++k) {
        const size_t row = (size_t)k * (size_t)R + (size_t)row0;
        emit_range<int8_t>(boards, row * SB, K * SB, t, nT, [&](int i) { return state_element<G>(fill, kept[i / SB], k, i % SB); });
        emit_range<float>(policies, row * G::A, K * G::A, t, nT, [&](int i) { return pol[kept[i / G::A] * G::A + policy_src_index<G>(k, i % G::A)]; });
    }
}

}  // namespace gaz
