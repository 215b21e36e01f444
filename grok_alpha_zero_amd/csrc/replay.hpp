// replay.hpp — the REPLAY WINDOW (gaz_replay_*): the training rows of the last generations, un-augmented, in device
// memory, and shuffled, augmented minibatches out of them.  What it replaces is the reference's Dataloader.py: re-open the replay files of the
// last generations, turn every row into a list element, balance / split / shuffle and copy minibatches together on the host, one row at a time
// (Dataloader.py:81-145, :178-189).
//
// The store is a circular buffer of rows — state int8 [SB], policy f32 [A], value f32, the row's game (a running number) and its row within that
// game — filled by gaz_replay_append from host arrays as gaz_engine_drain_samples2 returns them (augmentation plane 0 only).  The host mirrors a
// game table (generation, index of the game within its generation in append order, first row, rows).  Whole oldest generations leave when rows
// are needed.  Row s of the STORE ORDER (0 = the oldest live row) lives at physical row (head + s) % capacity.
//
// Every rule is a stateless function of the window's contents and its seed; a row is named (g, i, j) = (generation, game within the generation,
// row within the game), never by its place in the ring.  ph = Philox4x32-10 keyed by seed ^ 0x5245504C41590000, u52 = det::u_half of two words:
//   held-out   u52(ph(g, i, j, 0x80000000)) < test_fraction
//   admission  the reference's parity rule (Dataloader.py:90-105), on the host over the game table: see ReplayWindow::begin_epoch
//   inclusion  game admitted, held-out bit == split, u52(ph(g, i, j, 0x40000000 | epoch)) < max(percent - age * decay, 0)
//   order      position q of the epoch = plan entry perm(q): a 4-round Feistel network on 2 h bits (4^h >= M) with cycle walking
//   symmetry   k = augment ? (ph(epoch, q, split, 0xC0000000)[0] * n_aug) >> 32 : 0, applied with board_src_cell / policy_src_index of
//              samples.hpp, so that a sampled row is byte for byte plane k of gaz_engine_drain_samples for that row
// The epoch's PLAN — the included rows in store order — is built on the device: k_replay_flags (one flag per row, per-block counts by ballot /
// popcount), k_replay_scan (exclusive scan of the block counts, one workgroup, a carry from pass to pass), k_replay_compact.
// k_replay_sample gathers a batch: perm and the symmetry draw once per row, the source rows staged through LDS in whole dwords, the cell map
// applied on the LDS read, the batch's contiguous output written in 16-byte vectors (emit_range).
#pragma once
#include <math.h>
#include <deque>
#include <string>
#include <vector>
#include "samples.hpp"

namespace gaz {

constexpr uint64_t REPLAY_KEY = 0x5245504C41590000ull;
constexpr int REPLAY_THREADS = 256;
constexpr uint32_t REPLAY_C_HELD = 0x80000000u, REPLAY_C_EPOCH = 0x40000000u, REPLAY_C_SYM = 0xC0000000u, REPLAY_C_PERM = 0xC0000010u;

struct ReplayGame { int32_t gen; uint32_t idx; double p; };        // one live game as the flag kernel reads it: p = 0 where the game takes no part

GAZ_DEV double replay_u52(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    const det::U4 r = det::philox(c0, c1, c2, c3, k0, k1);
    return det::u_half(r.x, r.y);
}

// position q of the epoch -> plan entry: exact permutation of [0, M).  q itself lies on the cycle, so the walk ends; no iteration cap
GAZ_DEV uint32_t replay_perm(uint32_t q, uint32_t M, int h, uint32_t epoch, uint32_t split, uint32_t k0, uint32_t k1) {
    const uint32_t mask = (1u << h) - 1u;
    uint32_t x = q;
    do {
        uint32_t L = x >> h, R = x & mask;
        for (uint32_t r = 0; r < 4; ++r) {
            const uint32_t f = det::philox(R, r, epoch, REPLAY_C_PERM | split, k0, k1).x & mask;
            const uint32_t nR = L ^ f;
            L = R; R = nR;
        }
        x = (L << h) | R;
    } while (x >= M);
    return x;
}

// mode 0: the inclusion rule of an epoch; mode 1: the held-out bit alone (gaz_replay_info).  flags[s] and block_counts[b] for the rows
// [256 b, 256 b + 256) of the store order, in passes of nT lanes (the one-lane emulation: 256 passes)
GAZ_SAMPLES_BOUNDS GAZ_KERNEL_WIDE k_replay_flags(const uint32_t* row_game, const uint32_t* row_j, const ReplayGame* gtab, uint32_t game_lo, uint32_t n_live_games,
                                                  long long head, long long cap, long long live, int mode, uint32_t split, uint32_t epoch, double test_fraction,
                                                  uint32_t k0, uint32_t k1, uint8_t* flags, int32_t* block_counts) {
#ifdef GAZ_HOST_EMU
    const int b = block_id(), nT = 1, t = 0;
#else
    const int b = blockIdx.x, nT = blockDim.x, t = threadIdx.x;
#endif
    GAZ_SHARED int wave_cnt[REPLAY_THREADS / 64 + 1];
    const int lane = t % WAVE, wv = t / WAVE, n_wv = (nT + WAVE - 1) / WAVE;
    int K = 0;
    for (int base = 0; base < REPLAY_THREADS; base += nT) {
        const long long s = (long long)b * REPLAY_THREADS + base + t;
        bool keep = false;
        if (s < live) {
            const long long phys = (head + s) % cap;
            const uint32_t gi = row_game[phys] - game_lo;
            if (gi < n_live_games) {
                const ReplayGame ge = gtab[gi];
                const uint32_t j = row_j[phys];
                const bool held = replay_u52((uint32_t)ge.gen, ge.idx, j, REPLAY_C_HELD, k0, k1) < test_fraction;
                if (mode == 1) keep = held;
                else keep = ge.p > 0.0 && (uint32_t)held == split && replay_u52((uint32_t)ge.gen, ge.idx, j, REPLAY_C_EPOCH | epoch, k0, k1) < ge.p;
            }
            flags[s] = keep ? 1 : 0;
        }
        const uint64_t m = ballot(keep);
        if (lane == 0) wave_cnt[wv] = popcll(m);
        group_sync();
        for (int w = 0; w < n_wv; ++w) K += wave_cnt[w];
        group_sync();
    }
    if (t == 0) block_counts[b] = K;
}

// offsets[i] = counts[0] + .. + counts[i - 1], *total = the sum: one workgroup, nb / nT passes with a carry
GAZ_SAMPLES_BOUNDS GAZ_KERNEL_WIDE k_replay_scan(const int32_t* counts, int nb, int32_t* offsets, int32_t* total) {
#ifdef GAZ_HOST_EMU
    const int nT = 1, t = 0;
#else
    const int nT = blockDim.x, t = threadIdx.x;
#endif
    GAZ_SHARED int wave_sum[REPLAY_THREADS / 64 + 1];
    int carry = 0;
    for (int base = 0; base < nb; base += nT) {
        const int i = base + t;
        const int v = i < nb ? counts[i] : 0;
        const int incl = group_scan(v, t, nT, wave_sum, carry);
        if (i < nb) offsets[i] = incl - v;
    }
    if (t == 0) *total = carry;
}

// plan[offsets[b] + (flagged rows of the block below s)] = s for every flagged row s: the included rows in store order
GAZ_SAMPLES_BOUNDS GAZ_KERNEL_WIDE k_replay_compact(const uint8_t* flags, const int32_t* offsets, long long live, uint32_t* plan) {
#ifdef GAZ_HOST_EMU
    const int b = block_id(), nT = 1, t = 0;
#else
    const int b = blockIdx.x, nT = blockDim.x, t = threadIdx.x;
#endif
    GAZ_SHARED int wave_cnt[REPLAY_THREADS / 64 + 1];
    const int lane = t % WAVE, wv = t / WAVE, n_wv = (nT + WAVE - 1) / WAVE;
    const long long off = offsets[b];
    int K = 0;
    for (int base = 0; base < REPLAY_THREADS; base += nT) {
        const long long s = (long long)b * REPLAY_THREADS + base + t;
        const bool keep = s < live && flags[s] != 0;
        const uint64_t m = ballot(keep);
        if (lane == 0) wave_cnt[wv] = popcll(m);
        group_sync();
        int below = 0, all = 0;
        for (int w = 0; w < n_wv; ++w) { const int c = wave_cnt[w]; below += w < wv ? c : 0; all += c; }
        const long long pos = off + K + below + popcll(m & ((1ull << lane) - 1ull));
        if (keep && pos >= 0 && pos < live) plan[pos] = (uint32_t)s;             // (pos < M <= live: the counts are those of these very flags)
        K += all;
        group_sync();
    }
}

// batch rows per workgroup of 256 lanes: many of the small rows, one per wavefront of Gomoku's
template <class G> struct ReplayShape { static constexpr int RB = 64; };
template <> struct ReplayShape<Game<GAME_C4>> { static constexpr int RB = 16; };
template <> struct ReplayShape<Game<GAME_GMK>> { static constexpr int RB = 4; };
template <int C> struct ReplayCell { typedef uint16_t type; };                     // one board cell = its C planes, adjacent bytes of [H][W][C]
template <> struct ReplayCell<4> { typedef uint32_t type; };

// rows [RB b, RB b + RB) of a batch of n rows = positions first + .. of the epoch's order
template <class G> GAZ_SAMPLES_BOUNDS GAZ_KERNEL_WIDE k_replay_sample(const int8_t* st, const float* pol, const float* val, const uint32_t* plan, uint32_t M, int h,
                                                                       long long head, long long cap, uint32_t first, int n, int augment, uint32_t split, uint32_t epoch,
                                                                       uint32_t k0, uint32_t k1, int8_t* ob, float* op, float* ov, uint32_t* orow, uint8_t* osym) {
    constexpr int SB = G::HW * G::C, A = G::A, HW = G::HW, NA = SampleAug<G>::N, RB = ReplayShape<G>::RB;
    constexpr int SDW = (SB + 3 + 3) / 4;                                    // dwords that cover a row starting up to 3 bytes into a dword
    typedef typename ReplayCell<G::C>::type Cell;
    static_assert(SB % sizeof(Cell) == 0 && sizeof(Cell) == G::C, "a row starts on a cell boundary of the output");
#ifdef GAZ_HOST_EMU
    const int b = block_id(), nT = 1, t = 0;
#else
    const int b = blockIdx.x, nT = blockDim.x, t = threadIdx.x;
#endif
    GAZ_SHARED uint32_t s_state[RB * SDW];
    GAZ_SHARED float s_pol[RB * A];
    GAZ_SHARED long long s_phys[RB];
    GAZ_SHARED int s_k[RB];
    const int r0 = b * RB;
    const int nr = n - r0 < RB ? n - r0 : RB;
    if (nr <= 0) return;
    for (int r = t; r < nr; r += nT) {                                        // once per row: the order, the symmetry, the value
        const uint32_t q = first + (uint32_t)(r0 + r);
        long long phys = 0;
        uint32_t e = 0, k = 0;
        if (q < M) {                                                          // (the host refuses first + n > M)
            e = plan[replay_perm(q, M, h, epoch, split, k0, k1)];
            phys = (head + (long long)e) % cap;
            if (augment) k = (uint32_t)(((uint64_t)det::philox(epoch, q, split, REPLAY_C_SYM, k0, k1).x * (uint64_t)NA) >> 32);
        }
        s_phys[r] = phys; s_k[r] = (int)k;
        orow[r0 + r] = e; osym[r0 + r] = (uint8_t)k; ov[r0 + r] = val[phys];
    }
    group_sync();
    const uint32_t* st32 = reinterpret_cast<const uint32_t*>(st);
    for (int idx = t; idx < nr * SDW; idx += nT) {                            // the rows' dwords, consecutive lanes consecutive dwords
        const int r = idx / SDW, d = idx % SDW;
        const long long base = s_phys[r] * SB, a0 = base & ~3ll;
        const int ndw = ((int)(base - a0) + SB + 3) >> 2;                     // (the store has 16 spare bytes behind its last row)
        s_state[idx] = d < ndw ? st32[(a0 >> 2) + d] : 0u;
    }
    for (int idx = t; idx < nr * A; idx += nT) s_pol[idx] = pol[s_phys[idx / A] * A + idx % A];
    group_sync();
    const char* sbytes = reinterpret_cast<const char*>(s_state);
    emit_range<Cell>(reinterpret_cast<Cell*>(ob), (size_t)r0 * HW, nr * HW, t, nT, [&](int i) {
        const int r = i / HW, cell = i % HW;
        const int src = board_src_cell<G>(s_k[r], cell / G::W, cell % G::W);
        Cell v;
        memcpy(&v, sbytes + (size_t)r * SDW * 4 + (int)((s_phys[r] * SB) & 3) + src * (int)sizeof(Cell), sizeof(Cell));
        return v;
    });
    emit_range<float>(op, (size_t)r0 * A, nr * A, t, nT, [&](int i) { const int r = i / A; return s_pol[r * A + policy_src_index<G>(s_k[r], i % A)]; });
}

}  // namespace gaz

// ------------------------------------------------------------------------------------------------------------------------ the host side
struct gaz_replay {
    struct GameEnt { int32_t gen; uint32_t idx; long long row0; int32_t rows; };        // row0: the running number of the game's first row
    struct GenEnt { int32_t gen; long long games, rows; };

    gaz_replay_config cfg;
    std::string err;
    int SB = 0, A = 0, HW = 0;
    long long cap = 0;
    hipStream_t stream = 0;
    bool have_stream = false;
    int8_t* d_state = nullptr; float* d_pol = nullptr; float* d_val = nullptr; uint32_t* d_row_game = nullptr; uint32_t* d_row_j = nullptr;
    uint8_t* d_flags = nullptr; int32_t* d_counts = nullptr; int32_t* d_offsets = nullptr; int32_t* d_total = nullptr; uint32_t* d_plan = nullptr;
    gaz::ReplayGame* d_gtab = nullptr; size_t gtab_cap = 0;
    int8_t* o_boards = nullptr; float* o_pol = nullptr; float* o_val = nullptr; uint32_t* o_rows = nullptr; uint8_t* o_sym = nullptr; long long out_cap = 0;
    long long row_lo = 0, row_hi = 0;                                         // running numbers of the live rows [row_lo, row_hi)
    uint32_t game_lo = 0;                                                     // running number of games.front()
    std::deque<GameEnt> games;
    std::deque<GenEnt> gens;
    bool plan_valid = false; long long plan_M = 0; int plan_h = 1; uint32_t plan_split = 0, plan_epoch = 0;
    int last_n = 0;

    int fail(const std::string& m) { err = m; return 1; }
#define GAZ_RP_CK(expr) \
    do { hipError_t _e = (expr); if (_e != hipSuccess) { return fail(std::string(#expr) + ": " + hipGetErrorString(_e)); } } while (0)
    uint32_t key0() const { return (uint32_t)(cfg.seed ^ gaz::REPLAY_KEY); }
    uint32_t key1() const { return (uint32_t)((cfg.seed ^ gaz::REPLAY_KEY) >> 32); }
    long long live() const { return row_hi - row_lo; }

    ~gaz_replay() {
        if (have_stream) hipStreamSynchronize(stream);
        void* all[] = {d_state, d_pol, d_val, d_row_game, d_row_j, d_flags, d_counts, d_offsets, d_total, d_plan, d_gtab, o_boards, o_pol, o_val, o_rows, o_sym};
        for (void* p : all) if (p) hipFree(p);
        if (have_stream) hipStreamDestroy(stream);
    }

    int init(std::string* why) {
        static const int dims[3][3] = {{9, 2, 9}, {42, 4, 7}, {225, 2, 225}};                    // cells, planes, actions
        HW = dims[cfg.game][0]; SB = HW * dims[cfg.game][1]; A = dims[cfg.game][2];
        cap = cfg.capacity_rows;
        const size_t nb = (size_t)((cap + gaz::REPLAY_THREADS - 1) / gaz::REPLAY_THREADS);
        bool ok = hipSetDevice(cfg.device) == hipSuccess && hipStreamCreate(&stream) == hipSuccess;
        have_stream = ok;
        ok = ok && hipMalloc((void**)&d_state, (size_t)cap * SB + 16) == hipSuccess && hipMalloc((void**)&d_pol, (size_t)cap * A * 4) == hipSuccess
                && hipMalloc((void**)&d_val, (size_t)cap * 4) == hipSuccess && hipMalloc((void**)&d_row_game, (size_t)cap * 4) == hipSuccess
                && hipMalloc((void**)&d_row_j, (size_t)cap * 4) == hipSuccess && hipMalloc((void**)&d_flags, (size_t)cap) == hipSuccess
                && hipMalloc((void**)&d_counts, nb * 4) == hipSuccess && hipMalloc((void**)&d_offsets, nb * 4) == hipSuccess
                && hipMalloc((void**)&d_total, 16) == hipSuccess && hipMalloc((void**)&d_plan, (size_t)cap * 4) == hipSuccess;
        if (ok) ok = hipMemset(d_state + (size_t)cap * SB, 0, 16) == hipSuccess;            // the spare bytes behind the last row: a staged row's last dword may end there
        if (!ok) { *why = "replay_create: allocation failure: a window of " + std::to_string(cap) + " rows does not fit on device " + std::to_string(cfg.device); (void)hipGetLastError(); }
        return ok ? 0 : 1;
    }

    // rows [a, a + n) of the running numbering <-> the ring: at most two pieces
    template <class F> int ring_pieces(long long a, long long n, F f) {
        long long done = 0;
        while (done < n) {
            const long long phys = (a + done) % cap;
            const long long len = n - done < cap - phys ? n - done : cap - phys;
            if (f(phys, done, len)) return 1;
            done += len;
        }
        return 0;
    }

    void drop_oldest_generation() {
        const GenEnt g = gens.front();
        gens.pop_front();
        for (long long i = 0; i < g.games; ++i) { games.pop_front(); ++game_lo; }
        row_lo += g.rows;
        plan_valid = false;
    }

    int append(int32_t generation, int32_t n_games, const int32_t* g6, const int8_t* boards, const float* policies, const float* values, int64_t n_rows) {
        if (n_games < 0 || n_rows < 0) return fail("replay_append: n_games and n_rows must not be negative");
        if (n_games > 0 && !g6) return fail("replay_append: null games");
        if (n_rows > 0 && (!boards || !policies || !values)) return fail("replay_append: null arrays");
        if (!gens.empty() && generation < gens.back().gen)
            return fail("replay_append: generation " + std::to_string(generation) + " after generation " + std::to_string(gens.back().gen) + ": generations must arrive in non-decreasing order");
        if (n_games == 0) { if (n_rows) return fail("replay_append: rows without a game"); return 0; }
        const long long base = g6[4];
        std::vector<long long> r0((size_t)n_games + 1);
        for (int i = 0; i < n_games; ++i) r0[i] = (long long)g6[(size_t)6 * i + 4] - base;
        r0[n_games] = n_rows;
        for (int i = 0; i < n_games; ++i)
            if (r0[i] < 0 || r0[i + 1] < r0[i] || r0[i + 1] > n_rows || r0[i + 1] - r0[i] > 0x7fffffff)
                return fail("replay_append: the first rows of the games (games[i][4]) are not ascending within n_rows, at game " + std::to_string(i));
        const bool same = !gens.empty() && gens.back().gen == generation;
        const long long gen_rows = (same ? gens.back().rows : 0) + n_rows;
        if (gen_rows > cap)
            return fail("replay_append: generation " + std::to_string(generation) + " alone has " + std::to_string(gen_rows) + " rows, capacity_rows is " + std::to_string(cap));
        GAZ_RP_CK(hipStreamSynchronize(stream));
        while (live() + n_rows > cap) drop_oldest_generation();                  // never the one being appended to: gen_rows <= cap
        std::vector<uint32_t> rg((size_t)n_rows), rj((size_t)n_rows);
        uint32_t idx = same ? (uint32_t)gens.back().games : 0u;
        if (!same) gens.push_back(GenEnt{generation, 0, 0});
        for (int i = 0; i < n_games; ++i) {
            const uint32_t seq = game_lo + (uint32_t)games.size();
            games.push_back(GameEnt{generation, idx++, row_hi + r0[i], (int32_t)(r0[i + 1] - r0[i])});
            for (long long r = r0[i]; r < r0[i + 1]; ++r) { rg[(size_t)r] = seq; rj[(size_t)r] = (uint32_t)(r - r0[i]); }
        }
        gens.back().games += n_games; gens.back().rows += n_rows;
        const long long at = row_hi;
        row_hi += n_rows;
        plan_valid = false;
        if (ring_pieces(at, n_rows, [&](long long phys, long long done, long long len) {
                GAZ_RP_CK(hipMemcpyAsync(d_state + phys * SB, boards + done * SB, (size_t)len * SB, hipMemcpyHostToDevice, stream));
                GAZ_RP_CK(hipMemcpyAsync(d_pol + phys * A, policies + done * A, (size_t)len * A * 4, hipMemcpyHostToDevice, stream));
                GAZ_RP_CK(hipMemcpyAsync(d_val + phys, values + done, (size_t)len * 4, hipMemcpyHostToDevice, stream));
                GAZ_RP_CK(hipMemcpyAsync(d_row_game + phys, rg.data() + done, (size_t)len * 4, hipMemcpyHostToDevice, stream));
                GAZ_RP_CK(hipMemcpyAsync(d_row_j + phys, rj.data() + done, (size_t)len * 4, hipMemcpyHostToDevice, stream));
                return 0;
            })) return 1;
        GAZ_RP_CK(hipStreamSynchronize(stream));
        return 0;
    }

    int evict(int32_t before_generation) {
        GAZ_RP_CK(hipStreamSynchronize(stream));
        while (!gens.empty() && gens.front().gen < before_generation) drop_oldest_generation();
        plan_valid = false;
        return 0;
    }

    int upload_games(const std::vector<double>* p) {
        const size_t n = games.size();
        if (n > gtab_cap) {
            if (d_gtab) { GAZ_RP_CK(hipFree(d_gtab)); d_gtab = nullptr; gtab_cap = 0; }
            const size_t want = n + n / 2 + 64;
            if (hipMalloc((void**)&d_gtab, want * sizeof(gaz::ReplayGame)) != hipSuccess) { (void)hipGetLastError(); return fail("replay: allocation failure (game table of " + std::to_string(n) + " games)"); }
            gtab_cap = want;
        }
        std::vector<gaz::ReplayGame> tab(n);
        for (size_t i = 0; i < n; ++i) tab[i] = gaz::ReplayGame{games[i].gen, games[i].idx, p ? (*p)[i] : 0.0};
        if (n) GAZ_RP_CK(hipMemcpyAsync(d_gtab, tab.data(), n * sizeof(gaz::ReplayGame), hipMemcpyHostToDevice, stream));
        GAZ_RP_CK(hipStreamSynchronize(stream));                                  // (tab is a local)
        return 0;
    }

    // flags + block counts + scan (+ compaction into the plan) -> the number of flagged rows
    int count_rows(int mode, uint32_t split, uint32_t epoch, bool compact, long long* total) {
        *total = 0;
        const long long n = live();
        if (n == 0) return 0;
        const int nb = (int)((n + gaz::REPLAY_THREADS - 1) / gaz::REPLAY_THREADS);
        GAZ_LAUNCH(gaz::k_replay_flags, nb, gaz::REPLAY_THREADS, stream, d_row_game, d_row_j, d_gtab, game_lo, (uint32_t)games.size(), row_lo % cap, cap, n, mode, split, epoch,
                   cfg.test_fraction, key0(), key1(), d_flags, d_counts);
        GAZ_LAUNCH(gaz::k_replay_scan, 1, gaz::REPLAY_THREADS, stream, d_counts, nb, d_offsets, d_total);
        if (compact) GAZ_LAUNCH(gaz::k_replay_compact, nb, gaz::REPLAY_THREADS, stream, d_flags, d_offsets, n, d_plan);
        GAZ_RP_CK(hipGetLastError());
        int32_t t = 0;
        GAZ_RP_CK(hipMemcpyAsync(&t, d_total, 4, hipMemcpyDeviceToHost, stream));
        GAZ_RP_CK(hipStreamSynchronize(stream));
        *total = t;
        return 0;
    }

    int info(int64_t out[8], int32_t max_gens, int64_t* g3, int32_t* n_gens) {
        if (!out) return fail("replay_info: null argument");
        long long held = 0;
        if (cfg.test_fraction > 0.0 && live() > 0)                            // (flags, counts and the game table are scratch of the plan builder: a plan stays)
            if (upload_games(nullptr) || count_rows(1, 0, 0, false, &held)) return 1;
        out[0] = live(); out[1] = (int64_t)games.size(); out[2] = gens.empty() ? -1 : gens.front().gen; out[3] = gens.empty() ? -1 : gens.back().gen;
        out[4] = held; out[5] = cap; out[6] = (int64_t)gens.size(); out[7] = plan_valid ? plan_M : -1;
        if (n_gens) *n_gens = (int32_t)gens.size();
        for (size_t i = 0; g3 && i < gens.size() && (int32_t)i < max_gens; ++i) { g3[3 * i] = gens[i].gen; g3[3 * i + 1] = gens[i].games; g3[3 * i + 2] = gens[i].rows; }
        return 0;
    }

    int read_rows(int64_t first, int64_t n, int8_t* boards, float* policies, float* values, int32_t* meta) {
        if (first < 0 || n < 0 || first + n > live()) return fail("replay_read_rows: rows " + std::to_string(first) + " .. " + std::to_string(first + n) + " of " + std::to_string(live()) + " live rows");
        if (n == 0) return 0;
        GAZ_RP_CK(hipStreamSynchronize(stream));
        std::vector<uint32_t> rg(meta ? (size_t)n : 0);
        if (ring_pieces(row_lo + first, n, [&](long long phys, long long done, long long len) {
                if (boards) GAZ_RP_CK(hipMemcpyAsync(boards + done * SB, d_state + phys * SB, (size_t)len * SB, hipMemcpyDeviceToHost, stream));
                if (policies) GAZ_RP_CK(hipMemcpyAsync(policies + done * A, d_pol + phys * A, (size_t)len * A * 4, hipMemcpyDeviceToHost, stream));
                if (values) GAZ_RP_CK(hipMemcpyAsync(values + done, d_val + phys, (size_t)len * 4, hipMemcpyDeviceToHost, stream));
                if (meta) GAZ_RP_CK(hipMemcpyAsync(rg.data() + done, d_row_game + phys, (size_t)len * 4, hipMemcpyDeviceToHost, stream));
                return 0;
            })) return 1;
        GAZ_RP_CK(hipStreamSynchronize(stream));
        for (int64_t r = 0; meta && r < n; ++r) {                                 // (generation, game within it, row within the game) from the host's table
            const uint32_t gi = rg[(size_t)r] - game_lo;
            if (gi >= games.size()) return fail("replay_read_rows: a stored row names no live game");
            const GameEnt& ge = games[gi];
            meta[3 * r] = ge.gen; meta[3 * r + 1] = (int32_t)ge.idx; meta[3 * r + 2] = (int32_t)(row_lo + first + r - ge.row0);
        }
        return 0;
    }

    // ADMISSION is the reference's parity rule (Dataloader.py:90-105), kept as it is: a game counts as won by the first player iff it has an odd
    // number of rows.  Known blind spots: a draw on a board with an odd number of cells counts as a first-player win, a resigned game has the
    // parity of the resigner's last ply, and a game thinned by the playout cap, the surprise weighting or a book prefix has whatever parity is left.
    int begin_epoch(int32_t split, uint32_t epoch, int32_t newest, double percent, double decay, int64_t* n_rows) {
        if (n_rows) *n_rows = 0;
        if (split != 0 && split != 1) return fail("replay_begin_epoch: split must be 0 (train) or 1 (test), not " + std::to_string(split));
        if (epoch >= (1u << 30)) return fail("replay_begin_epoch: epoch must be below 2^30");
        if (percent != percent || decay != decay) return fail("replay_begin_epoch: percent and decay must not be NaN");
        plan_valid = false;
        std::vector<double> p(games.size(), 0.0);
        const bool balance = cfg.target_ratio == cfg.target_ratio;
        long long f = 0, s = 0;
        size_t end = games.size();
        for (size_t gi = gens.size(); gi-- > 0;) {                                // newest generation first, its games in append order
            const size_t begin = end - (size_t)gens[gi].games;
            if (gens[gi].gen <= newest) {
                const double pg0 = percent - (double)((long long)newest - gens[gi].gen) * decay;
                const double pg = pg0 > 0.0 ? pg0 : 0.0;
                for (size_t k = begin; k < end; ++k) {
                    bool admit = true;
                    if (balance) {
                        const double ratio = f + s == 0 ? 0.0 : (double)f / (double)(f + s);
                        if (games[k].rows & 1) { if (ratio - 0.02 > cfg.target_ratio) admit = false; else ++f; }
                        else { if (ratio + 0.02 < cfg.target_ratio) admit = false; else ++s; }
                    }
                    p[k] = admit ? pg : 0.0;
                }
            }
            end = begin;
        }
        long long M = 0;
        if (upload_games(&p) || count_rows(0, (uint32_t)split, epoch, true, &M)) return 1;
        int h = 1;
        while ((1ll << (2 * h)) < M) ++h;
        plan_valid = true; plan_M = M; plan_h = h; plan_split = (uint32_t)split; plan_epoch = epoch;
        if (n_rows) *n_rows = M;
        return 0;
    }

    int read_plan(int64_t first, int64_t n, uint32_t* rows) {
        if (!plan_valid) return fail("replay_read_plan: no plan: call gaz_replay_begin_epoch (append and evict drop the plan)");
        if (first < 0 || n < 0 || first + n > plan_M) return fail("replay_read_plan: entries " + std::to_string(first) + " .. " + std::to_string(first + n) + " of a plan of " + std::to_string(plan_M));
        if (n && !rows) return fail("replay_read_plan: null argument");
        if (n) GAZ_RP_CK(hipMemcpyAsync(rows, d_plan + first, (size_t)n * 4, hipMemcpyDeviceToHost, stream));
        GAZ_RP_CK(hipStreamSynchronize(stream));
        return 0;
    }

    int grow_outputs(long long n) {
        if (n <= out_cap) return 0;
        GAZ_RP_CK(hipStreamSynchronize(stream));
        void** ptrs[] = {(void**)&o_boards, (void**)&o_pol, (void**)&o_val, (void**)&o_rows, (void**)&o_sym};
        for (void** pp : ptrs) if (*pp) { GAZ_RP_CK(hipFree(*pp)); *pp = nullptr; }
        out_cap = 0;
        const long long want = n + n / 2 < 256 ? 256 : n + n / 2;
        const size_t bytes[] = {(size_t)want * SB, (size_t)want * A * 4, (size_t)want * 4, (size_t)want * 4, (size_t)want};
        for (int i = 0; i < 5; ++i)
            if (hipMalloc(ptrs[i], bytes[i]) != hipSuccess) { (void)hipGetLastError(); return fail("replay_sample: allocation failure (output buffers of " + std::to_string(want) + " rows)"); }
        out_cap = want;
        return 0;
    }

    template <class G> void launch_sample(uint32_t first, int n, int augment) {
        const int nb = (n + gaz::ReplayShape<G>::RB - 1) / gaz::ReplayShape<G>::RB;
        GAZ_LAUNCH(gaz::k_replay_sample<G>, nb, gaz::REPLAY_THREADS, stream, d_state, d_pol, d_val, d_plan, (uint32_t)plan_M, plan_h, row_lo % cap, cap, first, n, augment,
                   plan_split, plan_epoch, key0(), key1(), o_boards, o_pol, o_val, o_rows, o_sym);
    }

    int sample(int64_t first, int32_t n, int32_t augment) {
        if (!plan_valid) return fail("replay_sample: no plan: call gaz_replay_begin_epoch (append and evict drop the plan)");
        if (first < 0 || n < 0 || first + n > plan_M)
            return fail("replay_sample: positions " + std::to_string(first) + " .. " + std::to_string(first + n) + " of an epoch of " + std::to_string(plan_M) + " rows");
        last_n = n;
        if (n == 0) return 0;
        if (grow_outputs(n)) return 1;
        if (cfg.game == GAZ_GAME_TICTACTOE) launch_sample<gaz::Game<gaz::GAME_TTT>>((uint32_t)first, n, augment != 0);
        else if (cfg.game == GAZ_GAME_CONNECT4) launch_sample<gaz::Game<gaz::GAME_C4>>((uint32_t)first, n, augment != 0);
        else launch_sample<gaz::Game<gaz::GAME_GMK>>((uint32_t)first, n, augment != 0);
        GAZ_RP_CK(hipGetLastError());
        return 0;
    }

    // measurement hook (tools/replay_bench.py): `repeats` gathers of the same batch between two HIP events on the window's stream
    int sample_timed(int64_t first, int32_t n, int32_t augment, int32_t repeats, double* ms_per_batch) {
        if (repeats < 1 || !ms_per_batch) return fail("replay_sample_timed: repeats must be at least 1");
        if (sample(first, n, augment)) return 1;                                  // (checks, grows the buffers, warms up)
        hipEvent_t e0, e1;
        GAZ_RP_CK(hipEventCreate(&e0)); GAZ_RP_CK(hipEventCreate(&e1));
        GAZ_RP_CK(hipEventRecord(e0, stream));
        int rc = 0;
        for (int i = 0; i < repeats && !rc; ++i) rc = sample(first, n, augment);
        GAZ_RP_CK(hipEventRecord(e1, stream));
        GAZ_RP_CK(hipEventSynchronize(e1));
        float ms = 0.f;
        GAZ_RP_CK(hipEventElapsedTime(&ms, e0, e1));
        GAZ_RP_CK(hipEventDestroy(e0)); GAZ_RP_CK(hipEventDestroy(e1));
        *ms_per_batch = (double)ms / repeats;
        return rc;
    }

    int read_batch(int8_t* boards, float* policies, float* values, uint32_t* rows, uint8_t* sym) {
        const size_t n = (size_t)last_n;
        if (n) {
            if (boards) GAZ_RP_CK(hipMemcpyAsync(boards, o_boards, n * SB, hipMemcpyDeviceToHost, stream));
            if (policies) GAZ_RP_CK(hipMemcpyAsync(policies, o_pol, n * A * 4, hipMemcpyDeviceToHost, stream));
            if (values) GAZ_RP_CK(hipMemcpyAsync(values, o_val, n * 4, hipMemcpyDeviceToHost, stream));
            if (rows) GAZ_RP_CK(hipMemcpyAsync(rows, o_rows, n * 4, hipMemcpyDeviceToHost, stream));
            if (sym) GAZ_RP_CK(hipMemcpyAsync(sym, o_sym, n, hipMemcpyDeviceToHost, stream));
        }
        GAZ_RP_CK(hipStreamSynchronize(stream));
        return 0;
    }
#undef GAZ_RP_CK
};

static std::string g_replay_create_error;

extern "C" {

int gaz_replay_config_size(void) { return (int)sizeof(gaz_replay_config); }

int gaz_replay_create(const gaz_replay_config* cfg, gaz_replay** out) {
    std::string& e = g_replay_create_error;
    if (!cfg || !out) { e = "replay_create: null argument"; return 1; }
    *out = nullptr;
    if (cfg->struct_size != sizeof(gaz_replay_config)) {
        e = "gaz_replay_config.struct_size is " + std::to_string(cfg->struct_size) + ", this library's gaz_replay_config has " + std::to_string(sizeof(gaz_replay_config)) +
            " bytes: rebuild the binding from include/gaz_engine.h";
        return 1;
    }
    if (cfg->game < 0 || cfg->game > 2) { e = "replay_create: unknown game " + std::to_string(cfg->game); return 1; }
    if (cfg->capacity_rows < 1 || cfg->capacity_rows > 0x7fffffffll) { e = "replay_create: capacity_rows must be in [1, 2^31 - 1], not " + std::to_string(cfg->capacity_rows); return 1; }
    if (!(cfg->test_fraction >= 0.0 && cfg->test_fraction < 1.0)) { e = "replay_create: test_fraction must be in [0, 1)"; return 1; }
    if (cfg->target_ratio == cfg->target_ratio && !(cfg->target_ratio >= 0.0 && cfg->target_ratio <= 1.0)) { e = "replay_create: target_ratio must be NaN (no balancing) or in [0, 1]"; return 1; }
    gaz_replay* h = new gaz_replay();
    h->cfg = *cfg;
    if (h->init(&e)) { delete h; return 1; }
    *out = h;
    return 0;
}
void gaz_replay_destroy(gaz_replay* h) { delete h; }
const char* gaz_replay_last_error(gaz_replay* h) { return h ? h->err.c_str() : g_replay_create_error.c_str(); }
int gaz_replay_append(gaz_replay* h, int32_t generation, int32_t n_games, const int32_t* games, const int8_t* boards, const float* policies, const float* values, int64_t n_rows) {
    return h->append(generation, n_games, games, boards, policies, values, n_rows);
}
int gaz_replay_evict(gaz_replay* h, int32_t before_generation) { return h->evict(before_generation); }
int gaz_replay_info(gaz_replay* h, int64_t out[8], int32_t max_generations, int64_t* generations, int32_t* n_generations) { return h->info(out, max_generations, generations, n_generations); }
int gaz_replay_read_rows(gaz_replay* h, int64_t first, int64_t n, int8_t* boards, float* policies, float* values, int32_t* meta) { return h->read_rows(first, n, boards, policies, values, meta); }
int gaz_replay_begin_epoch(gaz_replay* h, int32_t split, uint32_t epoch, int32_t newest_generation, double percent, double decay, int64_t* n_rows) {
    return h->begin_epoch(split, epoch, newest_generation, percent, decay, n_rows);
}
int gaz_replay_read_plan(gaz_replay* h, int64_t first, int64_t n, uint32_t* rows) { return h->read_plan(first, n, rows); }
int gaz_replay_sample(gaz_replay* h, int64_t first, int32_t n, int32_t augment) { return h->sample(first, n, augment); }
int gaz_replay_sample_timed(gaz_replay* h, int64_t first, int32_t n, int32_t augment, int32_t repeats, double* ms_per_batch) { return h->sample_timed(first, n, augment, repeats, ms_per_batch); }
int gaz_replay_batch_ptrs(gaz_replay* h, void** boards, void** policies, void** values, void** rows, void** sym) {
    if (boards) *boards = h->o_boards;
    if (policies) *policies = h->o_pol;
    if (values) *values = h->o_val;
    if (rows) *rows = h->o_rows;
    if (sym) *sym = h->o_sym;
    return 0;
}
int gaz_replay_read_batch(gaz_replay* h, int8_t* boards, float* policies, float* values, uint32_t* rows, uint8_t* sym) { return h->read_batch(boards, policies, values, rows, sym); }
int gaz_replay_synchronize(gaz_replay* h) {
    const hipError_t e = hipStreamSynchronize(h->stream);
    return e == hipSuccess ? 0 : h->fail(std::string("replay_synchronize: ") + hipGetErrorString(e));
}

}  // extern "C"
