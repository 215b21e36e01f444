// score.hpp — HELD-OUT LOSS on the device (gaz_engine_score_outputs / gaz_engine_score_replay): what a network's
// predictions score on training rows — cross entropy, target entropy, squared value error, top-1 and value-sign agreement.  It replaces the
// reference's validation pass (Train.py:46-57: model.fit(validation_data=...) with Net/Alpha_Loss.py or Net/Gumbel_Loss.py as the losses and KL
// divergence as the metric), for the network self-play really runs: the engine's own evaluator with its imported weights.
//
// THE RULE is stated in include/gaz_engine.h ("HELD-OUT LOSS") and restated by tests/score_model.py; everything is float64 out of operations the
// project pins bit for bit (det::dexp, det::dlog, numpy's pairwise sum), so the device, the one-lane build and the model agree in every bit.
//
// k_score_rows<G>: one row per TEAM — 16 lanes for A <= 16 (TicTacToe, Connect4: four rows per wavefront, as the PUCT teams), the whole wavefront
// for Gomoku's 225 actions.  A lane takes the entries a = lane, lane + TEAM, .. and stages P and y as doubles in its team's LDS; the argmaxes
// over the raw prediction and the target are DPP reductions within the 16-lane row (quad_perm, row_half_mirror, row_mirror) and, for the wavefront team, four v_readlane on top; "bad" is a
// ballot.  The activation's terms and the products y * log(q), y * log(y) are STORED into per-team LDS doubles and then summed in numpy's order
// (det::np_pairwise_sum) — a stored product cannot be contracted into the first addition (the build also passes -ffp-contract=off).
// k_score_blocks: one wavefront per block of 128 rows: three det::np_sum_block and four popcounts of ballots.  No atomics, vector stores only.
#pragma once
#include <string>
#include <vector>
#include "det.hpp"
#include "evaluator.hpp"
#include "samples.hpp"

namespace gaz {

constexpr int SCORE_THREADS = 256, SCORE_BLOCK_ROWS = 128;
enum : int { SCORE_ACT_NONE = 0, SCORE_ACT_SOFTMAX = 1, SCORE_ACT_STABLEMAX = 2 };
enum : uint8_t { SCORE_TOP1 = 1, SCORE_VSIGN = 2, SCORE_VROW = 4, SCORE_BAD = 8 };

template <class G> struct ScoreShape {
    static constexpr int HW_TEAM = G::A <= 16 ? 16 : 64;                     // lanes of a row's team on the device
    static constexpr int TEAM = GAZ_TEAM(HW_TEAM);                           // (1 on the one-lane build)
    static constexpr int RPB = SCORE_THREADS / HW_TEAM;                      // rows per workgroup
    static constexpr int SA = G::A < 8 ? 8 : G::A;                           // LDS doubles per row and array (np_sum_block reads at least 7)
};

GAZ_DEV bool score_finite(float x) { uint32_t u; memcpy(&u, &x, 4); return (u & 0x7F800000u) != 0x7F800000u; }

#ifndef GAZ_HOST_EMU
template <int CTRL> GAZ_DEV void score_argmax_dpp(float& s, int& i) {        // (value, index) of the lane CTRL names; larger value, then LOWER index
    int sb; memcpy(&sb, &s, 4);
    const int ob = __builtin_amdgcn_update_dpp(0, sb, CTRL, 0xF, 0xF, false);
    const int oi = __builtin_amdgcn_update_dpp(0, i, CTRL, 0xF, 0xF, false);
    float os; memcpy(&os, &ob, 4);
    if (os > s || (os == s && oi < i)) { s = os; i = oi; }
}
#endif
// argmax over the team, lowest index among equals (np.argmax): every lane ends with the result.  All lanes of the wavefront are active here.
template <int HW_TEAM> GAZ_DEV void score_team_argmax(float& s, int& i) {
#ifndef GAZ_HOST_EMU
    score_argmax_dpp<0xB1>(s, i);                                            // quad_perm [1, 0, 3, 2]
    score_argmax_dpp<0x4E>(s, i);                                            // quad_perm [2, 3, 0, 1]
    score_argmax_dpp<0x141>(s, i);                                           // row_half_mirror: the other quad of the half row
    score_argmax_dpp<0x140>(s, i);                                           // row_mirror: the other half of the 16-lane row
    if (HW_TEAM == 64) {
        int sb; memcpy(&sb, &s, 4);
        float bs = s; int bi = i;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int ob = __builtin_amdgcn_readlane(sb, 16 * r), oi = __builtin_amdgcn_readlane(i, 16 * r);
            float os; memcpy(&os, &ob, 4);
            if (r == 0 || os > bs || (os == bs && oi < bi)) { bs = os; bi = oi; }
        }
        s = bs; i = bi;
    }
#endif
}

// one row: `row` of this launch (P, V, Y, Z start at the launch's first row), written at out_row of the per-row arrays.  live = false: the
// team takes every step and touches no memory outside its LDS
template <class G> GAZ_DEV void score_row(const float* P, const float* V, const float* Y, const float* Z, long long row, long long out_row, bool live, int tl, int tw, int act, int n_act,
                                          double* sX, double* sC, double* sE, double* row_ce, double* row_ent, double* row_se, uint8_t* row_flags) {
    typedef ScoreShape<G> S;
    constexpr int A = G::A, T = S::TEAM, NONE = 0x7fffffff;
    // the length of the three sums: a kernel argument (= A) for the wide head, so that the compiler does not unroll np_sum_block over 225 LDS reads
    // held in registers at once (512 VGPRs and 1.6 KB of scratch per lane when it did); the small heads' sums unroll into a handful of registers
    const int n_sum = A > 64 ? n_act : A;
    const float NEG_INF = -__builtin_inff();
    bool bad = false;
    float bp = NEG_INF, by = NEG_INF; int bpi = NONE, byi = NONE;
    // ---- stage P and y as doubles; the lane's share of the argmaxes and of "bad"
#pragma unroll 1
    for (int a = tl; a < A; a += T) {
        const float p = live ? P[row * A + a] : 0.f, y = live ? Y[row * A + a] : 0.f;
        if (!score_finite(p)) bad = true;
        if (bpi == NONE || p > bp) { bp = p; bpi = a; }                        // (a ascends: the first of equals stays)
        if (byi == NONE || y > by) { by = y; byi = a; }
        sX[a] = (double)p; sC[a] = (double)y;
    }
    const float v = live ? V[row] : 0.f, z = live ? Z[row] : 0.f;
    if (!score_finite(v)) bad = true;
    const uint64_t bm = ballot(bad);
    const bool team_bad = ((T >= 64 ? bm : (bm >> (tw * (T & 63))) & ((1ull << (T & 63)) - 1ull))) != 0;
    score_team_argmax<S::HW_TEAM>(bp, bpi);
    score_team_argmax<S::HW_TEAM>(by, byi);
    const bool good = live && !team_bad;
    // ---- the prediction as probabilities q = sX[a] / tot
    double tot = 1.0;
    if (act != SCORE_ACT_NONE) {
        const double c = -(good ? (double)bp : 0.0);
#pragma unroll 1
        for (int a = tl; a < A; a += T) {
            const double x = good ? sX[a] : 0.0;
            sX[a] = act == SCORE_ACT_SOFTMAX ? det::dexp(x + c) : (x >= 0.0 ? x + 1.0 : 1.0 / (1.0 - x));
        }
        wave_sync();
        tot = det::np_pairwise_sum<double, S::SA>(sX, n_sum);
    }
    // ---- the terms, stored before they are summed
#pragma unroll 1
    for (int a = tl; a < A; a += T) {
        const double q = act != SCORE_ACT_NONE ? sX[a] / tot : sX[a], y = sC[a];
        const bool on = good && y > 0.0;
        const double yd = on ? y : 1.0;
        const double qc = (good && q > 1e-7) ? q : 1e-7;
        const double tc = yd * det::dlog(qc), te = yd * det::dlog(yd);
        sC[a] = on ? tc : 0.0; sE[a] = on ? te : 0.0;
    }
    wave_sync();
    const double ce = -det::np_pairwise_sum<double, S::SA>(sC, n_sum), ent = -det::np_pairwise_sum<double, S::SA>(sE, n_sum);
    wave_sync();                                                              // (the one-lane build runs the block's rows one after the other)
    if (tl == 0 && live) {
        const double d = (double)v - (double)z;
        const double se = d * d;
        uint8_t f = SCORE_BAD;
        if (good) f = (uint8_t)((bpi == byi ? SCORE_TOP1 : 0) | (z != 0.f && (double)v * (double)z > 0.0 ? SCORE_VSIGN : 0) | (z != 0.f ? SCORE_VROW : 0));
        row_ce[out_row] = good ? ce : 0.0; row_ent[out_row] = good ? ent : 0.0; row_se[out_row] = good ? se : 0.0; row_flags[out_row] = f;
    }
}

// rows [RPB b, RPB b + RPB) of a launch of n rows; row r is written at base + r
template <class G> GAZ_SAMPLES_BOUNDS GAZ_KERNEL_WIDE k_score_rows(const float* P, const float* V, const float* Y, const float* Z, int n, long long base, int act, int n_act,
                                                                    double* row_ce, double* row_ent, double* row_se, uint8_t* row_flags) {
    typedef ScoreShape<G> S;
    GAZ_SHARED double sX[S::RPB * S::SA];
    GAZ_SHARED double sC[S::RPB * S::SA];
    GAZ_SHARED double sE[S::RPB * S::SA];
#ifdef GAZ_HOST_EMU
    for (int tm = 0; tm < S::RPB; ++tm) {
        const long long row = (long long)block_id() * S::RPB + tm;
        score_row<G>(P, V, Y, Z, row, base + row, row < n, 0, 0, act, n_act, sX + tm * S::SA, sC + tm * S::SA, sE + tm * S::SA, row_ce, row_ent, row_se, row_flags);
    }
#else
    const int tm = threadIdx.x / S::HW_TEAM, tl = threadIdx.x % S::HW_TEAM;
    const long long row = (long long)blockIdx.x * S::RPB + tm;
    score_row<G>(P, V, Y, Z, row, base + row, row < n, tl, (threadIdx.x & 63) / S::HW_TEAM, act, n_act, sX + tm * S::SA, sC + tm * S::SA, sE + tm * S::SA, row_ce, row_ent, row_se, row_flags);
#endif
}

// block b = rows [128 b, 128 b + 128) of M: partials[b][3] = np.sum of ce, entropy, se; counts[b][4] = rows with top1, value sign, z != 0, bad.
// One wavefront per block, four per workgroup.  (The per-row arrays have 8 spare elements: np_sum_block reads seven whatever the length.)
GAZ_SAMPLES_BOUNDS GAZ_KERNEL_WIDE k_score_blocks(const double* row_ce, const double* row_ent, const double* row_se, const uint8_t* row_flags, long long M,
                                                  double* partials, uint32_t* counts) {
#ifdef GAZ_HOST_EMU
    for (int w = 0; w < SCORE_THREADS / 64; ++w) {
        const long long b = (long long)block_id() * (SCORE_THREADS / 64) + w;
#else
    {
        const long long b = (long long)blockIdx.x * (SCORE_THREADS / 64) + threadIdx.x / 64;
#endif
        const long long r0 = b * SCORE_BLOCK_ROWS;
        if (r0 < M) {                                                        // (uniform in the wavefront)
            const int len = M - r0 < SCORE_BLOCK_ROWS ? (int)(M - r0) : SCORE_BLOCK_ROWS;
            const int lane = lane_id();
            for (int l = lane; l < 3; l += WAVE) {
                const double* src = l == 0 ? row_ce : (l == 1 ? row_ent : row_se);
                partials[b * 3 + l] = det::np_sum_block(src + r0, len);
            }
            uint32_t c[4] = {0, 0, 0, 0};
            for (int i0 = 0; i0 < SCORE_BLOCK_ROWS; i0 += WAVE) {
                const int i = i0 + lane;
                const uint8_t f = i < len ? row_flags[r0 + i] : (uint8_t)0;
#pragma unroll
                for (int k = 0; k < 4; ++k) c[k] += (uint32_t)popcll(ballot(((f >> k) & 1) != 0));
            }
            if (lane == 0) { counts[b * 4 + 0] = c[0]; counts[b * 4 + 1] = c[1]; counts[b * 4 + 2] = c[2]; counts[b * 4 + 3] = c[3]; }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------ the host side
// The buffers and launches of both entry points; owned by the engine handle, made on first use.  Every call ends with the stream idle.
struct ScoreState {
    int game = 0, A = 0, device = 0;
    hipStream_t stream = 0; bool have_stream = false;                          // gaz_engine_score_outputs works here; score_replay on the engine's stream
    hipEvent_t ev_gather = 0, ev_scored = 0, ev_t0 = 0, ev_t1 = 0; bool have_events = false;
    float* d_pp = nullptr; float* d_pv = nullptr; float* d_tp = nullptr; float* d_tv = nullptr; long long pred_cap = 0, tgt_cap = 0;
    double* d_ce = nullptr; double* d_ent = nullptr; double* d_se = nullptr; uint8_t* d_flags = nullptr; long long row_cap = 0;
    double* d_part = nullptr; uint32_t* d_cnt = nullptr; long long blk_cap = 0;
    int last_n = 0, last_act = 0;                                             // the launch of the last score_outputs (the measurement hook repeats it)
    std::string err;

#define GAZ_SC_CK(expr) \
    do { hipError_t _e = (expr); if (_e != hipSuccess) { err = std::string(#expr) + ": " + hipGetErrorString(_e); return 1; } } while (0)

    ~ScoreState() {
        if (have_stream) hipStreamSynchronize(stream);
        void* all[] = {d_pp, d_pv, d_tp, d_tv, d_ce, d_ent, d_se, d_flags, d_part, d_cnt};
        for (void* p : all) if (p) hipFree(p);
        if (have_events) { hipEventDestroy(ev_gather); hipEventDestroy(ev_scored); hipEventDestroy(ev_t0); hipEventDestroy(ev_t1); }
        if (have_stream) hipStreamDestroy(stream);
    }
    int init() {
        GAZ_SC_CK(hipSetDevice(device));
        if (!have_stream) { GAZ_SC_CK(hipStreamCreate(&stream)); have_stream = true; }
        if (!have_events) {
            GAZ_SC_CK(hipEventCreateWithFlags(&ev_gather, hipEventDisableTiming)); GAZ_SC_CK(hipEventCreateWithFlags(&ev_scored, hipEventDisableTiming));
            GAZ_SC_CK(hipEventCreate(&ev_t0)); GAZ_SC_CK(hipEventCreate(&ev_t1));
            have_events = true;
        }
        return 0;
    }
    template <class T> int regrow(T** p, size_t n) {
        if (*p) { GAZ_SC_CK(hipFree(*p)); *p = nullptr; }
        if (hipMalloc((void**)p, n * sizeof(T)) != hipSuccess) { (void)hipGetLastError(); err = "score: allocation failure (" + std::to_string(n * sizeof(T)) + " bytes)"; return 1; }
        return 0;
    }
    // predictions of `pred` rows (with the spare elements the evaluators' output buffers have), targets of `tgt` rows, per-row results of M rows
    int ensure(long long pred, long long tgt, long long M) {
        if (pred > pred_cap) { pred_cap = 0; if (regrow(&d_pp, (size_t)pred * A + 64) || regrow(&d_pv, (size_t)pred + 64)) return 1; pred_cap = pred; }
        if (tgt > tgt_cap) { tgt_cap = 0; if (regrow(&d_tp, (size_t)tgt * A + 64) || regrow(&d_tv, (size_t)tgt + 64)) return 1; tgt_cap = tgt; }
        if (M > row_cap || !d_ce) {
            row_cap = 0;
            const long long want = M + M / 2 + 256;
            if (regrow(&d_ce, (size_t)want + 8) || regrow(&d_ent, (size_t)want + 8) || regrow(&d_se, (size_t)want + 8) || regrow(&d_flags, (size_t)want + 8)) return 1;
            row_cap = want;
        }
        const long long nb = (M + SCORE_BLOCK_ROWS - 1) / SCORE_BLOCK_ROWS;
        if (nb > blk_cap || !d_part) { blk_cap = 0; const long long want = nb + nb / 2 + 8; if (regrow(&d_part, (size_t)want * 3) || regrow(&d_cnt, (size_t)want * 4)) return 1; blk_cap = want; }
        return 0;
    }
    template <class G> void launch_rows_g(hipStream_t s, const float* P, const float* V, const float* Y, const float* Z, int n, long long base, int act) {
        GAZ_LAUNCH(k_score_rows<G>, (n + ScoreShape<G>::RPB - 1) / ScoreShape<G>::RPB, SCORE_THREADS, s, P, V, Y, Z, n, base, act, (int)G::A, d_ce, d_ent, d_se, d_flags);
    }
    // rows [base, base + n) of the per-row arrays; the caller has checked base + n <= row_cap
    void launch_rows(hipStream_t s, const float* P, const float* V, const float* Y, const float* Z, int n, long long base, int act) {
        if (n <= 0) return;
        if (game == GAZ_GAME_TICTACTOE) launch_rows_g<Game<GAME_TTT>>(s, P, V, Y, Z, n, base, act);
        else if (game == GAZ_GAME_CONNECT4) launch_rows_g<Game<GAME_C4>>(s, P, V, Y, Z, n, base, act);
        else launch_rows_g<Game<GAME_GMK>>(s, P, V, Y, Z, n, base, act);
    }
    static int act_of(int mode) { return mode == 1 ? SCORE_ACT_SOFTMAX : (mode == 3 ? SCORE_ACT_STABLEMAX : SCORE_ACT_NONE); }

    // the block sums of rows [0, M), ONE read-back and the host's left-to-right sum of the blocks; synchronises s
    int finish(hipStream_t s, long long M, int mode, gaz_score_totals* t, double* row_ce, double* row_ent, double* row_se, uint8_t* row_flags, bool timed, double* ms) {
        const uint32_t size = t->struct_size;
        memset(t, 0, sizeof(*t));
        t->struct_size = size; t->policy_mode = mode; t->rows = M;
        const long long nb = (M + SCORE_BLOCK_ROWS - 1) / SCORE_BLOCK_ROWS;
        std::vector<double> part((size_t)nb * 3);
        std::vector<uint32_t> cnt((size_t)nb * 4);
        if (M > 0) {
            GAZ_LAUNCH(k_score_blocks, (int)((nb + SCORE_THREADS / 64 - 1) / (SCORE_THREADS / 64)), SCORE_THREADS, s, (const double*)d_ce, (const double*)d_ent, (const double*)d_se,
                       (const uint8_t*)d_flags, M, d_part, d_cnt);
            GAZ_SC_CK(hipGetLastError());
            if (timed) GAZ_SC_CK(hipEventRecord(ev_t1, s));
            GAZ_SC_CK(hipMemcpyAsync(part.data(), d_part, part.size() * 8, hipMemcpyDeviceToHost, s));
            GAZ_SC_CK(hipMemcpyAsync(cnt.data(), d_cnt, cnt.size() * 4, hipMemcpyDeviceToHost, s));
            if (row_ce) GAZ_SC_CK(hipMemcpyAsync(row_ce, d_ce, (size_t)M * 8, hipMemcpyDeviceToHost, s));
            if (row_ent) GAZ_SC_CK(hipMemcpyAsync(row_ent, d_ent, (size_t)M * 8, hipMemcpyDeviceToHost, s));
            if (row_se) GAZ_SC_CK(hipMemcpyAsync(row_se, d_se, (size_t)M * 8, hipMemcpyDeviceToHost, s));
            if (row_flags) GAZ_SC_CK(hipMemcpyAsync(row_flags, d_flags, (size_t)M, hipMemcpyDeviceToHost, s));
        } else if (timed) GAZ_SC_CK(hipEventRecord(ev_t1, s));
        GAZ_SC_CK(hipStreamSynchronize(s));
        if (ms) {
            float f = 0.f;
            if (timed) GAZ_SC_CK(hipEventElapsedTime(&f, ev_t0, ev_t1));
            *ms = (double)f;
        }
        double ce = 0.0, ent = 0.0, se = 0.0;
        for (long long b = 0; b < nb; ++b) {
            ce = ce + part[(size_t)b * 3]; ent = ent + part[(size_t)b * 3 + 1]; se = se + part[(size_t)b * 3 + 2];
            t->top1 += cnt[(size_t)b * 4]; t->value_sign += cnt[(size_t)b * 4 + 1]; t->value_rows += cnt[(size_t)b * 4 + 2]; t->bad_rows += cnt[(size_t)b * 4 + 3];
        }
        t->ce_sum = ce; t->entropy_sum = ent; t->se_sum = se;
        return 0;
    }

    int outputs(const float* pp, const float* pv, const float* tp, const float* tv, long long n, int mode, gaz_score_totals* t, double* row_ce, double* row_ent, double* row_se,
                uint8_t* row_flags) {
        if (init() || ensure(n, n, n)) return 1;
        if (n > 0) {
            GAZ_SC_CK(hipMemcpyAsync(d_pp, pp, (size_t)n * A * 4, hipMemcpyHostToDevice, stream)); GAZ_SC_CK(hipMemcpyAsync(d_pv, pv, (size_t)n * 4, hipMemcpyHostToDevice, stream));
            GAZ_SC_CK(hipMemcpyAsync(d_tp, tp, (size_t)n * A * 4, hipMemcpyHostToDevice, stream)); GAZ_SC_CK(hipMemcpyAsync(d_tv, tv, (size_t)n * 4, hipMemcpyHostToDevice, stream));
            launch_rows(stream, d_pp, d_pv, d_tp, d_tv, (int)n, 0, act_of(mode));
        }
        last_n = (int)n; last_act = act_of(mode);
        return finish(stream, n, mode, t, row_ce, row_ent, row_se, row_flags, false, nullptr);
    }

    // measurement hook (tools/score_bench.py): the k_score_rows launch of the last outputs() call, `repeats` times between two HIP events
    int rows_timed(int repeats, double* ms_per_launch) {
        if (repeats < 1 || !ms_per_launch) { err = "score_rows_timed: repeats must be at least 1"; return 1; }
        if (last_n < 1 || init()) { if (last_n < 1) err = "score_rows_timed: call gaz_engine_score_outputs with n >= 1 first"; return 1; }
        launch_rows(stream, d_pp, d_pv, d_tp, d_tv, last_n, 0, last_act);
        GAZ_SC_CK(hipEventRecord(ev_t0, stream));
        for (int i = 0; i < repeats; ++i) launch_rows(stream, d_pp, d_pv, d_tp, d_tv, last_n, 0, last_act);
        GAZ_SC_CK(hipEventRecord(ev_t1, stream));
        GAZ_SC_CK(hipStreamSynchronize(stream));
        GAZ_SC_CK(hipGetLastError());
        float f = 0.f;
        GAZ_SC_CK(hipEventElapsedTime(&f, ev_t0, ev_t1));
        *ms_per_launch = (double)f / repeats;
        return 0;
    }
#undef GAZ_SC_CK
};

}  // namespace gaz
