// det_probe.hpp — gaz_engine_probe_det: the device's bit-exact math, one function at a time, on inputs the caller chooses.
//
// The parity of the search with the CPU checker rests on det.hpp computing what oracle/gaz_det.h computes, bit for bit.  Every other
// test sees that arithmetic through a float32 cast, an argmax or a cdf step; this probe hands the float64 / uint32 results back as
// raw bits.  The kernels call the functions the search calls and restate nothing; they are compiled in engine.hip, with the flags and
// the kernel attributes (GAZ_KERNEL / GAZ_KERNEL_TEAMS) of the tree kernels.
//
// Everything travels as 64-bit words: item i reads in[i * in_words ...] and writes out[i * out_words ...]; a float64 is its bit
// pattern, a float32 / uint32 sits in the low half of its word.
//
// Element ops, one LANE per item (in_words / out_words are exact):
//   DP_PHILOX        c0 c1 c2 c3 k0 k1                                   -> 4 words
//   DP_DRAW          key0 key1 slot game_seq event tree purpose lane attempt -> 4 words
//   DP_UNIT          a b                                                 -> k52, u_open, u_half
//   DP_DLOG / DP_DEXP / DP_DSQRT   x                                     -> f(x)
//   DP_DPOW / DP_DDIV              x y                                   -> dpow(x, y) / the plain float64 x / y
//   DP_PUCT_C        pv(f64) c_init c_base                               -> puct_c_of
//   DP_PUCT_FACTORS  parent_visits(u64) use_table                        -> s, c, 1 if the engine's table served the item
//                    (the engine's own c_init / c_base; use_table = 0 passes table = nullptr)
//   DP_SAMPLE        key0 key1 slot game_seq event tree purpose lane alpha pick_n
//                    -> uniform, pick(pick_n), gumbel(lane), normal(lane), its draws, gamma(lane, alpha), its draws, its accepting test
// Team ops, one TEAM per item, word 0 = n (the arrays behind it hold max(n, 8) entries: the n < 8 paths of the functions read eight
// elements, and what the caller puts behind n travels with them):
//   DP_SUM_F32 / DP_SUM_F64   n, a[]               -> np_pairwise_sum, on S.pri / S.spri / S.gam (n <= APAD) or on an LDS array of the
//                                                     probe's own (APAD < n <= 256, which no Scratch array holds)
//   DP_PUCT_SCORES   n, s, c, {N W P}[]            -> best_puct_slot's slot, then the float64 score of every slot
//   DP_SOFTMAX       n, x[]                        -> softmax_inplace's S.gam[0..n)
//   DP_PI            n, stable, c_visit, c_scale, {N W logit RAW}[]
//                    -> N_b, sum of visits, g_det_select's slot, then compute_pi's S.pri (float32 bits) or, stable, S.gam (float64 bits)
//   The node of the last three is built with NodeLayout in S.node (RAW in S.raw), where the descent stages a record.
// A team is what the engine's tree kernels make it: four 16-lane teams per wavefront for Connect4 / TicTacToe, the wavefront for Gomoku;
// op | DP_WHOLE_WAVE runs a small board's item on a whole wavefront, as its one-game-per-wavefront kernels do.
#pragma once
#include "gumbel_core.hpp"

namespace gaz {

enum : int32_t {
    DP_PHILOX = 0, DP_DRAW = 1, DP_UNIT = 2, DP_DLOG = 3, DP_DEXP = 4, DP_DPOW = 5, DP_DSQRT = 6, DP_DDIV = 7, DP_PUCT_C = 8,
    DP_PUCT_FACTORS = 9, DP_SAMPLE = 10,
    DP_SUM_F32 = 16, DP_SUM_F64 = 17, DP_PUCT_SCORES = 18, DP_SOFTMAX = 19, DP_PI = 20,
    DP_WHOLE_WAVE = 0x100
};
constexpr int DP_SUM_MAX = 256;        // np_pairwise_sum's own limit

// what an op reads and writes per item.  Element op: exactly in / out words.  Team op: in_hdr + in_per * max(n, 8) words at least,
// out_hdr + out_per * n
struct DetProbeOp { bool team; int in, out, in_per, out_per; };
inline bool det_probe_op(int code, DetProbeOp* d) {
    switch (code) {
        case DP_PHILOX: *d = {false, 6, 4, 0, 0}; return true;
        case DP_DRAW: *d = {false, 9, 4, 0, 0}; return true;
        case DP_UNIT: *d = {false, 2, 3, 0, 0}; return true;
        case DP_DLOG: case DP_DEXP: case DP_DSQRT: *d = {false, 1, 1, 0, 0}; return true;
        case DP_DPOW: case DP_DDIV: *d = {false, 2, 1, 0, 0}; return true;
        case DP_PUCT_C: *d = {false, 3, 1, 0, 0}; return true;
        case DP_PUCT_FACTORS: *d = {false, 2, 3, 0, 0}; return true;
        case DP_SAMPLE: *d = {false, 10, 8, 0, 0}; return true;
        case DP_SUM_F32: case DP_SUM_F64: *d = {true, 1, 1, 1, 0}; return true;
        case DP_PUCT_SCORES: *d = {true, 3, 1, 3, 1}; return true;
        case DP_SOFTMAX: *d = {true, 1, 0, 1, 1}; return true;
        case DP_PI: *d = {true, 4, 3, 4, 1}; return true;
    }
    return false;
}

GAZ_DEV float dp_f32(uint64_t w) { const uint32_t u = (uint32_t)w; float f; memcpy(&f, &u, 4); return f; }
GAZ_DEV uint64_t dp_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return (uint64_t)u; }
GAZ_DEV det::Event dp_event(const uint64_t* a) {
    det::Event e;
    e.key0 = (uint32_t)a[0]; e.key1 = (uint32_t)a[1]; e.slot = (uint32_t)a[2]; e.game_seq = (uint32_t)a[3];
    e.event = (uint32_t)a[4]; e.tree = (uint32_t)a[5]; e.purpose = (uint32_t)a[6];
    return e;
}

template <class G> GAZ_KERNEL k_probe_det(DevParams<G> E, int op, int n_items, const uint64_t* in, int in_words, uint64_t* out, int out_words) {
    const int item = block_id() * WAVE + lane_id();
    if (item >= n_items) return;
    const uint64_t* a = in + (size_t)item * in_words;
    uint64_t* o = out + (size_t)item * out_words;
    switch (op) {
        case DP_PHILOX: {
            const det::U4 r = det::philox((uint32_t)a[0], (uint32_t)a[1], (uint32_t)a[2], (uint32_t)a[3], (uint32_t)a[4], (uint32_t)a[5]);
            o[0] = r.x; o[1] = r.y; o[2] = r.z; o[3] = r.w;
        } break;
        case DP_DRAW: {
            const det::U4 r = det::draw(dp_event(a), (uint32_t)a[7], (uint32_t)a[8]);
            o[0] = r.x; o[1] = r.y; o[2] = r.z; o[3] = r.w;
        } break;
        case DP_UNIT:
            o[0] = det::k52((uint32_t)a[0], (uint32_t)a[1]);
            o[1] = det::d2bits(det::u_open((uint32_t)a[0], (uint32_t)a[1]));
            o[2] = det::d2bits(det::u_half((uint32_t)a[0], (uint32_t)a[1]));
            break;
        case DP_DLOG: o[0] = det::d2bits(det::dlog(det::bits2d(a[0]))); break;
        case DP_DEXP: o[0] = det::d2bits(det::dexp(det::bits2d(a[0]))); break;
        case DP_DSQRT: o[0] = det::d2bits(dsqrt(det::bits2d(a[0]))); break;
        case DP_DPOW: o[0] = det::d2bits(det::dpow(det::bits2d(a[0]), det::bits2d(a[1]))); break;
        case DP_DDIV: o[0] = det::d2bits(det::bits2d(a[0]) / det::bits2d(a[1])); break;
        case DP_PUCT_C: o[0] = det::d2bits(puct_c_of(det::bits2d(a[0]), det::bits2d(a[1]), det::bits2d(a[2]))); break;
        case DP_PUCT_FACTORS: {
            const double* table = a[1] ? E.puct_table : nullptr;
            double s, c;
            puct_factors(a[0], E.c_init, E.c_base, table, s, c);
            o[0] = det::d2bits(s); o[1] = det::d2bits(c); o[2] = (table && a[0] < (uint64_t)PUCT_TABLE_N) ? 1u : 0u;
        } break;
        case DP_SAMPLE: {
            const det::Event e = dp_event(a);
            const uint32_t lane = (uint32_t)a[7];
            o[0] = det::d2bits(det::uniform(e));
            o[1] = det::pick(e, (uint32_t)a[9]);
            o[2] = det::d2bits(det::gumbel(e, lane));
            uint32_t attempt = 0;
            o[3] = det::d2bits(det::normal(e, lane, attempt));
            o[4] = attempt;
            uint32_t info[2] = {0u, 0u};
            o[5] = det::d2bits(det::gamma(e, lane, det::bits2d(a[8]), info));
            o[6] = info[0]; o[7] = info[1];
        } break;
        default: break;
    }
}

// a synthetic node record in S.node / S.raw, as g_stage_node and puct_select leave one: slot i from words rec[per * i ...] = N, W, P or
// logit (, RAW)
template <class G> GAZ_DEV NodeRef<G> dp_stage_node(Scratch<G>& S, const uint64_t* rec, int per, int n, int n_fill) {
    NodeRef<G> nd{reinterpret_cast<uint8_t*>(S.node)};
    for (int i = tlane<G>(); i < n_fill; i += G::TEAM) {
        nd.N()[i] = (uint32_t)rec[per * i]; nd.W()[i] = dp_f32(rec[per * i + 1]); nd.P()[i] = dp_f32(rec[per * i + 2]);
        nd.child()[i] = CHILD_NONE; nd.act()[i] = (uint8_t)i;
        if (per > 3) S.raw[i] = dp_f32(rec[per * i + 3]);
    }
    if (tlane<G>() == 0) {
        NodeHdr h; memset(&h, 0, sizeof(h));
        h.parent = -1; h.player = 1; h.n_actions = (uint8_t)n;
        *nd.hdr() = h;
    }
    wave_sync();
    return nd;
}

template <class G> GAZ_DEV void probe_det_team(const DevParams<G>& E, int op, int n_items, const uint64_t* in, int in_words, uint64_t* out,
                                               int out_words) {
    constexpr int PER = WAVE / G::TEAM;
    GAZ_SHARED Scratch<G> Ss[PER];
    GAZ_SHARED double wide[PER][DP_SUM_MAX];
    const int t = team_in_wave<G>();
    const int item = block_id() * PER + t;
    if (item >= n_items) return;
    Scratch<G>& S = Ss[t];
    const uint64_t* a = in + (size_t)item * in_words;
    uint64_t* o = out + (size_t)item * out_words;
    const int n = (int)a[0];
    const int n_fill = n < 8 ? 8 : n;
    const int l = tlane<G>();
    const bool writer = l == item % G::TEAM;          // every lane of the team holds a reduction's result: the items take turns over the lanes
    if (op == DP_SUM_F32) {
        float* arr = n > G::APAD ? reinterpret_cast<float*>(wide[t]) : ((item & 1) ? S.spri : S.pri);
        for (int i = l; i < n_fill; i += G::TEAM) arr[i] = dp_f32(a[1 + i]);
        wave_sync();
        const float r = n > G::APAD ? det::np_pairwise_sum<float, DP_SUM_MAX>(arr, n) : det::np_pairwise_sum<float, G::APAD>(arr, n);   // the search's instantiation where it applies
        if (writer) o[0] = dp_bits(r);
    } else if (op == DP_SUM_F64) {
        double* arr = n > G::APAD ? wide[t] : S.gam;
        for (int i = l; i < n_fill; i += G::TEAM) arr[i] = det::bits2d(a[1 + i]);
        wave_sync();
        const double r = n > G::APAD ? det::np_pairwise_sum<double, DP_SUM_MAX>(arr, n) : det::np_pairwise_sum<double, G::APAD>(arr, n);
        if (writer) o[0] = det::d2bits(r);
    } else if (op == DP_PUCT_SCORES) {
        const NodeRef<G> nd = dp_stage_node<G>(S, a + 3, 3, n, n_fill);
        const int slot = best_puct_slot<G>(nd, n, det::bits2d(a[1]), det::bits2d(a[2]), false, nullptr, S.gam);
        wave_sync();
        for (int i = l; i < n; i += G::TEAM) o[1 + i] = det::d2bits(S.gam[i]);
        if (writer) o[0] = (uint64_t)(uint32_t)slot;
    } else if (op == DP_SOFTMAX) {
        for (int i = l; i < n_fill; i += G::TEAM) S.gam[i] = det::bits2d(a[1 + i]);
        wave_sync();
        softmax_inplace<G>(S, n);
        for (int i = l; i < n; i += G::TEAM) o[i] = det::d2bits(S.gam[i]);
    } else if (op == DP_PI) {
        const bool stable = a[1] != 0;
        DevParams<G> E2 = E;
        E2.c_visit = det::bits2d(a[2]); E2.c_scale = det::bits2d(a[3]); E2.g_stablemax = stable ? 1 : 0;
        const NodeRef<G> nd = dp_stage_node<G>(S, a + 4, 4, n, n_fill);
        uint32_t nb = 0; uint64_t sumv = 0;
        compute_pi<G>(E2, nd, S.raw, n, S, nb, sumv, stable);
        wave_sync();
        for (int i = l; i < n; i += G::TEAM) o[3 + i] = stable ? det::d2bits(S.gam[i]) : dp_bits(S.pri[i]);
        wave_sync();
        const int slot = g_det_select<G>(E2, nd, S.raw, n, S);
        if (writer) { o[0] = nb; o[1] = sumv; o[2] = (uint64_t)(uint32_t)slot; }
    }
}
template <class G> GAZ_KERNEL k_probe_det_wave(DevParams<G> E, int op, int n_items, const uint64_t* in, int in_words, uint64_t* out, int out_words) {
    probe_det_team<G>(E, op, n_items, in, in_words, out, out_words);
}
template <class G> GAZ_KERNEL_TEAMS k_probe_det_teams(DevParams<G> E, int op, int n_items, const uint64_t* in, int in_words, uint64_t* out, int out_words) {
    probe_det_team<G>(E, op, n_items, in, in_words, out, out_words);
}

}  // namespace gaz
