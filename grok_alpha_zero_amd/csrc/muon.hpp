// muon.hpp — MUON in the fused optimizer step (gaz_muon_*): the reference's Net/Optimizers/muon.py, whose hot path is five
// Newton-Schulz iterations of three matrix products on every weight matrix, as a fixed number of launches over work tables, on f32 MFMA.
// Included by optim.hpp between its device code, which this file builds on (OptArgs, the chunk table, the chunk sums), and its host code.
//
// THE RULE is stated in include/gaz_engine.h ("MUON") and restated by tests/muon_model.py.  The operands of the iteration are bf16 VALUES HELD IN
// F32: products of two of them are exact in f32, and v_mfma_f32_32x32x2_f32 accumulates like a sequential fmaf chain over k ascending (DESIGN.md
// section 7, tools/probes/mfma_f32_order.hip), so the device, the one-lane build and the numpy model agree in every bit.
//
// A step in Muon mode:  [k_optim_dots, k_optim_gogo]  k_optim_apply_muon  k_muon_norm  ns_steps x (k_muon_gram, k_muon_poly, k_muon_update)  k_muon_finish
// k_optim_apply_muon  k_optim_apply's chunk table: an Adam tensor is finished here; a Muon tensor gets m (momentum arena), u (velocity arena) and
//                     the chunk's float64 sum of bf16(u)^2
// k_muon_norm         finishes n of its tensor, X = bf16(bf16(u) / (n + 1e-7f))
// k_muon_gram         GENERAL tensors (smaller dimension >= 5): a 64 x 64 tile of A = bf16(X X^T) per workgroup, four wavefronts of one 32 x 32
//                     MFMA tile each, operands staged through LDS 32 k at a time, the next stage's loads in flight during the MFMAs.
//                     THIN tensors (smaller dimension <= 4): the float64 partial sums of the at most ten Gram entries over 2048 columns
// k_muon_poly         general: a tile of A A, then B = bf16(bf16(b A) + bf16(c bf16(A A)))
// k_muon_update       general: a tile of B X, then X' = bf16(bf16(a X) + bf16(B X)) into the other X buffer.  thin: finishes the Gram sums, the
//                     4 x 4 polynomial in registers, the elementwise update of 2048 columns
// k_muon_finish       w = w - ((float)X * scale) * lr, then the decay
// A matrix whose rows outnumber its columns is iterated transposed by indexing: element (p, q) of X lies at off + p * sp + q * sq.
// No atomics, no cooperative launch, no grid-wide wait: a launch boundary separates a product from its readers.
#pragma once

namespace gaz {

constexpr int MU_TILE = 64, MU_K = 32, MU_LD = MU_K + 1, MU_THIN = 4, MU_PAIRS = 10;

struct MuonTensor { long long off, aoff; int P, Q, sp, sq, first_thin, n_thin; float scale; int thin; };      // P = 0: an Adam tensor
struct MuonTile { int tensor, ti, tj; };                                                                  // thin: ti = the chunk of columns
struct MuonArgs {
    const MuonTensor* mt; const MuonTile* pp; const MuonTile* pq; const MuonTile* thin;
    int n_pp, n_pq, n_thin, nesterov;
    const float* xs; float* xd;                     // this iteration's X and the next one's
    float* A; float* B; float* nrm;
    double* gpart;                                  // [thin chunks][10]
    double* npart;                                  // [chunks][4]: [0] = a chunk's sum of bf16(u)^2
    float beta, omb, ca, cb, cc, lr_adam, wd;
};

// round to nearest even on the bit pattern; NaN stays NaN
GAZ_HD float bf16r(float x) {
    uint32_t u;
    memcpy(&u, &x, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) u = (u | 0x00400000u) & 0xffff0000u;
    else u = (u + 0x7fffu + ((u >> 16) & 1u)) & 0xffff0000u;
    memcpy(&x, &u, 4);
    return x;
}

GAZ_DEV float muon_decayed(float w, float lr, float wd) {
    if (wd == 0.f) return w;
    const float a = lr * wd;
    const float b = a * w;
    return w - b;
}

#ifdef GAZ_HOST_EMU
#define GAZ_MU_FIRST 0
#define GAZ_MU_STEP 1
#else
#define GAZ_MU_FIRST ((int)threadIdx.x)
#define GAZ_MU_STEP OPT_THREADS
#endif

// N sums over the slots of a chunk in section 28's order: slot_fn(slot, acc) adds what the slot adds.  All threads of the workgroup call it, once
// per kernel; true in the thread that holds the sums.
template <int N, class F> GAZ_DEV bool muon_reduce(F slot_fn, double* out) {
#ifdef GAZ_HOST_EMU
    static thread_local double x[N][OPT_THREADS];
    static thread_local double y[OPT_THREADS];
    for (int s = 0; s < OPT_THREADS; ++s) {
        double acc[N];
        for (int k = 0; k < N; ++k) acc[k] = 0.0;
        slot_fn(s, acc);
        for (int k = 0; k < N; ++k) x[k][s] = acc[k];
    }
    for (int k = 0; k < N; ++k) {
        for (int d = 32; d >= 1; d >>= 1) {
            for (int s = 0; s < OPT_THREADS; ++s) y[s] = x[k][s] + x[k][s ^ d];
            for (int s = 0; s < OPT_THREADS; ++s) x[k][s] = y[s];
        }
        out[k] = ((x[k][0] + x[k][64]) + x[k][128]) + x[k][192];
    }
    return true;
#else
    __shared__ double sw[OPT_THREADS / 64][N];
    double acc[N];
#pragma unroll
    for (int k = 0; k < N; ++k) acc[k] = 0.0;
    slot_fn((int)threadIdx.x, acc);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
        for (int k = 0; k < N; ++k) acc[k] = acc[k] + shfl_xor(acc[k], d);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) sw[threadIdx.x >> 6][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x != 0) return false;
#pragma unroll
    for (int k = 0; k < N; ++k) out[k] = ((sw[0][k] + sw[1][k]) + sw[2][k]) + sw[3][k];
    return true;
#endif
}

// the elements a slot adds of a chunk of len: its groups of four in ascending order, slot 0 also the elements behind the last whole group
template <class F> GAZ_DEV void muon_slot_elements(int len, int slot, F fn) {
    const int G = len >> 2;
#pragma unroll
    for (int i = 0; i < OPT_GPS; ++i) {
        const int j = slot + i * OPT_THREADS;
        if (j < G) { fn(j * 4); fn(j * 4 + 1); fn(j * 4 + 2); fn(j * 4 + 3); }
    }
    if (slot == 0)
        for (int k = G * 4; k < len; ++k) fn(k);
}

// ------------------------------------------------------------------------------------------------ the momentum stage
// one element of a tensor in Muon mode through the stages 1 .. 3 (the decay of an Adam tensor included; a Muon tensor's w moves in k_muon_finish)
GAZ_DEV void muon_element(const OptArgs& a, const MuonArgs& mu, bool muon, float proj, float s, float& w, float& g, float& m, float& v, float& e) {
    const float g2 = opt_g2(a, proj, s, w, g, e);
    if (muon) {
        const float m1 = mu.beta * m;
        const float m2 = g2 * mu.omb;
        m = m1 + m2;
        float u = m;
        if (mu.nesterov) {
            const float mb = m * mu.beta;
            u = g2 + mb;
        }
        v = u;
    } else {
        const float u = opt_adam(a, g2, m, v);
        const float ul = u * mu.lr_adam;
        const float w2 = w - ul;
        w = muon_decayed(w2, mu.lr_adam, mu.wd);
    }
    if (a.zero) g = 0.f;
}

GAZ_DEV void muon_apply_slot(const OptArgs& a, const MuonArgs& mu, bool muon, long long at, int len, int slot, float proj, float s) {
    const int G = len >> 2;
    float zero_e = 0.f;
#pragma unroll
    for (int i = 0; i < OPT_GPS; ++i) {
        const int j = slot + i * OPT_THREADS;
        if (j < G) {
            OptF4* pw = (OptF4*)(a.w + at) + j; OptF4* pg = (OptF4*)(a.g + at) + j; OptF4* pm = (OptF4*)(a.m + at) + j; OptF4* pv = (OptF4*)(a.v + at) + j;
            OptF4 W = *pw, Gv = *pg, M = *pm, V = *pv, E = {0.f, 0.f, 0.f, 0.f};
            if (a.grok) E = *((OptF4*)(a.e + at) + j);
            muon_element(a, mu, muon, proj, s, W.x, Gv.x, M.x, V.x, E.x); muon_element(a, mu, muon, proj, s, W.y, Gv.y, M.y, V.y, E.y);
            muon_element(a, mu, muon, proj, s, W.z, Gv.z, M.z, V.z, E.z); muon_element(a, mu, muon, proj, s, W.w, Gv.w, M.w, V.w, E.w);
            if (!muon) *pw = W;
            *pm = M; *pv = V;
            if (a.zero) *pg = Gv;
            if (a.grok) *((OptF4*)(a.e + at) + j) = E;
        }
    }
    if (slot == 0)
        for (int k = G * 4; k < len; ++k)
            muon_element(a, mu, muon, proj, s, a.w[at + k], a.g[at + k], a.m[at + k], a.v[at + k], a.grok ? a.e[at + k] : zero_e);
}

GAZ_OPT_BOUNDS GAZ_KERNEL_WIDE k_optim_apply_muon(OptArgs a, MuonArgs mu) {
    const OptPlace p = opt_place(a);
    const bool muon = mu.mt[p.tensor].P > 0;
    float proj = 0.f, s = 1.f;
    if (a.ortho) {
        double sums[4];
        opt_tensor_sums<0, 4>(a.part, p.first_chunk, p.n_chunks, sums);
        proj = opt_proj(sums); s = opt_scale(sums);
#ifdef GAZ_HOST_EMU
        if (p.index == 0) a.norms[(long long)p.tensor * 4 + 3] = sums[3];
#else
        if (p.index == 0 && threadIdx.x == 0) a.norms[(long long)p.tensor * 4 + 3] = sums[3];
#endif
    }
#ifdef GAZ_HOST_EMU
    for (int slot = 0; slot < OPT_THREADS; ++slot) muon_apply_slot(a, mu, muon, p.at, p.len, slot, proj, s);
#else
    muon_apply_slot(a, mu, muon, p.at, p.len, (int)threadIdx.x, proj, s);
#endif
    if (!muon) return;                                                            // (uniform in the workgroup)
    // the chunk's sum of X0^2: a slot reads back the u it stored itself
    const float* u = a.v + p.at;
    double out[1];
    const bool holder = muon_reduce<1>([&](int slot, double* acc) {
        muon_slot_elements(p.len, slot, [&](int k) { const float x = bf16r(u[k]); acc[0] = acc[0] + (double)x * (double)x; });
    }, out);
    if (holder) mu.npart[(long long)block_id() * 4] = out[0];
}

GAZ_OPT_BOUNDS GAZ_KERNEL_WIDE k_muon_norm(OptArgs a, MuonArgs mu) {
    const OptPlace p = opt_place(a);
    if (mu.mt[p.tensor].P == 0) return;
    double sums[4];
    opt_tensor_sums<0, 1>(mu.npart, p.first_chunk, p.n_chunks, sums);
    const float n = __builtin_sqrtf((float)sums[0]);
    const float d = n + 1e-7f;
    for (int k = GAZ_MU_FIRST; k < p.len; k += GAZ_MU_STEP) {
        const float x0 = bf16r(a.v[p.at + k]);
        const float q = x0 / d;
        mu.xd[p.at + k] = bf16r(q);
    }
    if (p.index == 0 && GAZ_MU_FIRST == 0) mu.nrm[p.tensor] = n;
}

GAZ_OPT_BOUNDS GAZ_KERNEL_WIDE k_muon_finish(OptArgs a, MuonArgs mu) {
    const OptPlace p = opt_place(a);
    const MuonTensor t = mu.mt[p.tensor];
    if (t.P == 0) return;
    for (int k = GAZ_MU_FIRST; k < p.len; k += GAZ_MU_STEP) {
        const float xs = mu.xs[p.at + k] * t.scale;
        const float ul = xs * a.lr;
        const float w2 = a.w[p.at + k] - ul;
        a.w[p.at + k] = muon_decayed(w2, a.lr, mu.wd);
    }
}

// ------------------------------------------------------------------------------------------------ the general path: tiles on f32 MFMA
struct MuonOp { const float* p; long long si, sk; int n; };      // element (idx, k) of an operand at p[idx * si + k * sk], idx < n

#ifndef GAZ_HOST_EMU
typedef float mu_f32x16 __attribute__((ext_vector_type(16)));
// 64 idx x 32 k of an operand, eight elements a thread: the threads run along whichever index is contiguous in memory
GAZ_DEV void muon_stage_load(const MuonOp& op, int base, int k0, int K, float* r) {
    const int t = (int)threadIdx.x;
    const bool kfast = op.sk == 1;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int idx = kfast ? (t >> 5) + 8 * e : (t & 63);
        const int kk = kfast ? (t & 31) : (t >> 6) + 4 * e;
        const int gi = base + idx, gk = k0 + kk;
        r[e] = (gi < op.n && gk < K) ? op.p[(long long)gi * op.si + (long long)gk * op.sk] : 0.f;
    }
}
GAZ_DEV void muon_stage_store(const MuonOp& op, float* lds, const float* r) {
    const int t = (int)threadIdx.x;
    const bool kfast = op.sk == 1;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int idx = kfast ? (t >> 5) + 8 * e : (t & 63);
        const int kk = kfast ? (t & 31) : (t >> 6) + 4 * e;
        lds[idx * MU_LD + kk] = r[e];
    }
}
#endif

// C[i][j] = the f32 chain over k = 0 .. K - 1 of A[i][k] * B[j][k] for the 64 x 64 tile at (i0, j0), partial at the edges; epi(i, j, c) per element
template <class E> GAZ_DEV void muon_tile(const MuonOp& Aop, const MuonOp& Bop, int K, int i0, int j0, E epi) {
#ifdef GAZ_HOST_EMU
    for (int i = i0; i < i0 + MU_TILE && i < Aop.n; ++i)
        for (int j = j0; j < j0 + MU_TILE && j < Bop.n; ++j) {
            float acc = 0.f;
            for (int k = 0; k < K; ++k) {
                const float pr = Aop.p[(long long)i * Aop.si + (long long)k * Aop.sk] * Bop.p[(long long)j * Bop.si + (long long)k * Bop.sk];     // exact
                acc = acc + pr;
            }
            epi(i, j, acc);
        }
#else
    __shared__ float As[MU_TILE * MU_LD];
    __shared__ float Bs[MU_TILE * MU_LD];
    const int t = (int)threadIdx.x, lane = t & 63, wv = t >> 6, wi = wv >> 1, wj = wv & 1, l31 = lane & 31, lhi = lane >> 5;
    float ra[8], rb[8];
    mu_f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    muon_stage_load(Aop, i0, 0, K, ra); muon_stage_load(Bop, j0, 0, K, rb);
    const float* pa = As + (wi * 32 + l31) * MU_LD + lhi;
    const float* pb = Bs + (wj * 32 + l31) * MU_LD + lhi;
    for (int k0 = 0; k0 < K; k0 += MU_K) {
        muon_stage_store(Aop, As, ra); muon_stage_store(Bop, Bs, rb);
        __syncthreads();
        if (k0 + MU_K < K) { muon_stage_load(Aop, i0, k0 + MU_K, K, ra); muon_stage_load(Bop, j0, k0 + MU_K, K, rb); }
#pragma unroll
        for (int kk = 0; kk < MU_K; kk += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[kk], pb[kk], acc, 0, 0, 0);
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int i = i0 + wi * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi, j = j0 + wj * 32 + l31;
        if (i < Aop.n && j < Bop.n) epi(i, j, acc[r]);
    }
#endif
}

GAZ_DEV MuonOp muon_x_rows(const MuonArgs& mu, const MuonTensor& t) { return MuonOp{mu.xs + t.off, t.sp, t.sq, t.P}; }     // idx = p, k = q
GAZ_DEV MuonOp muon_x_cols(const MuonArgs& mu, const MuonTensor& t) { return MuonOp{mu.xs + t.off, t.sq, t.sp, t.Q}; }     // idx = q, k = p

// ------------------------------------------------------------------------------------------------ the thin path
// column q of a thin X: x[r] = X[r][q], 0 for r >= P
GAZ_DEV void muon_thin_column(const float* x0, const MuonTensor& t, int q, float* x) {
#pragma unroll
    for (int r = 0; r < MU_THIN; ++r) x[r] = r < t.P ? x0[(long long)r * t.sp + (long long)q * t.sq] : 0.f;
}

GAZ_DEV void muon_thin_gram(const MuonArgs& mu, int entry) {
    const MuonTile e = mu.thin[entry];
    const MuonTensor t = mu.mt[e.tensor];
    const int q0 = e.ti * OPT_CHUNK, len = t.Q - q0 < OPT_CHUNK ? t.Q - q0 : OPT_CHUNK;
    const float* x0 = mu.xs + t.off;
    double out[MU_PAIRS];
    const bool holder = muon_reduce<MU_PAIRS>([&](int slot, double* acc) {
        muon_slot_elements(len, slot, [&](int k) {
            float x[MU_THIN];
            muon_thin_column(x0, t, q0 + k, x);
            int n = 0;
#pragma unroll
            for (int i = 0; i < MU_THIN; ++i) {
#pragma unroll
                for (int j = i; j < MU_THIN; ++j, ++n) acc[n] = acc[n] + (double)x[i] * (double)x[j];
            }
        });
    }, out);
    if (holder) {
        double* dst = mu.gpart + (long long)entry * MU_PAIRS;
#pragma unroll
        for (int n = 0; n < MU_PAIRS; ++n) dst[n] = out[n];
    }
}

GAZ_DEV void muon_thin_update(const MuonArgs& mu, int entry) {
    const MuonTile e = mu.thin[entry];
    const MuonTensor t = mu.mt[e.tensor];
    const int q0 = e.ti * OPT_CHUNK, len = t.Q - q0 < OPT_CHUNK ? t.Q - q0 : OPT_CHUNK;
    // the Gram entries: the chunks' sums in ascending order from +0.0, to f32, to bf16
    double g[MU_PAIRS];
#pragma unroll
    for (int n = 0; n < MU_PAIRS; ++n) g[n] = 0.0;
    for (int c = 0; c < t.n_thin; ++c) {
        const double* src = mu.gpart + (long long)(t.first_thin + c) * MU_PAIRS;
#pragma unroll
        for (int n = 0; n < MU_PAIRS; ++n) g[n] = g[n] + src[n];
    }
    float A[MU_THIN][MU_THIN], B[MU_THIN][MU_THIN];
    {
        int n = 0;
#pragma unroll
        for (int i = 0; i < MU_THIN; ++i) {
#pragma unroll
            for (int j = i; j < MU_THIN; ++j, ++n) { A[i][j] = bf16r((float)g[n]); A[j][i] = A[i][j]; }
        }
    }
#pragma unroll
    for (int i = 0; i < MU_THIN; ++i) {
#pragma unroll
        for (int j = 0; j < MU_THIN; ++j) {
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < MU_THIN; ++k)
                if (k < t.P) { const float pr = A[i][k] * A[k][j]; acc = acc + pr; }
            const float aa = bf16r(acc);
            const float t1 = bf16r(mu.cb * A[i][j]);
            const float t2 = bf16r(mu.cc * aa);
            B[i][j] = bf16r(t1 + t2);
        }
    }
    if (e.ti == 0 && GAZ_MU_FIRST == 0) {
#pragma unroll
        for (int i = 0; i < MU_THIN; ++i) {
#pragma unroll
            for (int j = 0; j < MU_THIN; ++j)
                if (i < t.P && j < t.P) { mu.A[t.aoff + i * t.P + j] = A[i][j]; mu.B[t.aoff + i * t.P + j] = B[i][j]; }
        }
    }
    const float* x0 = mu.xs + t.off;
    float* xd = mu.xd + t.off;
    for (int k = GAZ_MU_FIRST; k < len; k += GAZ_MU_STEP) {
        float x[MU_THIN];
        muon_thin_column(x0, t, q0 + k, x);
#pragma unroll
        for (int i = 0; i < MU_THIN; ++i) {
            if (i < t.P) {
                float acc = 0.f;
#pragma unroll
                for (int kk = 0; kk < MU_THIN; ++kk)
                    if (kk < t.P) { const float pr = B[i][kk] * x[kk]; acc = acc + pr; }
                const float t1 = bf16r(mu.ca * x[i]);
                const float t2 = bf16r(acc);
                xd[(long long)i * t.sp + (long long)(q0 + k) * t.sq] = bf16r(t1 + t2);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ the three kernels of an iteration
GAZ_OPT_BOUNDS GAZ_KERNEL_WIDE k_muon_gram(MuonArgs mu) {
    const int b = block_id();
    if (b >= mu.n_pp) { muon_thin_gram(mu, b - mu.n_pp); return; }
    const MuonTile e = mu.pp[b];
    const MuonTensor t = mu.mt[e.tensor];
    float* A = mu.A + t.aoff;
    const MuonOp X = muon_x_rows(mu, t);
    muon_tile(X, X, t.Q, e.ti * MU_TILE, e.tj * MU_TILE, [&](int i, int j, float c) { A[(long long)i * t.P + j] = bf16r(c); });
}

GAZ_OPT_BOUNDS GAZ_KERNEL_WIDE k_muon_poly(MuonArgs mu) {
    const MuonTile e = mu.pp[block_id()];
    const MuonTensor t = mu.mt[e.tensor];
    const float* A = mu.A + t.aoff;
    float* B = mu.B + t.aoff;
    const MuonOp rows = MuonOp{A, t.P, 1, t.P}, cols = MuonOp{A, 1, t.P, t.P};       // (A A)[i][j] = chain of A[i][k] * A[k][j]
    muon_tile(rows, cols, t.P, e.ti * MU_TILE, e.tj * MU_TILE, [&](int i, int j, float c) {
        const float aa = bf16r(c);
        const float t1 = bf16r(mu.cb * A[(long long)i * t.P + j]);
        const float t2 = bf16r(mu.cc * aa);
        B[(long long)i * t.P + j] = bf16r(t1 + t2);
    });
}

GAZ_OPT_BOUNDS GAZ_KERNEL_WIDE k_muon_update(MuonArgs mu) {
    const int b = block_id();
    if (b >= mu.n_pq) { muon_thin_update(mu, b - mu.n_pq); return; }
    const MuonTile e = mu.pq[b];
    const MuonTensor t = mu.mt[e.tensor];
    const float* x0 = mu.xs + t.off;
    float* xd = mu.xd + t.off;
    const MuonOp rows = MuonOp{mu.B + t.aoff, t.P, 1, t.P};                           // (B X)[i][q] = chain of B[i][k] * X[k][q]
    muon_tile(rows, muon_x_cols(mu, t), t.P, e.ti * MU_TILE, e.tj * MU_TILE, [&](int i, int q, float c) {
        const long long at = (long long)i * t.sp + (long long)q * t.sq;
        const float t1 = bf16r(mu.ca * x0[at]);
        const float t2 = bf16r(c);
        xd[at] = bf16r(t1 + t2);
    });
}

}  // namespace gaz
