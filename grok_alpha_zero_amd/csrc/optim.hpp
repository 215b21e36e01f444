// optim.hpp — THE OPTIMIZER STEP on the device (gaz_optim_*): the reference's chain Orthograd(Grokfast_EMA(Adam | Nadam))
// (Train.py:25-31, Net/Optimizers/{ortho_grad,grok_fast,adam,nadam}.py) as one multi-tensor step over flat arenas.  Keras runs the chain tensor
// by tensor, some fifteen small launches per variable; here a step is ONE launch, or three with Orthograd, whatever the number of tensors.
//
// THE RULE is stated in include/gaz_engine.h ("OPTIMIZER") and restated by tests/optim_model.py: f32 elementwise operations that are rounded one by
// one (the build passes -ffp-contract=off), correctly rounded division and square root, and four float64 dot products per tensor whose summation
// order depends on nothing but the tensor's size — so the device, the one-lane build and the numpy model agree in every bit.
//
// THE CHUNK TABLE, built once at create, names (tensor, chunk within it) for every workgroup: a chunk is 2048 elements, 256 threads, two 16-byte
// groups per thread and arena (the tensors start on 16-byte boundaries), and scalar code for the tensor's last one to three elements.
// k_optim_dots   a chunk's w.g, w.w, g.g: thread = slot, a butterfly of __shfl_xor within the wavefront, the four wavefronts through LDS
// k_optim_gogo   finishes the three sums of its tensor (every wavefront adds the tensor's chunk sums in ascending order: v_readlane of a
//                wave-uniform index), then the chunk's go.go
// k_optim_apply  finishes go.go likewise, then decay, Orthograd's rescale, Grokfast, Adam / Nadam and the zeroing of the grads
// No atomics, no cooperative launch, no grid-wide wait: a launch boundary separates a sum from its readers.
#pragma once
#include <math.h>
#include <string>
#include <vector>
#include "det.hpp"
#include "rt.hpp"

namespace gaz {

constexpr int OPT_THREADS = 256, OPT_CHUNK = 2048, OPT_GROUPS = OPT_CHUNK / 4, OPT_GPS = OPT_GROUPS / OPT_THREADS;
#ifdef GAZ_HOST_EMU
#define GAZ_OPT_BOUNDS
#else
#define GAZ_OPT_BOUNDS __launch_bounds__(256)
#endif

struct alignas(16) OptF4 { float x, y, z, w; };
struct OptTensor { long long off, n; int first_chunk, n_chunks; };
struct OptChunk { int tensor, index; };
struct OptArgs {
    float* w; float* g; float* m; float* v; float* e;
    const OptTensor* tens; const OptChunk* chunks;
    double* part;                                   // [chunks][4]: w.g, w.w, g.g, go.go of a chunk
    double* norms;                                  // [tensors][4]: the same of a tensor
    float lr, wd, b1, b2, omb1, omb2, eps, alpha, oma, lamb, c1, c2;
    int kind, ortho, grok, zero;
};

GAZ_DEV float opt_decayed(float w, float wd, float lr) {
    if (wd == 0.f) return w;
    const float a = w * wd;
    const float b = a * lr;
    return w - b;
}

// PASS 1: acc[0 .. 2] += w.g, w.w, g.g;  PASS 2: acc[0] += go.go.  The products of two f32 values are exact in f64.
template <int PASS> GAZ_DEV void opt_term(float w0, float g, const OptArgs& a, float proj, double* acc) {
    const float w = opt_decayed(w0, a.wd, a.lr);
    if (PASS == 1) {
        acc[0] = acc[0] + (double)w * (double)g; acc[1] = acc[1] + (double)w * (double)w; acc[2] = acc[2] + (double)g * (double)g;
    } else {
        const float p = proj * w;
        const float go = g - p;
        acc[0] = acc[0] + (double)go * (double)go;
    }
}

// what slot `slot` adds of a chunk of len elements: its groups in ascending order, slot 0 also the elements behind the last whole group
template <int PASS> GAZ_DEV void opt_slot(const OptArgs& a, const float* w, const float* g, int len, int slot, float proj, double* acc) {
    const int G = len >> 2;
#pragma unroll
    for (int i = 0; i < OPT_GPS; ++i) {
        const int j = slot + i * OPT_THREADS;
        if (j < G) {
            const OptF4 W = ((const OptF4*)w)[j], Gv = ((const OptF4*)g)[j];
            opt_term<PASS>(W.x, Gv.x, a, proj, acc); opt_term<PASS>(W.y, Gv.y, a, proj, acc);
            opt_term<PASS>(W.z, Gv.z, a, proj, acc); opt_term<PASS>(W.w, Gv.w, a, proj, acc);
        }
    }
    if (slot == 0)
        for (int k = G * 4; k < len; ++k) opt_term<PASS>(w[k], g[k], a, proj, acc);
}

// the N sums of one chunk -> out[N]; true in the thread that holds them (every call on the one-lane build).  All threads of the workgroup call it.
template <int PASS, int N> GAZ_DEV bool opt_reduce_chunk(const OptArgs& a, const float* w, const float* g, int len, float proj, double* out) {
#ifdef GAZ_HOST_EMU
    static thread_local double x[N][OPT_THREADS];
    static thread_local double y[OPT_THREADS];
    for (int s = 0; s < OPT_THREADS; ++s) {
        double acc[N];
        for (int k = 0; k < N; ++k) acc[k] = 0.0;
        opt_slot<PASS>(a, w, g, len, s, proj, acc);
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
    opt_slot<PASS>(a, w, g, len, (int)threadIdx.x, proj, acc);
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

// the value lane j of the wavefront holds; j is uniform
GAZ_DEV double opt_lane_value(double v, int j) {
#ifdef GAZ_HOST_EMU
    (void)j;
    return v;
#else
    int p[2];
    memcpy(p, &v, 8);
    p[0] = __builtin_amdgcn_readlane(p[0], j); p[1] = __builtin_amdgcn_readlane(p[1], j);
    memcpy(&v, p, 8);
    return v;
#endif
}

// sums[k], k = K0 .. K1 - 1, of a tensor: its chunks' sums in ascending order.  Every lane of every wavefront ends with the same values.
template <int K0, int K1> GAZ_DEV void opt_tensor_sums(const double* part, int first_chunk, int nc, double* sums) {
#pragma unroll
    for (int k = K0; k < K1; ++k) sums[k] = 0.0;
    const int lane = lane_id();
    for (int base = 0; base < nc; base += WAVE) {
        double v[4] = {0.0, 0.0, 0.0, 0.0};
        const int idx = base + lane;
        if (idx < nc) {
#pragma unroll
            for (int k = K0; k < K1; ++k) v[k] = part[(long long)(first_chunk + idx) * 4 + k];
        }
        const int cnt = nc - base < WAVE ? nc - base : WAVE;
        for (int j = 0; j < cnt; ++j) {
#pragma unroll
            for (int k = K0; k < K1; ++k) sums[k] = sums[k] + opt_lane_value(v[k], j);
        }
    }
}

GAZ_DEV float opt_proj(const double* sums) { return (float)sums[0] / ((float)sums[1] + 1e-30f); }
GAZ_DEV float opt_scale(const double* sums) { return __builtin_sqrtf((float)sums[2]) / (__builtin_sqrtf((float)sums[3]) + 1e-30f); }

struct OptPlace { const float* w; const float* g; long long at; int len; int tensor, index, first_chunk, n_chunks; };
GAZ_DEV OptPlace opt_place(const OptArgs& a) {
    const OptChunk c = a.chunks[block_id()];
    const OptTensor t = a.tens[c.tensor];
    const long long first = (long long)c.index * OPT_CHUNK;
    const long long left = t.n - first;
    OptPlace p;
    p.at = t.off + first; p.len = left < OPT_CHUNK ? (int)left : OPT_CHUNK; p.w = a.w + p.at; p.g = a.g + p.at;
    p.tensor = c.tensor; p.index = c.index; p.first_chunk = t.first_chunk; p.n_chunks = t.n_chunks;
    return p;
}

GAZ_OPT_BOUNDS GAZ_KERNEL_WIDE k_optim_dots(OptArgs a) {
    const OptPlace p = opt_place(a);
    double out[3];
    if (opt_reduce_chunk<1, 3>(a, p.w, p.g, p.len, 0.f, out)) {
        double* dst = a.part + (long long)block_id() * 4;
        dst[0] = out[0]; dst[1] = out[1]; dst[2] = out[2];
    }
}

GAZ_OPT_BOUNDS GAZ_KERNEL_WIDE k_optim_gogo(OptArgs a) {
    const OptPlace p = opt_place(a);
    double sums[4] = {0.0, 0.0, 0.0, 0.0};
    opt_tensor_sums<0, 3>(a.part, p.first_chunk, p.n_chunks, sums);
    const float proj = opt_proj(sums);
    double out[1];
    if (opt_reduce_chunk<2, 1>(a, p.w, p.g, p.len, proj, out)) {
        a.part[(long long)block_id() * 4 + 3] = out[0];
        if (p.index == 0) { double* n = a.norms + (long long)p.tensor * 4; n[0] = sums[0]; n[1] = sums[1]; n[2] = sums[2]; }
    }
}

// stages 2 and 3 of one element: Orthograd's rescale and Grokfast -> g2
GAZ_DEV float opt_g2(const OptArgs& a, float proj, float s, float w1, float g, float& e) {
    float g1 = g;
    if (a.ortho) {
        const float p = proj * w1;
        const float go = g - p;
        g1 = go * s;
    }
    float g2 = g1;
    if (a.grok) {
        const float ea = e * a.alpha;
        const float gb = g1 * a.oma;
        e = ea + gb;
        const float el = e * a.lamb;
        g2 = g1 + el;
    }
    return g2;
}

// stage 4 of one element up to the update u, which the caller scales by its learning rate
GAZ_DEV float opt_adam(const OptArgs& a, float g2, float& m, float& v) {
    const float m1 = a.b1 * m;
    const float m2 = a.omb1 * g2;
    m = m1 + m2;
    const float v1 = a.b2 * v;
    const float gg = g2 * g2;
    const float v2 = a.omb2 * gg;
    v = v1 + v2;
    const float mh = m / a.c1;
    const float vh = v / a.c2;
    float num = mh;
    if (a.kind == 1) {
        const float n1 = mh * a.b1;
        const float n2 = m2 / a.c1;
        num = n1 + n2;
    }
    const float den = __builtin_sqrtf(vh) + a.eps;
    return num / den;
}

// one element through the stages 1 .. 5
GAZ_DEV void opt_update(const OptArgs& a, float proj, float s, float& w, float& g, float& m, float& v, float& e) {
    const float w1 = opt_decayed(w, a.wd, a.lr);
    const float g2 = opt_g2(a, proj, s, w1, g, e);
    const float u = opt_adam(a, g2, m, v);
    const float ul = u * a.lr;
    w = w1 - ul;
    if (a.zero) g = 0.f;
}

GAZ_DEV void opt_apply_slot(const OptArgs& a, long long at, int len, int slot, float proj, float s) {
    const int G = len >> 2;
    float zero_e = 0.f;
#pragma unroll
    for (int i = 0; i < OPT_GPS; ++i) {
        const int j = slot + i * OPT_THREADS;
        if (j < G) {
            OptF4* pw = (OptF4*)(a.w + at) + j; OptF4* pg = (OptF4*)(a.g + at) + j; OptF4* pm = (OptF4*)(a.m + at) + j; OptF4* pv = (OptF4*)(a.v + at) + j;
            OptF4 W = *pw, Gv = *pg, M = *pm, V = *pv, E = {0.f, 0.f, 0.f, 0.f};
            if (a.grok) E = *((OptF4*)(a.e + at) + j);
            opt_update(a, proj, s, W.x, Gv.x, M.x, V.x, E.x); opt_update(a, proj, s, W.y, Gv.y, M.y, V.y, E.y);
            opt_update(a, proj, s, W.z, Gv.z, M.z, V.z, E.z); opt_update(a, proj, s, W.w, Gv.w, M.w, V.w, E.w);
            *pw = W; *pm = M; *pv = V;
            if (a.zero) *pg = Gv;
            if (a.grok) *((OptF4*)(a.e + at) + j) = E;
        }
    }
    if (slot == 0)
        for (int k = G * 4; k < len; ++k)
            opt_update(a, proj, s, a.w[at + k], a.g[at + k], a.m[at + k], a.v[at + k], a.grok ? a.e[at + k] : zero_e);
}

GAZ_OPT_BOUNDS GAZ_KERNEL_WIDE k_optim_apply(OptArgs a) {
    const OptPlace p = opt_place(a);
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
    for (int slot = 0; slot < OPT_THREADS; ++slot) opt_apply_slot(a, p.at, p.len, slot, proj, s);
#else
    opt_apply_slot(a, p.at, p.len, (int)threadIdx.x, proj, s);
#endif
}

}  // namespace gaz

#include "muon.hpp"

// ------------------------------------------------------------------------------------------------------------------------ the host side
struct gaz_optim {
    gaz_optim_config cfg;
    std::string err;
    std::vector<long long> sizes, offs;
    long long total = 0;
    int n_chunks = 0;
    float* d_arena[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    gaz::OptTensor* d_tens = nullptr; gaz::OptChunk* d_chunks = nullptr; double* d_part = nullptr; double* d_norms = nullptr;
    hipStream_t stream{};                                                     // the default stream: in order with the caller's own work there
    hipEvent_t ev0{}, ev1{}; bool have_events = false;
    gaz::OptArgs base;
    // Muon mode (gaz_muon_set): the per-tensor table, the work tables, two X buffers of the arenas' layout, A and B of every Muon tensor
    bool muon = false, stepped = false;
    int ns_steps = 0, n_pp = 0, n_pq = 0, n_thin = 0, n_muon = 0;
    double adam_lr_ratio = 1.0;
    std::vector<gaz::MuonTensor> mtens;
    long long ab_total = 0;
    gaz::MuonTensor* d_mt = nullptr; gaz::MuonTile* d_pp = nullptr; gaz::MuonTile* d_pq = nullptr; gaz::MuonTile* d_thin = nullptr;
    float* d_x[2] = {nullptr, nullptr}; float* d_A = nullptr; float* d_B = nullptr; float* d_nrm = nullptr; double* d_gpart = nullptr; double* d_npart = nullptr;
    gaz::MuonArgs mbase;

    int fail(const std::string& m) { err = m; return 1; }
#define GAZ_OP_CK(expr) \
    do { hipError_t _e = (expr); if (_e != hipSuccess) { return fail(std::string(#expr) + ": " + hipGetErrorString(_e)); } } while (0)

    ~gaz_optim() {
        hipStreamSynchronize(stream);
        for (float* p : d_arena) if (p) hipFree(p);
        void* all[] = {d_tens, d_chunks, d_part, d_norms, d_mt, d_pp, d_pq, d_thin, d_x[0], d_x[1], d_A, d_B, d_nrm, d_gpart, d_npart};
        for (void* p : all) if (p) hipFree(p);
        if (have_events) { hipEventDestroy(ev0); hipEventDestroy(ev1); }
    }
    int launches() const {
        const int base_launches = cfg.orthograd ? 3 : 1;
        if (!muon || n_muon == 0) return base_launches;
        return base_launches + 2 + ns_steps * ((n_pp + n_thin > 0) + (n_pp > 0) + 1);     // norm and finish; gram, poly (general tensors only), update
    }

    int init(std::string* why) {
        const int T = cfg.n_tensors;
        offs.resize((size_t)T);
        std::vector<gaz::OptTensor> tens((size_t)T);
        std::vector<gaz::OptChunk> chunks;
        long long at = 0;
        for (int k = 0; k < T; ++k) {
            offs[(size_t)k] = at;
            const int nc = (int)((sizes[(size_t)k] + gaz::OPT_CHUNK - 1) / gaz::OPT_CHUNK);
            tens[(size_t)k] = gaz::OptTensor{at, sizes[(size_t)k], (int)chunks.size(), nc};
            for (int c = 0; c < nc; ++c) chunks.push_back(gaz::OptChunk{k, c});
            at += (sizes[(size_t)k] + 3) / 4 * 4;
        }
        total = at; n_chunks = (int)chunks.size();
        bool ok = hipSetDevice(cfg.device) == hipSuccess;
        for (int i = 0; ok && i < 5; ++i)
            if (i < 4 || cfg.grokfast) ok = hipMalloc((void**)&d_arena[i], (size_t)total * 4) == hipSuccess && hipMemset(d_arena[i], 0, (size_t)total * 4) == hipSuccess;
        ok = ok && hipMalloc((void**)&d_tens, tens.size() * sizeof(gaz::OptTensor)) == hipSuccess && hipMalloc((void**)&d_chunks, chunks.size() * sizeof(gaz::OptChunk)) == hipSuccess
                && hipMalloc((void**)&d_part, (size_t)n_chunks * 32) == hipSuccess && hipMalloc((void**)&d_norms, (size_t)T * 32) == hipSuccess
                && hipMemset(d_part, 0, (size_t)n_chunks * 32) == hipSuccess && hipMemset(d_norms, 0, (size_t)T * 32) == hipSuccess
                && hipMemcpy(d_tens, tens.data(), tens.size() * sizeof(gaz::OptTensor), hipMemcpyHostToDevice) == hipSuccess
                && hipMemcpy(d_chunks, chunks.data(), chunks.size() * sizeof(gaz::OptChunk), hipMemcpyHostToDevice) == hipSuccess
                && hipEventCreate(&ev0) == hipSuccess && hipEventCreate(&ev1) == hipSuccess;
        have_events = ok;
        ok = ok && hipDeviceSynchronize() == hipSuccess;
        if (!ok) { *why = "optim_create: allocation failure: five arenas of " + std::to_string(total) + " floats do not fit on device " + std::to_string(cfg.device); (void)hipGetLastError(); return 1; }
        gaz::OptArgs& a = base;
        memset(&a, 0, sizeof(a));
        a.w = d_arena[0]; a.g = d_arena[1]; a.m = d_arena[2]; a.v = d_arena[3]; a.e = d_arena[4];
        a.tens = d_tens; a.chunks = d_chunks; a.part = d_part; a.norms = d_norms;
        a.wd = (float)cfg.weight_decay; a.b1 = (float)cfg.beta_1; a.b2 = (float)cfg.beta_2; a.eps = (float)cfg.epsilon; a.alpha = (float)cfg.alpha; a.lamb = (float)cfg.lamb;
        a.omb1 = 1.0f - a.b1; a.omb2 = 1.0f - a.b2; a.oma = 1.0f - a.alpha;
        a.kind = cfg.kind; a.ortho = cfg.orthograd; a.grok = cfg.grokfast;
        return 0;
    }

    int check_range(const char* fn, int32_t arena, int64_t first, int64_t n, const void* p) {
        if (arena < 0 || arena > 4) return fail(std::string(fn) + ": arena must be 0 (params), 1 (grads), 2 (momentum), 3 (velocity) or 4 (ema), not " + std::to_string(arena));
        if (arena == 4 && !cfg.grokfast) return fail(std::string(fn) + ": this optimizer has no ema arena (grokfast is off)");
        if (first < 0 || n < 0 || first > total || n > total - first)
            return fail(std::string(fn) + ": elements " + std::to_string(first) + " .. " + std::to_string(first + n) + " of an arena of " + std::to_string(total));
        if (n > 0 && !p) return fail(std::string(fn) + ": null argument");
        return 0;
    }
    int read(int32_t arena, int64_t first, int64_t n, float* out) {
        if (check_range("optim_read", arena, first, n, out)) return 1;
        GAZ_OP_CK(hipStreamSynchronize(stream));
        if (n) GAZ_OP_CK(hipMemcpy(out, d_arena[arena] + first, (size_t)n * 4, hipMemcpyDeviceToHost));
        return 0;
    }
    int write(int32_t arena, int64_t first, int64_t n, const float* in) {
        if (check_range("optim_write", arena, first, n, in)) return 1;
        if (n == 0) return 0;
        std::vector<float> tmp(in, in + n);
        for (size_t k = 0; k < sizes.size(); ++k) {                               // the pads inside the range stay zero
            const long long p0 = offs[k] + sizes[k], p1 = k + 1 < sizes.size() ? offs[k + 1] : total;
            for (long long i = p0 > first ? p0 : first; i < p1 && i < first + n; ++i) tmp[(size_t)(i - first)] = 0.f;
        }
        GAZ_OP_CK(hipStreamSynchronize(stream));
        GAZ_OP_CK(hipMemcpy(d_arena[arena] + first, tmp.data(), (size_t)n * 4, hipMemcpyHostToDevice));
        return 0;
    }

    int set_muon(const gaz_muon_config* c) {
        if (!c) return fail("muon_set: null argument");
        if (c->struct_size != sizeof(gaz_muon_config))
            return fail("gaz_muon_config.struct_size is " + std::to_string(c->struct_size) + ", this library's gaz_muon_config has " + std::to_string(sizeof(gaz_muon_config)) +
                        " bytes: rebuild the binding from include/gaz_engine.h");
        if (muon) return fail("muon_set: this optimizer is in Muon mode already");
        if (stepped) return fail("muon_set: call it before the first step");
        const int T = cfg.n_tensors;
        if (c->n_tensors != T) return fail("muon_set: n_tensors is " + std::to_string(c->n_tensors) + ", the optimizer has " + std::to_string(T) + " tensors");
        if (!c->rows || !c->cols || !c->scale) return fail("muon_set: null rows, cols or scale");
        if (c->ns_steps < 0 || c->ns_steps > 16) return fail("muon_set: ns_steps must be in 0 .. 16, not " + std::to_string(c->ns_steps));
        if (!(c->muon_a - c->muon_a == 0.0 && c->muon_b - c->muon_b == 0.0 && c->muon_c - c->muon_c == 0.0)) return fail("muon_set: muon_a, muon_b and muon_c must be finite");
        if (!(c->muon_beta >= 0.0 && c->muon_beta < 1.0)) return fail("muon_set: muon_beta must be in [0, 1), not " + std::to_string(c->muon_beta));
        if (!(c->adam_lr_ratio >= 0.0 && c->adam_lr_ratio - c->adam_lr_ratio == 0.0)) return fail("muon_set: adam_lr_ratio must be finite and not negative");
        if (c->nesterov != 0 && c->nesterov != 1) return fail("muon_set: nesterov must be 0 or 1");
        std::vector<gaz::MuonTensor> mt((size_t)T);
        std::vector<gaz::MuonTile> pp, pq, thin;
        long long ab = 0;
        int nm = 0;
        for (int k = 0; k < T; ++k) {
            gaz::MuonTensor& m = mt[(size_t)k];
            memset(&m, 0, sizeof(m));
            const long long r = c->rows[k], q = c->cols[k];
            if (r == 0 && q == 0) continue;                                       // an Adam tensor
            if (r < 1 || q < 1 || r * q != sizes[(size_t)k])
                return fail("muon_set: tensor " + std::to_string(k) + ": rows * cols = " + std::to_string(r) + " * " + std::to_string(q) + " is not its size " + std::to_string(sizes[(size_t)k]));
            if (!(c->scale[k] - c->scale[k] == 0.f)) return fail("muon_set: tensor " + std::to_string(k) + ": scale must be finite");
            const bool tr = r > q;                                                // iterate on the transpose: element (p, q) of X at p * sp + q * sq
            m.off = offs[(size_t)k]; m.aoff = ab; m.P = (int)(tr ? q : r); m.Q = (int)(tr ? r : q); m.sp = tr ? 1 : (int)q; m.sq = tr ? (int)q : 1; m.scale = c->scale[k];
            m.thin = m.P <= gaz::MU_THIN;
            ab += ((long long)m.P * m.P + 3) / 4 * 4;
            ++nm;
            if (m.thin) {
                m.first_thin = (int)thin.size(); m.n_thin = (m.Q + gaz::OPT_CHUNK - 1) / gaz::OPT_CHUNK;
                for (int ch = 0; ch < m.n_thin; ++ch) thin.push_back(gaz::MuonTile{k, ch, 0});
            } else {
                const int tp = (m.P + gaz::MU_TILE - 1) / gaz::MU_TILE, tq = (m.Q + gaz::MU_TILE - 1) / gaz::MU_TILE;
                for (int i = 0; i < tp; ++i) for (int j = 0; j < tp; ++j) pp.push_back(gaz::MuonTile{k, i, j});
                for (int i = 0; i < tp; ++i) for (int j = 0; j < tq; ++j) pq.push_back(gaz::MuonTile{k, i, j});
            }
        }
        auto table = [](auto** dst, const auto& v) {
            const size_t bytes = (v.size() ? v.size() : 1) * sizeof(v[0]);
            return hipMalloc((void**)dst, bytes) == hipSuccess && (v.empty() || hipMemcpy(*dst, v.data(), v.size() * sizeof(v[0]), hipMemcpyHostToDevice) == hipSuccess);
        };
        auto zeros = [](auto** dst, size_t bytes) { return hipMalloc((void**)dst, bytes ? bytes : 1) == hipSuccess && hipMemset(*dst, 0, bytes ? bytes : 1) == hipSuccess; };
        bool ok = hipStreamSynchronize(stream) == hipSuccess && table(&d_mt, mt) && table(&d_pp, pp) && table(&d_pq, pq) && table(&d_thin, thin)
               && zeros(&d_x[0], (size_t)total * 4) && zeros(&d_x[1], (size_t)total * 4) && zeros(&d_A, (size_t)ab * 4) && zeros(&d_B, (size_t)ab * 4)
               && zeros(&d_nrm, (size_t)T * 4) && zeros(&d_gpart, thin.size() * gaz::MU_PAIRS * 8) && zeros(&d_npart, (size_t)n_chunks * 32)
               && hipDeviceSynchronize() == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            void** all[] = {(void**)&d_mt, (void**)&d_pp, (void**)&d_pq, (void**)&d_thin, (void**)&d_x[0], (void**)&d_x[1], (void**)&d_A, (void**)&d_B, (void**)&d_nrm, (void**)&d_gpart, (void**)&d_npart};
            for (void** p : all) { if (*p) hipFree(*p); *p = nullptr; }
            return fail("muon_set: allocation failure: two X buffers of " + std::to_string(total) + " floats and A, B of " + std::to_string(ab) + " do not fit");
        }
        mtens = mt; ab_total = ab; n_pp = (int)pp.size(); n_pq = (int)pq.size(); n_thin = (int)thin.size(); n_muon = nm;
        ns_steps = c->ns_steps; adam_lr_ratio = c->adam_lr_ratio;
        gaz::MuonArgs& m = mbase;
        memset(&m, 0, sizeof(m));
        m.mt = d_mt; m.pp = d_pp; m.pq = d_pq; m.thin = d_thin; m.n_pp = n_pp; m.n_pq = n_pq; m.n_thin = n_thin; m.nesterov = c->nesterov;
        m.A = d_A; m.B = d_B; m.nrm = d_nrm; m.gpart = d_gpart; m.npart = d_npart;
        m.beta = (float)c->muon_beta; m.omb = 1.0f - m.beta;
        m.ca = gaz::bf16r((float)c->muon_a); m.cb = gaz::bf16r((float)c->muon_b); m.cc = gaz::bf16r((float)c->muon_c);
        m.wd = base.wd;
        base.wd = 0.f;                                                            // Orthograd sees the undecayed w; the decay follows the update
        muon = true;
        return 0;
    }

    int step_muon(gaz::OptArgs a) {
        gaz::MuonArgs m = mbase;
        m.lr_adam = (float)adam_lr_ratio * a.lr;
        m.xs = d_x[1]; m.xd = d_x[0];
        GAZ_LAUNCH(gaz::k_optim_apply_muon, n_chunks, gaz::OPT_THREADS, stream, a, m);
        if (n_muon == 0) return 0;
        GAZ_LAUNCH(gaz::k_muon_norm, n_chunks, gaz::OPT_THREADS, stream, a, m);
        int cur = 0;
        for (int it = 0; it < ns_steps; ++it) {
            m.xs = d_x[cur]; m.xd = d_x[cur ^ 1];
            GAZ_LAUNCH(gaz::k_muon_gram, n_pp + n_thin, gaz::OPT_THREADS, stream, m);
            if (n_pp) GAZ_LAUNCH(gaz::k_muon_poly, n_pp, gaz::OPT_THREADS, stream, m);
            GAZ_LAUNCH(gaz::k_muon_update, n_pq + n_thin, gaz::OPT_THREADS, stream, m);
            cur ^= 1;
        }
        m.xs = d_x[cur]; m.xd = d_x[cur ^ 1];
        GAZ_LAUNCH(gaz::k_muon_finish, n_chunks, gaz::OPT_THREADS, stream, a, m);
        return 0;
    }

    // what: 0 X0 [size], 1 n [1], 2 the final X [size], 3 / 4 A / B of the last iteration [P * P], P = min(rows, cols)
    int read_muon(int32_t tensor, int32_t what, float* out) {
        if (!muon) return fail("muon_read: this optimizer is not in Muon mode");
        if (tensor < 0 || tensor >= cfg.n_tensors) return fail("muon_read: tensor " + std::to_string(tensor) + " of " + std::to_string(cfg.n_tensors));
        const gaz::MuonTensor& t = mtens[(size_t)tensor];
        if (t.P == 0) return fail("muon_read: tensor " + std::to_string(tensor) + " is an Adam tensor");
        if (what < 0 || what > 4) return fail("muon_read: what must be 0 (X0), 1 (n), 2 (X), 3 (A) or 4 (B), not " + std::to_string(what));
        if (!out) return fail("muon_read: null argument");
        GAZ_OP_CK(hipStreamSynchronize(stream));
        const size_t n = (size_t)sizes[(size_t)tensor], pp = (size_t)t.P * t.P;
        if (what == 0) {
            GAZ_OP_CK(hipMemcpy(out, d_arena[3] + t.off, n * 4, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < n; ++i) out[i] = gaz::bf16r(out[i]);
        } else if (what == 1) GAZ_OP_CK(hipMemcpy(out, d_nrm + tensor, 4, hipMemcpyDeviceToHost));
        else if (what == 2) GAZ_OP_CK(hipMemcpy(out, d_x[ns_steps & 1] + t.off, n * 4, hipMemcpyDeviceToHost));
        else GAZ_OP_CK(hipMemcpy(out, (what == 3 ? d_A : d_B) + t.aoff, pp * 4, hipMemcpyDeviceToHost));
        return 0;
    }

    int step(double lr, int64_t t, int32_t zero_grads) {
        if (t < 1) return fail("optim_step: t must be at least 1, not " + std::to_string(t));
        if (!(lr - lr == 0.0)) return fail("optim_step: lr must be finite");
        stepped = true;
        gaz::OptArgs a = base;
        a.lr = (float)lr; a.zero = zero_grads != 0;
        a.c1 = (float)(1.0 - gaz::det::dpow(cfg.beta_1, (double)t)); a.c2 = (float)(1.0 - gaz::det::dpow(cfg.beta_2, (double)t));
        if (cfg.orthograd) {
            GAZ_LAUNCH(gaz::k_optim_dots, n_chunks, gaz::OPT_THREADS, stream, a);
            GAZ_LAUNCH(gaz::k_optim_gogo, n_chunks, gaz::OPT_THREADS, stream, a);
        }
        if (muon) step_muon(a);
        else GAZ_LAUNCH(gaz::k_optim_apply, n_chunks, gaz::OPT_THREADS, stream, a);
        GAZ_OP_CK(hipGetLastError());
        return 0;
    }
    int step_timed(double lr, int64_t t, int32_t zero_grads, int32_t repeats, double* ms_per_step) {
        if (repeats < 1 || !ms_per_step) return fail("optim_step_timed: repeats must be at least 1");
        if (step(lr, t, zero_grads)) return 1;                                    // (checks, warms up)
        GAZ_OP_CK(hipEventRecord(ev0, stream));
        int rc = 0;
        for (int i = 0; i < repeats && !rc; ++i) rc = step(lr, t + i, zero_grads);
        GAZ_OP_CK(hipEventRecord(ev1, stream));
        GAZ_OP_CK(hipEventSynchronize(ev1));
        float ms = 0.f;
        GAZ_OP_CK(hipEventElapsedTime(&ms, ev0, ev1));
        *ms_per_step = (double)ms / repeats;
        return rc;
    }
    int read_norms(double* out) {
        if (!out) return fail("optim_read_norms: null argument");
        GAZ_OP_CK(hipStreamSynchronize(stream));
        GAZ_OP_CK(hipMemcpy(out, d_norms, sizes.size() * 32, hipMemcpyDeviceToHost));
        return 0;
    }
#undef GAZ_OP_CK
};

static std::string g_optim_create_error;

extern "C" {

int gaz_optim_config_size(void) { return (int)sizeof(gaz_optim_config); }

int gaz_optim_create(const gaz_optim_config* cfg, gaz_optim** out) {
    std::string& e = g_optim_create_error;
    if (!cfg || !out) { e = "optim_create: null argument"; return 1; }
    *out = nullptr;
    if (cfg->struct_size != sizeof(gaz_optim_config)) {
        e = "gaz_optim_config.struct_size is " + std::to_string(cfg->struct_size) + ", this library's gaz_optim_config has " + std::to_string(sizeof(gaz_optim_config)) +
            " bytes: rebuild the binding from include/gaz_engine.h";
        return 1;
    }
    if (cfg->n_tensors < 1) { e = "optim_create: n_tensors must be at least 1, not " + std::to_string(cfg->n_tensors); return 1; }
    if (!cfg->sizes) { e = "optim_create: null sizes"; return 1; }
    long long sum = 0;
    for (int32_t k = 0; k < cfg->n_tensors; ++k) {
        if (cfg->sizes[k] < 1) { e = "optim_create: sizes[" + std::to_string(k) + "] must be at least 1, not " + std::to_string(cfg->sizes[k]); return 1; }
        if (cfg->sizes[k] >= (1ll << 40) || (sum += cfg->sizes[k] + 3) >= (1ll << 40)) { e = "optim_create: the tensors must have fewer than 2^40 elements in all"; return 1; }
    }
    if (cfg->kind != 0 && cfg->kind != 1) { e = "optim_create: kind must be 0 (Adam) or 1 (Nadam), not " + std::to_string(cfg->kind); return 1; }
    if (!(cfg->beta_1 >= 0.0 && cfg->beta_1 < 1.0)) { e = "optim_create: beta_1 must be in [0, 1), not " + std::to_string(cfg->beta_1); return 1; }
    if (!(cfg->beta_2 >= 0.0 && cfg->beta_2 < 1.0)) { e = "optim_create: beta_2 must be in [0, 1), not " + std::to_string(cfg->beta_2); return 1; }
    if (!(cfg->epsilon >= 0.0 && cfg->epsilon - cfg->epsilon == 0.0)) { e = "optim_create: epsilon must be finite and not negative"; return 1; }
    if (!(cfg->weight_decay >= 0.0 && cfg->weight_decay - cfg->weight_decay == 0.0)) { e = "optim_create: weight_decay must be finite and not negative"; return 1; }
    if ((cfg->orthograd != 0 && cfg->orthograd != 1) || (cfg->grokfast != 0 && cfg->grokfast != 1)) { e = "optim_create: orthograd and grokfast must be 0 or 1"; return 1; }
    if (!(cfg->alpha - cfg->alpha == 0.0 && cfg->lamb - cfg->lamb == 0.0)) { e = "optim_create: alpha and lamb must be finite"; return 1; }
    gaz_optim* h = new gaz_optim();
    h->cfg = *cfg;
    h->sizes.assign(cfg->sizes, cfg->sizes + cfg->n_tensors);
    h->cfg.sizes = nullptr;                                                      // (the caller's array is read here only)
    if (h->init(&e)) { delete h; return 1; }
    *out = h;
    return 0;
}
void gaz_optim_destroy(gaz_optim* h) { delete h; }
const char* gaz_optim_last_error(gaz_optim* h) { return h ? h->err.c_str() : g_optim_create_error.c_str(); }
int gaz_optim_layout(gaz_optim* h, int64_t* offsets, int64_t info[5]) {
    for (size_t k = 0; offsets && k < h->offs.size(); ++k) offsets[k] = h->offs[k];
    if (info) { info[0] = h->total; info[1] = h->n_chunks; info[2] = gaz::OPT_CHUNK; info[3] = h->launches(); info[4] = gaz::WAVE == 1 ? 1 : 0; }
    return 0;
}
int gaz_optim_ptrs(gaz_optim* h, void** params, void** grads, void** momentum, void** velocity, void** ema) {
    void** out[] = {params, grads, momentum, velocity, ema};
    for (int i = 0; i < 5; ++i) if (out[i]) *out[i] = h->d_arena[i];
    return 0;
}
int gaz_optim_read(gaz_optim* h, int32_t arena, int64_t first, int64_t n, float* out) { return h->read(arena, first, n, out); }
int gaz_optim_write(gaz_optim* h, int32_t arena, int64_t first, int64_t n, const float* in) { return h->write(arena, first, n, in); }
int gaz_optim_step(gaz_optim* h, double lr, int64_t t, int32_t zero_grads) { return h->step(lr, t, zero_grads); }
int gaz_optim_step_timed(gaz_optim* h, double lr, int64_t t, int32_t zero_grads, int32_t repeats, double* ms_per_step) { return h->step_timed(lr, t, zero_grads, repeats, ms_per_step); }
int gaz_optim_read_norms(gaz_optim* h, double* out) { return h->read_norms(out); }
int gaz_muon_config_size(void) { return (int)sizeof(gaz_muon_config); }
int gaz_muon_set(gaz_optim* h, const gaz_muon_config* cfg) { return h->set_muon(cfg); }
int gaz_muon_read(gaz_optim* h, int32_t tensor, int32_t what, float* out) { return h->read_muon(tensor, what, out); }
int gaz_optim_synchronize(gaz_optim* h) {
    const hipError_t e = hipStreamSynchronize(h->stream);
    return e == hipSuccess ? 0 : h->fail(std::string("optim_synchronize: ") + hipGetErrorString(e));
}

}  // extern "C"
