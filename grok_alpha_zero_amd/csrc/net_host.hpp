// net_host.hpp — host side shared by the two network evaluators of resnet.hip (ResNetEvaluator: Connect4; GenericEvaluator: Gomoku /
// TicTacToe): the device tensor store, the timing bracket around the trunk, the stamp dump, the k_stem_mfma launch,
// the width dispatch and the k_conv_wide trunk.  No device code lives here: every kernel is declared by the headers included below.
#pragma once
#include <map>
#include <string>
#include <type_traits>
#include <vector>
#include "evaluator.hpp"
#include "conv_common.hpp"
#include "conv_wide.hpp"
#include "netops.hpp"
#include "trunk.hpp"

namespace gaz {

inline bf16_t f2bf_host(float f) { unsigned u; memcpy(&u, &f, 4); return (bf16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16); }    // round to nearest even

// ---- device tensors of one evaluator: every allocation (freed here), the host tensors of the load call by name, the uploaded fp32 tensors
// and bf16 convolution operands by name, and the text of the first error.
enum ConvOrder { CONV_MFMA, CONV_WIDE };            // arrange_conv_weights (conv_common.hpp) | arrange_wide_weights (conv_wide.hpp)
struct DeviceStore {
    std::vector<void*> allocs; std::string err;
    std::map<std::string, const gaz_tensor*> by; std::map<std::string, float*> f32; std::map<std::string, bf16_t*> b16;
    ~DeviceStore() { for (void* p : allocs) hipFree(p); }
    // Every allocation ends in PAD spare elements.  The convolution kernels read halo rows and whole 16-byte LDS-DMA slots next to the rows
    // they own and mask the values afterwards, so a buffer that ended exactly at its last element would have them read past the allocation.
    // Callers that need more slack add it to n (the Connect4 activation buffers: 1024 elements).  The padding may grow, never shrink.
    static constexpr size_t PAD = 64;
    template <class T> T* dalloc(size_t n) {
        void* p = nullptr;
        if (hipMalloc(&p, (n + PAD) * sizeof(T)) != hipSuccess) { err = "hipMalloc"; return nullptr; }
        allocs.push_back(p); return (T*)p;
    }
    template <class T> T* upload(const T* h, size_t n) { T* d = dalloc<T>(n); if (d) hipMemcpy(d, h, n * sizeof(T), hipMemcpyHostToDevice); return d; }
    void set_tensors(const gaz_tensor* t, int n) { by.clear(); for (int i = 0; i < n; ++i) by[t[i].name] = &t[i]; }
    const gaz_tensor* need(const std::string& name, int64_t numel) {
        auto it = by.find(name);
        if (it == by.end()) { err = "missing tensor " + name; return nullptr; }
        if (it->second->numel != numel) { err = "tensor " + name + " has " + std::to_string(it->second->numel) + " elements, expected " + std::to_string(numel); return nullptr; }
        return it->second;
    }
    float* g(const std::string& name) const { auto it = f32.find(name); return it == f32.end() ? nullptr : it->second; }
    bf16_t* w(const std::string& name) const { auto it = b16.find(name); return it == b16.end() ? nullptr : it->second; }
    bool up_f32(const std::string& name, int64_t numel) { const gaz_tensor* t = need(name, numel); return t && (f32[name] = upload(t->data, (size_t)numel)) != nullptr; }
    // convolution weights [ntaps][cout][cin] fp32 -> bf16 in the operand order of the kernel that reads them
    bool up_conv(const std::string& name, int cout, int cin, int ntaps, ConvOrder order) {
        const int64_t numel = (int64_t)ntaps * cout * cin;
        const gaz_tensor* t = need(name, numel); if (!t) return false;
        std::vector<bf16_t> h(numel);
        if (order == CONV_WIDE) arrange_wide_weights(t->data, cout, cin, ntaps, h.data(), f2bf_host);
        else arrange_conv_weights(t->data, cout, cin, h.data(), f2bf_host, ntaps);
        return (b16[name] = upload(h.data(), h.size())) != nullptr;
    }
    // conv1 / conv2 of a C -> C block in ONE allocation, conv2 right behind conv1: k_resblock3 and k_trunk walk them as 18 slices
    bool up_conv_pair(const std::string& n1, const std::string& n2, int C) {
        const int64_t numel = 9LL * C * C;
        const gaz_tensor* t1 = need(n1, numel); const gaz_tensor* t2 = need(n2, numel); if (!t1 || !t2) return false;
        std::vector<bf16_t> h(2 * numel);
        arrange_conv_weights(t1->data, C, C, h.data(), f2bf_host, 9);
        arrange_conv_weights(t2->data, C, C, h.data() + numel, f2bf_host, 9);
        bf16_t* d = upload(h.data(), h.size()); if (!d) return false;
        b16[n1] = d; b16[n2] = d + numel; return true;
    }
    // a[c] + b[c] on the host: conv2 and the projection of a projecting block share one accumulator, so they share one fp32 bias
    bool bias_sum(const std::string& a, const std::string& b, std::vector<float>& h) {
        const gaz_tensor* ta = need(a, by.count(a) ? by[a]->numel : 0); const gaz_tensor* tb = ta ? need(b, ta->numel) : nullptr;
        if (!tb) return false;
        h.resize(ta->numel);
        for (size_t c = 0; c < h.size(); ++c) h[c] = ta->data[c] + tb->data[c];
        return true;
    }
    bool up_bias_sum(const std::string& dst, const std::string& a, const std::string& b) { std::vector<float> h; return bias_sum(a, b, h) && (f32[dst] = upload(h.data(), h.size())) != nullptr; }
    // k_trunk operands of the 128 -> 128 blocks [first, first + n): their 18 slices each as one array (TrunkArgs::w), their parameters as
    // [block][5][128] (TrunkArgs::prm).  The blocks were uploaded with up_conv_pair.
    bool pack_trunk(int first, int n, bf16_t** w_out, float** prm_out) {
        const size_t WB = 18 * (size_t)128 * 128;
        bf16_t* tw = dalloc<bf16_t>(n * WB); float* tp = dalloc<float>((size_t)n * TR_PRM);
        if (!tw || !tp) return false;
        for (int i = 0; i < n; ++i) {
            const std::string b = "block" + std::to_string(first + i);
            hipMemcpy(tw + i * WB, w(b + ".conv1.w"), WB * 2, hipMemcpyDeviceToDevice);
            const char* names[5] = {".bn1.scale", ".bn1.shift", ".conv1.scale", ".conv1.shift", ".conv2.bias"};
            for (int k = 0; k < 5; ++k) hipMemcpy(tp + ((size_t)i * 5 + k) * 128, g(b + names[k]), 128 * 4, hipMemcpyDeviceToDevice);
        }
        *w_out = tw; *prm_out = tp; return true;
    }
};

// ---- event brackets around the trunk of each timed forward pass (engine timing: gaz_engine_trunk_timing)
struct TrunkTimer {
    std::vector<hipEvent_t> ev; bool open = false;  // ev: pairs
    ~TrunkTimer() { reset(); }
    void begin(hipStream_t s, bool on) {
        hipEvent_t e0 = 0, e1 = 0;
        if ((open = on)) { hipEventCreate(&e0); hipEventCreate(&e1); ev.push_back(e0); ev.push_back(e1); hipEventRecord(e0, s); }
    }
    void end(hipStream_t s) { if (open) hipEventRecord(ev.back(), s); open = false; }
    void reset() { for (auto e : ev) hipEventDestroy(e); ev.clear(); open = false; }
    int64_t brackets() const { return (int64_t)(ev.size() / 2); }
    double total_ms() const {
        double t = 0;
        for (size_t i = 0; i + 1 < ev.size(); i += 2) { float a = 0; hipEventElapsedTime(&a, ev[i], ev[i + 1]); t += a; }
        return t;
    }
};

// ---- diagnostic: the phase stamps one launch writes (GAZ_TRUNK_STAMPS / GAZ_RB_STAMPS) -> file.  path == nullptr: nothing happens and
// dev stays null (the kernels take a null stamp pointer as "off").
struct StampDump {
    const char* path; size_t n; hipStream_t s; unsigned long long* dev = nullptr;
    StampDump(const char* path_, size_t n_qwords, hipStream_t s_) : path(path_), n(n_qwords), s(s_) {
        if (path) { hipMalloc((void**)&dev, n * 8); hipMemsetAsync(dev, 0, n * 8, s); }
    }
    void finish() {
        if (!path) return;
        std::vector<unsigned long long> hst(n);
        hipStreamSynchronize(s);
        hipMemcpy(hst.data(), dev, hst.size() * 8, hipMemcpyDeviceToHost); hipFree(dev); dev = nullptr;
        if (FILE* f = fopen(path, "wb")) { fwrite(hst.data(), 8, hst.size(), f); fclose(f); }
    }
};

// ---- the residual widths of k_conv_wide as a compile-time constant: fn(std::integral_constant<int, F>)
template <class Fn> void with_width(int F, Fn&& fn) {
    switch (F) {
    case 64: fn(std::integral_constant<int, 64>{}); break;
    case 192: fn(std::integral_constant<int, 192>{}); break;
    default: fn(std::integral_constant<int, 256>{});
    }
}

// ---- the trunk at num_filters != 128 (conv_wide.hpp), one convolution per launch, for both networks.  The stem wrote x0 (SC channels); here:
// a0 = relu(bn1_0(x0)); block 0: conv1 SC -> F (a0 -> h), conv2 + the 1x1 projection SC -> F of x0 in one accumulator (h, x0 -> x) — or, where
// SC == F (Gomoku at 256), conv2 + x0 as a plain residual; blocks 1..: conv1 (a -> h), conv2 + residual (h, x -> x).  Every conv2 also writes
// the next block's operand relu(bn1(bf16 x)) -> a; the last one writes relu(p.bn0(bf16 x)) -> a where the policy head starts from it
// (policy_preact: Gomoku) and nothing otherwise (Connect4).  x may be the buffer of a0: a0 is dead when block 0's conv2 writes.
struct WideTrunk { int stem_c, F, blocks, M, H, W; bf16_t *x0, *a0, *x, *a, *h; bool policy_preact; };      // stem_c: 128 (Connect4) or 256 (Gomoku)
template <int SC> void forward_trunk_wide_sc(hipStream_t s, const DeviceStore& st, TrunkTimer& timer, bool timing, const WideTrunk& t) {
    const long n8 = (long)t.M * SC / 8;
    hipLaunchKernelGGL(k_affine_relu, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, s, t.x0, st.g("block0.bn1.scale"), st.g("block0.bn1.shift"), t.a0, n8, SC);
    timer.begin(s, timing);
    for (int i = 0; i < t.blocks; ++i) {
        const std::string b = "block" + std::to_string(i), nb = "block" + std::to_string(i + 1);
        const bool last = i + 1 == t.blocks, proj = i == 0 && SC != t.F;      // block 0 projects unless the stem already has F channels
        WideConvArgs c1; memset(&c1, 0, sizeof(c1));
        c1.in = i == 0 ? t.a0 : t.a; c1.wgt = st.w(b + ".conv1.w"); c1.scaleA = st.g(b + ".conv1.scale"); c1.shiftA = st.g(b + ".conv1.shift");
        c1.out1 = t.h; c1.act1 = ACT_RELU; c1.M = t.M; c1.H = t.H; c1.W = t.W;
        WideConvArgs c2; memset(&c2, 0, sizeof(c2));
        c2.in = t.h; c2.wgt = st.w(b + ".conv2.w"); c2.out1 = t.x; c2.act1 = ACT_NONE; c2.M = t.M; c2.H = t.H; c2.W = t.W;
        if (!last) { c2.scaleB = st.g(nb + ".bn1.scale"); c2.shiftB = st.g(nb + ".bn1.shift"); c2.out2 = t.a; }
        else if (t.policy_preact) { c2.scaleB = st.g("p.bn0.scale"); c2.shiftB = st.g("p.bn0.shift"); c2.out2 = t.a; }
        if (proj) { c2.in2 = t.x0; c2.wgt2 = st.w(b + ".proj.w"); c2.shiftA = st.g(b + ".bias2p"); }
        else { c2.shiftA = st.g(b + ".conv2.bias"); c2.res = i == 0 ? t.x0 : t.x; }
        with_width(t.F, [&](auto Fc) {
            constexpr int F = decltype(Fc)::value;
            if (i == 0) conv_wide_launch<SC, F, 9, 0, CW_EPI_BF16>(s, c1); else conv_wide_launch<F, F, 9, 0, CW_EPI_BF16>(s, c1);
            if constexpr (SC != F) { if (proj) { conv_wide_launch<F, F, 9, SC, CW_EPI_BF16>(s, c2); return; } }
            conv_wide_launch<F, F, 9, 0, CW_EPI_BF16>(s, c2);
        });
    }
    timer.end(s);
}
inline void forward_trunk_wide(hipStream_t s, const DeviceStore& st, TrunkTimer& timer, bool timing, const WideTrunk& t) {
    if (t.stem_c == 128) forward_trunk_wide_sc<128>(s, st, timer, timing, t); else forward_trunk_wide_sc<256>(s, st, timer, timing, t);
}

}  // namespace gaz
