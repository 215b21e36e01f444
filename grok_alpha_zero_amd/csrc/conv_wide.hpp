// conv_wide.hpp — the trunk and head convolutions of networks whose residual width F is not 128 (F in {64, 192, 256}):
// 3x3 F -> F and 128 | 256 -> F, the block-0 1x1 projection 128 | 256 -> F accumulated into conv2, and the heads' first
// convolution F -> 32.  The 128-wide networks keep their own kernels (resblock.hpp, trunk.hpp); nothing here is
// reached at F = 128.
//
// A 3x3 "same" convolution on NHWC bf16 board tensors as an implicit GEMM on the gfx950 matrix cores (v_mfma_f32_32x32x16_bf16,
// bf16 operands, fp32 accumulate); it replaces the Conv2D layers of the reference network (Net/ResNet/ResNet_Block.py:12-20,
// Connect4/Build_Model.py:41,62) as executed by ONNX Runtime.  GEMM view: M = B*H*W flattened board cells, N = Cout,
// K = taps * Cin.  A 256-thread workgroup owns BM = 128 consecutive cells x BN output channels (blockIdx.y = the BN-wide
// column tile of Cout):
//   * the 128 rows plus a (W+1)-row halo of the activation are brought into LDS ONCE by LDS-DMA (global_load_lds_dwordx4) and
//     serve all nine taps: the tap (dy,dx) operand of cell r is image row r + dy*W + dx; masked taps (board edges, rows past M)
//     read a zero row instead of being zeroed in registers, so the rows of neighbouring boards that the halo drags in are never
//     selected and nothing needs to be zero-filled;
//   * the image is XOR-swizzled in 16-byte slots by permuting the per-lane SOURCE address of the DMA (the LDS side of a DMA is
//     lane-linear), which makes every A-fragment ds_read_b128 conflict-free (LDS swizzle, below);
//   * the weights are arranged on the host in fragment order [column tile][tap][Cin/16][2][BN][8] (arrange_wide_weights; k =
//     k-step * 16 + half * 8 + j), so each workgroup's stream is one contiguous array cut into 9 * KSPLIT slices, its DMA is a
//     straight copy and every fragment read is base + compile-time offset; the slices are double-buffered in LDS: slice s+1 is
//     DMA'd while slice s multiplies, one barrier per slice; fragments are register double-buffered across k-steps;
//   * an optional second operand (CIN2 > 0: the 1x1 projection of block 0) is staged after the first and accumulates into the
//     SAME fp32 accumulators, so conv2 + projection take one bias (b2 + bp) and one rounding;
//   * epilogue: accumulators -> fp32 LDS tile -> per-thread 16-byte channel groups (dwordx4
//     stores): folded BN scale / shift, residual add, activation, and (for the pre-activation blocks) the second output
//     relu(bn_next(x)) — taken from the bf16-ROUNDED x, the value the next block reads (net.py forward_engine_numerics).  EPI_HEADS
//     instead writes the Connect4 heads' fp32 features: channels 0-7 policy, 8-15 value, flat BN over (cell * 8 + c), ReLU.
//
// LDS swizzle.  ds_read_b128 serves a wave in four 16-lane groups (MI355X_MICROARCH.md §LDS); a group is conflict-free iff its
// 16 lanes hit the 16 distinct 16-byte slots of one 256-byte bank row.  The A-fragment read of a group is 16 rows with distinct
// residues mod 16 at one logical slot s.  A row of SLOTS 16-byte slots starts at bank-row slot (row * SLOTS) mod 16:
//   SLOTS = 16, 32 (Cin 128, 256): every row starts at slot 0 -> store slot s at s ^ (row & 15);
//   SLOTS = 8, 24  (Cin 64, 192):  rows alternate between offsets 0 and 8 -> store slot s at s ^ ((row >> 1) & 7): bit 3 of the
//                                  bank-row slot comes from row & 1, bits 0-2 from (row >> 1) & 7, a bijection of row mod 16.
// The XOR never leaves the aligned group of 8 (16) slots, so it stays inside the row for every width.  tests/test_net_widths.py
// checks all four widths against the bank rule.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "conv_common.hpp"

namespace gaz {

enum { CW_EPI_BF16 = 0, CW_EPI_HEADS = 1 };

struct WideConvArgs {
    const bf16_t* in;  const bf16_t* wgt;    // [M][CIN] rows; [COUT / BN][NTAPS][CIN/16][2][BN][8]
    const bf16_t* in2; const bf16_t* wgt2;   // CIN2 > 0: [M][CIN2] rows; [COUT / BN][CIN2/16][2][BN][8] (1x1, same accumulator)
    const float* scaleA; const float* shiftA;    // [COUT] or null (= 1 / 0)
    const bf16_t* res;                        // [M][COUT] residual or null (may alias out1)
    bf16_t* out1; int act1;                   // [M][COUT]: act1(acc * scaleA + shiftA + res)
    const float* scaleB; const float* shiftB; bf16_t* out2;     // [M][COUT]: relu(bf16(out1) * scaleB + shiftB); out2 null = none
    float* feat_p; float* feat_v;             // CW_EPI_HEADS: [M][8] each, relu((acc + shiftA) * fs + ft) with fs / ft over cell * 8 + c
    const float* p_fs; const float* p_ft; const float* v_fs; const float* v_ft;
    int M, H, W;
};

template <int SLOTS> __device__ __forceinline__ int cw_swz(int row) {
    static_assert(SLOTS == 8 || SLOTS == 16 || SLOTS == 24 || SLOTS == 32, "Cin in {64, 128, 192, 256}");
    return SLOTS % 16 == 0 ? (row & 15) : ((row >> 1) & 7);
}

// weight slices per tap: at most 16 KB each (two are resident), dividing the Cin / 16 k-steps evenly
template <int CIN, int BN> constexpr int cw_ksplit() {
    int k = BN * CIN / 8192;
    if (k < 1) k = 1;
    while ((CIN / 16) % k) --k;
    return k;
}
template <int CIN, int BN, int BM, int KSPLIT> constexpr size_t cw_phase_bytes() {
    return (size_t)((BM + 2 * CONV_HALO_MAX + 1) * (CIN / 8) + 2 * BN * (CIN / 8) / KSPLIT) * 16;
}
constexpr size_t cw_max(size_t a, size_t b) { return a > b ? a : b; }
template <int CIN, int BN, int BM, int KSPLIT, int CIN2, int KSPLIT2> constexpr size_t conv_wide_lds_bytes() {
    return cw_max(cw_max(cw_phase_bytes<CIN, BN, BM, KSPLIT>(), CIN2 > 0 ? cw_phase_bytes<CIN2, BN, BM, KSPLIT2>() : 0), (size_t)BM * (BN + 4) * 4);
}

// One operand: stage the image (+ halo), stream the NTAPS * KSPLIT weight slices, accumulate into acc.  Ends on a barrier: the
// LDS is free again when it returns.
template <int CIN, int BN, int BM, int WN, int TM, int TN, int KSPLIT, int NTAPS, int THREADS>
__device__ __forceinline__ void cw_phase(f32x16 (&acc)[TM][TN], uint4* lds, const bf16_t* in, const bf16_t* wgt, long m0, int M, int H, int W) {
    constexpr int SLOTS = CIN / 8, AROWS = BM + 2 * CONV_HALO_MAX + 1, ZROW = AROWS - 1;
    constexpr int KSS = CIN / 16 / KSPLIT, BSL = BN * SLOTS / KSPLIT;
    static_assert((CIN / 16) % KSPLIT == 0 && BSL % 64 == 0, "slice shape");
    static_assert(NTAPS == 9 || NTAPS == 1, "3x3 or 1x1 (centre tap only)");
    uint4* As = lds;
    uint4* Bs = lds + AROWS * SLOTS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN, l31 = lane & 31, lhi = lane >> 5;
    const int halo = NTAPS == 9 ? W + 1 : 0, HW = H * W;
    const uint4* in4 = reinterpret_cast<const uint4*>(in);
    const uint4* w4 = reinterpret_cast<const uint4*>(wgt);

    // image rows [m0 - halo, m0 + BM + halo): (BM + 2 halo) * SLOTS is a multiple of 64 (halo W + 1 = 8 | 16)
    const int n_aslots = (BM + 2 * halo) * SLOTS;
    for (int base = wave * 64; base < n_aslots; base += THREADS) {
        const int i = base + lane, lr = i / SLOTS, sp = i % SLOTS;
        long gr = m0 - halo + lr;
        gr = gr < 0 ? 0 : (gr >= M ? (long)M - 1 : gr);        // rows outside the tensor are never selected
        __builtin_amdgcn_global_load_lds((const void*)(in4 + gr * SLOTS + (sp ^ cw_swz<SLOTS>(lr))), (lds_ptr_t)(As + base), 16, 0, 0);
    }
    if (tid < SLOTS) As[ZROW * SLOTS + tid] = make_uint4(0, 0, 0, 0);
    for (int base = wave * 64; base < BSL; base += THREADS)
        __builtin_amdgcn_global_load_lds((const void*)(w4 + base + lane), (lds_ptr_t)(Bs + base), 16, 0, 0);

    int lrow[TM]; unsigned vmask[TM];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) {
        lrow[tm] = (wm * TM + tm) * 32 + l31;
        const long gr = m0 + lrow[tm];
        const int cell = (int)((unsigned)gr % (unsigned)HW), y = cell / W, x = cell % W;
        unsigned m = 0;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int dy = t / 3 - 1, dx = t % 3 - 1;
            const bool ok = gr < M && (unsigned)(y + dy) < (unsigned)H && (unsigned)(x + dx) < (unsigned)W;
            m |= (ok ? 1u : 0u) << t;
        }
        vmask[tm] = m;
    }
    int bbase[TN];
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) bbase[tn] = lhi * BN + (wn * TN + tn) * 32 + l31;

    __syncthreads();                                // image + slice 0 have landed

    for (int sl = 0; sl < NTAPS * KSPLIT; ++sl) {
        const int tap = NTAPS == 9 ? sl / KSPLIT : 4, ks0 = (sl % KSPLIT) * KSS;
        const uint4* Bc = Bs + (sl & 1) * BSL;
        if (sl + 1 < NTAPS * KSPLIT) {
            uint4* Bn = Bs + ((sl + 1) & 1) * BSL;
            const uint4* wsrc = w4 + (size_t)(sl + 1) * BSL;
            for (int base = wave * 64; base < BSL; base += THREADS)
                __builtin_amdgcn_global_load_lds((const void*)(wsrc + base + lane), (lds_ptr_t)(Bn + base), 16, 0, 0);
        }
        const int off = NTAPS == 9 ? (tap / 3 - 1) * W + (tap % 3 - 1) : 0;
        int abase[TM], axor[TM];
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) {
            const bool ok = (vmask[tm] >> tap) & 1u;
            const int ar = ok ? lrow[tm] + halo + off : ZROW;
            abase[tm] = ar * SLOTS; axor[tm] = cw_swz<SLOTS>(ar);
        }
        uint4 afr[2][TM], bfr[2][TN];
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) afr[0][tm] = As[abase[tm] + ((ks0 * 2 + lhi) ^ axor[tm])];
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) bfr[0][tn] = Bc[bbase[tn]];
#pragma unroll
        for (int ks = 0; ks < KSS; ++ks) {
            const int cur = ks & 1, nxt = cur ^ 1;
            if (ks + 1 < KSS) {
#pragma unroll
                for (int tm = 0; tm < TM; ++tm) afr[nxt][tm] = As[abase[tm] + (((ks0 + ks + 1) * 2 + lhi) ^ axor[tm])];
#pragma unroll
                for (int tn = 0; tn < TN; ++tn) bfr[nxt][tn] = Bc[bbase[tn] + (ks + 1) * 2 * BN];
            }
#pragma unroll
            for (int tm = 0; tm < TM; ++tm) {
                const bf16x8 af = *reinterpret_cast<bf16x8*>(&afr[cur][tm]);
#pragma unroll
                for (int tn = 0; tn < TN; ++tn)
                    acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, *reinterpret_cast<bf16x8*>(&bfr[cur][tn]), acc[tm][tn], 0, 0, 0);
            }
        }
        __syncthreads();                            // slice sl+1 landed; everyone is done reading slice sl (and, after the last, the image)
    }
}

// BM = WM * TM * 32 cells x BN = WN * TN * 32 channels per workgroup; OCC = workgroups per CU the LDS allows.
template <int CIN, int BN, int WM, int WN, int TM, int TN, int KSPLIT, int NTAPS, int CIN2, int KSPLIT2, int EPI, int OCC>
__global__ __launch_bounds__(WM * WN * 64, (WM * WN * OCC + 3) / 4) void k_conv_wide(WideConvArgs a) {
    constexpr int BM = WM * TM * 32, THREADS = WM * WN * 64;
    static_assert(WN * TN * 32 == BN, "tile shape");
    extern __shared__ uint4 lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN, l31 = lane & 31, lhi = lane >> 5;
    const long m0 = (long)blockIdx.x * BM;
    const int n0 = (int)blockIdx.y * BN, COUT = (int)gridDim.y * BN;

    f32x16 acc[TM][TN];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[tm][tn][r] = 0.0f;
    cw_phase<CIN, BN, BM, WN, TM, TN, KSPLIT, NTAPS, THREADS>(acc, lds, a.in, a.wgt + (size_t)blockIdx.y * NTAPS * CIN * BN, m0, a.M, a.H, a.W);
    if constexpr (CIN2 > 0)
        cw_phase<CIN2, BN, BM, WN, TM, TN, KSPLIT2, 1, THREADS>(acc, lds, a.in2, a.wgt2 + (size_t)blockIdx.y * CIN2 * BN, m0, a.M, a.H, a.W);

    // C/D layout of the 32x32 MFMA: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
    constexpr int CT = BN + 4;
    float* Ct = reinterpret_cast<float*>(lds);      // [BM][BN + 4] fp32 over the idle image + slices
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) {
            const int col = (wn * TN + tn) * 32 + l31;
            const float sA = a.scaleA ? a.scaleA[n0 + col] : 1.0f, tA = a.shiftA ? a.shiftA[n0 + col] : 0.0f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (wm * TM + tm) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
                Ct[row * CT + col] = acc[tm][tn][r] * sA + tA;
            }
        }
    __syncthreads();
    if constexpr (EPI == CW_EPI_HEADS) {            // 16 real channels of the 32: policy 0-7, value 8-15
        static_assert(BN == 32, "heads tile");
        const int HW = a.H * a.W;
        for (int i = tid; i < BM * 16; i += THREADS) {
            const int row = i >> 4, c = i & 15;
            const long gr = m0 + row;
            if (gr >= a.M) break;
            const int cell = (int)(gr % HW), f = cell * 8 + (c & 7);
            const float v = Ct[row * CT + c];
            if (c < 8) a.feat_p[gr * 8 + c] = fmaxf(v * a.p_fs[f] + a.p_ft[f], 0.0f);
            else a.feat_v[gr * 8 + c - 8] = fmaxf(v * a.v_fs[f] + a.v_ft[f], 0.0f);
        }
    } else {
        constexpr int CHUNKS = BN / 8;              // 16-byte (8 x bf16) groups per row
        static_assert(THREADS % CHUNKS == 0, "epilogue rows");
        const int chunk = tid % CHUNKS, r0 = tid / CHUNKS, c0 = n0 + chunk * 8;
        float sB[8], tB[8];
        if (a.out2) {
#pragma unroll
            for (int j = 0; j < 8; ++j) { sB[j] = a.scaleB[c0 + j]; tB[j] = a.shiftB[c0 + j]; }
        }
        for (int row = r0; row < BM; row += THREADS / CHUNKS) {
            const long gr = m0 + row;
            if (gr >= a.M) break;
            const float4 q0 = *reinterpret_cast<const float4*>(&Ct[row * CT + chunk * 8]);
            const float4 q1 = *reinterpret_cast<const float4*>(&Ct[row * CT + chunk * 8 + 4]);
            float v[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
            const size_t o = (size_t)gr * COUT + c0;
            if (a.res) {
                const uint4 rv = *reinterpret_cast<const uint4*>(a.res + o);
                const unsigned rw[4] = {rv.x, rv.y, rv.z, rv.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    v[2 * j] += __uint_as_float(rw[j] << 16);
                    v[2 * j + 1] += __uint_as_float(rw[j] & 0xFFFF0000u);
                }
            }
            if (a.act1 == ACT_RELU) {
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = fmaxf(v[j], 0.0f);
            }
            const unsigned pk[4] = {pack_bf16(v[0], v[1]), pack_bf16(v[2], v[3]), pack_bf16(v[4], v[5]), pack_bf16(v[6], v[7])};
            *reinterpret_cast<uint4*>(a.out1 + o) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
            if (a.out2) {
                float w[8];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    w[2 * j] = fmaxf(__uint_as_float(pk[j] << 16) * sB[2 * j] + tB[2 * j], 0.0f);
                    w[2 * j + 1] = fmaxf(__uint_as_float(pk[j] & 0xFFFF0000u) * sB[2 * j + 1] + tB[2 * j + 1], 0.0f);
                }
                *reinterpret_cast<uint4*>(a.out2 + o) =
                    make_uint4(pack_bf16(w[0], w[1]), pack_bf16(w[2], w[3]), pack_bf16(w[4], w[5]), pack_bf16(w[6], w[7]));
            }
        }
    }
}

// Column tile per output width: 32 (heads: 4 waves x 32 rows), 64 (F = 64, and F = 192 as three tiles), 128 (F = 256, two tiles)
template <int COUT> struct CwTile;
template <> struct CwTile<32>  { enum { BN = 32, WM = 4, WN = 1, TM = 1, TN = 1 }; };
template <> struct CwTile<64>  { enum { BN = 64, WM = 2, WN = 2, TM = 2, TN = 1 }; };
template <> struct CwTile<192> { enum { BN = 64, WM = 2, WN = 2, TM = 2, TN = 1 }; };
template <> struct CwTile<256> { enum { BN = 128, WM = 2, WN = 2, TM = 2, TN = 2 }; };
constexpr int CW_BM = 128;
inline int conv_wide_bn(int cout) { return cout == 32 ? 32 : (cout == 256 ? 128 : 64); }

// Host launch of one convolution CIN -> COUT (NTAPS = 9 | 1), with the projection operand when CIN2 > 0.
template <int CIN, int COUT, int NTAPS, int CIN2, int EPI>
inline void conv_wide_launch(hipStream_t s, const WideConvArgs& a) {
    typedef CwTile<COUT> T;
    constexpr int KS1 = cw_ksplit<CIN, T::BN>(), KS2 = CIN2 > 0 ? cw_ksplit<(CIN2 > 0 ? CIN2 : 16), T::BN>() : 1;
    constexpr int BM = T::WM * T::TM * 32;
    static_assert(BM == CW_BM, "row tile");
    constexpr size_t lds = conv_wide_lds_bytes<CIN, T::BN, BM, KS1, CIN2, KS2>();
    static_assert(lds <= 160 * 1024, "LDS budget");
    constexpr int OCC = (int)((160 * 1024) / lds) < 2 ? 1 : 2;
    const void* k = (const void*)(k_conv_wide<CIN, T::BN, T::WM, T::WN, T::TM, T::TN, KS1, NTAPS, CIN2, KS2, EPI, OCC>);
    if (lds > 64 * 1024) {                          // dynamic LDS above 64 KB needs the attribute, once per device
        static unsigned long long done = 0;
        int dev = 0; hipGetDevice(&dev);
        if (dev >= 64 || !(__atomic_load_n(&done, __ATOMIC_ACQUIRE) >> dev & 1ull)) {
            hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (dev < 64) __atomic_fetch_or(&done, 1ull << dev, __ATOMIC_RELEASE);
        }
    }
    hipLaunchKernelGGL((k_conv_wide<CIN, T::BN, T::WM, T::WN, T::TM, T::TN, KS1, NTAPS, CIN2, KS2, EPI, OCC>),
                       dim3((a.M + BM - 1) / BM, COUT / T::BN), dim3(T::WM * T::WN * 64), lds, s, a);
}

// Host: [ntaps][cout][cin] (export order) -> [cout / bn][ntaps][cin / 16][2][bn][8] (column tile, then MFMA B-fragment order).
inline void arrange_wide_weights(const float* src, int cout, int cin, int ntaps, bf16_t* dst, bf16_t (*cvt)(float)) {
    const int bn = conv_wide_bn(cout);
    for (int nt = 0; nt < cout / bn; ++nt)
        for (int tap = 0; tap < ntaps; ++tap)
            for (int n = 0; n < bn; ++n)
                for (int k = 0; k < cin; ++k) {
                    const int ks = k / 16, half = (k % 16) / 8, j = k % 8;
                    dst[(((((size_t)nt * ntaps + tap) * (cin / 16) + ks) * 2 + half) * bn + n) * 8 + j] =
                        cvt(src[((size_t)tap * cout + nt * bn + n) * cin + k]);
                }
}

}  // namespace gaz
