// conv_common.hpp — what the convolution kernels share (resblock.hpp, trunk.hpp, conv_wide.hpp, netops.hpp): the bf16 types and
// conversions, the activation codes, the halo bound of the LDS activation image, and the host-side arrangement of convolution
// weights into MFMA B-fragment order.  No kernel lives here; the implicit-GEMM scheme is described in conv_wide.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gaz {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef unsigned short bf16_t;

__device__ __forceinline__ float bf2f(bf16_t v) { return __uint_as_float((unsigned)v << 16); }
__device__ __forceinline__ bf16_t f2bf(float f) {
    unsigned u = __float_as_uint(f);
    return (bf16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

enum { ACT_NONE = 0, ACT_RELU = 1 };

constexpr int CONV_HALO_MAX = 16;           // W + 1 <= 16

typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
__device__ __forceinline__ unsigned pack_bf16(float a, float b) {     // v_cvt_pk_bf16_f32 (round to nearest even)
    bf16x2 v; v[0] = (__bf16)a; v[1] = (__bf16)b;
    return *reinterpret_cast<unsigned*>(&v);
}

typedef __attribute__((address_space(3))) void* lds_ptr_t;

// Host: [9][cout][cin] (export order) -> [9][cin/16][2][cout][8] (MFMA B-fragment order).
inline void arrange_conv_weights(const float* src, int cout, int cin, bf16_t* dst, bf16_t (*cvt)(float), int ntaps = 9) {
    for (int tap = 0; tap < ntaps; ++tap)
        for (int n = 0; n < cout; ++n)
            for (int k = 0; k < cin; ++k) {
                const int ks = k / 16, half = (k % 16) / 8, j = k % 8;
                dst[((((size_t)tap * (cin / 16) + ks) * 2 + half) * cout + n) * 8 + j] = cvt(src[((size_t)tap * cout + n) * cin + k]);
            }
}

}  // namespace gaz
