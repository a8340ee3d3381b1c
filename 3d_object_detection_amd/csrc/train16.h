// The bf16 operand helpers of the mixed-precision backwards (block_train16.hip, down_train16.hip, neck_train16.hip): packing and
// splitting fp32 values into bf16 fragments, the bf16 MFMA, the funnel shift of a fragment by one element, and the weight image of the
// 3 x 3 dgrads (k_conv3_wt16: the unit's with cin = cout = C, and the strided stage's).
#pragma once
#include "pp_common.h"
#include "train_host.h" // f32x4

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned pk_bf16(float a, float b) // v_cvt_pk_bf16_f32 (round to nearest even), a in the low half
{
    return __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2){a, b}, bf16x2));
}
// the residual the lo image rounds: x - bf16(x), one fp32 subtraction (exact for finite x)
__device__ __forceinline__ float bf16_rest(float x) { return x - __uint_as_float(pk_bf16(x, 0.f) << 16); }
__device__ __forceinline__ u32x4 pk8(const float* v) { return u32x4{pk_bf16(v[0], v[1]), pk_bf16(v[2], v[3]), pk_bf16(v[4], v[5]), pk_bf16(v[6], v[7])}; }
__device__ __forceinline__ u32x4 pk8_rest(const float* v)
{
    float r[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) r[e] = bf16_rest(v[e]);
    return pk8(r);
}
__device__ __forceinline__ f32x4 mfma16(const u32x4 a, const u32x4 b, const f32x4 c)
{
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// wT16[part][t][ci][co] = bf16 parts of w[co][ci][t]: the A operand of k_unit_dgrad16 and k_down_dgrad16, 8 consecutive co per lane
template <bool X3>
__global__ void __launch_bounds__(256) k_conv3_wt16(const float* __restrict__ w, uint16_t* __restrict__ wT, int cin, int cout)
{
    const int i = blockIdx.x * 256 + threadIdx.x; // index into wT [9][cin][cout]
    if (i >= 9 * cin * cout) return;
    const int co = i % cout, ci = (i / cout) % cin, t = i / (cin * cout);
    const float v = w[((size_t)co * cin + ci) * 9 + t];
    wT[i] = (uint16_t)pk_bf16(v, 0.f);
    if (X3) wT[(size_t)9 * cin * cout + i] = (uint16_t)pk_bf16(bf16_rest(v), 0.f);
}

// eight consecutive bf16 elements starting one element before (kx = 0) or behind (kx = 2) an aligned 16-byte group d: e is the dword
// before / behind d, and the five dwords are shifted by 16 bits in registers (v_alignbit_b32); kx = 1 is d itself
__device__ __forceinline__ u32x4 shift_frag(const u32x4 d, const unsigned e, const int kx)
{
    const bool left = kx == 0; // elements P - 1 .. P + 6: e, d0 .. d3; kx = 2: P + 1 .. P + 8: d0 .. d3, e; kx = 1: d
    const unsigned s0 = left ? e : d[0], s1 = left ? d[0] : d[1], s2 = left ? d[1] : d[2], s3 = left ? d[2] : d[3], s4 = left ? d[3] : e;
    const unsigned sh = kx == 1 ? 0u : 16u;
    return u32x4{__builtin_amdgcn_alignbit(s1, s0, sh), __builtin_amdgcn_alignbit(s2, s1, sh), __builtin_amdgcn_alignbit(s3, s2, sh),
                 __builtin_amdgcn_alignbit(s4, s3, sh)};
}

} // namespace
