// The dense chain's row-tile product and its dX = dY W fragment, shared by the chain
// kernels (gine_chain.hip) and the DeepSet backward that runs the chain's backward tile in
// its own launch (gine_deepset.hip: k_deepset_bwd_chain).  One definition, so both compute
// a tile with the same instructions in the same k order -- the same bits.
#pragma once

#include "gine_common.hpp"

namespace gine {

typedef float chr_floatx16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ chr_floatx16 chr_zero16() {
  chr_floatx16 v;
#pragma unroll
  for (int i = 0; i < 16; ++i) v[i] = 0.f;
  return v;
}

// acc = A[32 x K] (LDS rows, stride lda) x B-fragments (K/2 per lane half)
template <int K>
__device__ __forceinline__ chr_floatx16 tile_mma(const float* sA, int lda,
                                                 const float (&bf)[K / 2], int c32, int h) {
  constexpr int KS = K / 2;
  chr_floatx16 acc = chr_zero16();
  const float* arow = sA + c32 * lda + h * KS;
#pragma unroll
  for (int q = 0; q < KS / 4; ++q) {
    const float4 a4 = *reinterpret_cast<const float4*>(&arow[4 * q]);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, bf[4 * q], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, bf[4 * q + 1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, bf[4 * q + 2], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, bf[4 * q + 3], acc, 0, 0, 0);
  }
  return acc;
}

// dX = dY W fragment: bf[s] = W[h*KS + s][coff + col]
template <int K>
__device__ __forceinline__ void frag_n(float (&bf)[K / 2], const float* W, int ldw, int coff,
                                       int col, int h) {
  constexpr int KS = K / 2;
#pragma unroll
  for (int s = 0; s < KS; ++s) bf[s] = W[(size_t)(h * KS + s) * ldw + coff + col];
}

}  // namespace gine
