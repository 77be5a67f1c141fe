// The tile loop of the Checkers networks on the exact-f32 matrix instruction: every layer of the Checkers actor (actor_checkers.hip), of
// the Checkers critics (critic_checkers.hip) and of the Checkers QMIX mixer (mixer.hip) is gemm_tiles over packed per-lane B tiles
// [col tile][k group][lane][4]; toeplitz (below) is the matrix form of their grid and window convolutions, for the pack kernels.
#pragma once
#include "actor_common.h"

namespace cm3 {

// ---- the tile loop -----------------------------------------------------------------------------------------------------
// acc[t][c] += A[16 (rt0 + t) .. +16][0 .. 16 KG) x B[.., 16 (ct0 + c) .. +16].  A: LDS, row stride lda floats;
// Bp: packed tiles of this layer.  B operands of group g + 1 are requested before the MFMAs of group g issue; those of
// group 0 (b0) are requested by the caller with load_b0 BEFORE the previous layer's epilogue and barrier, so that their
// L2 latency hides behind the LDS stores (1.5-3 k cycles per layer when it was exposed).
template <int CT, int KG>
__device__ __forceinline__ void load_b0(const float *Bp, int ct0, int lane, float4 (&b0)[CT]) {
#pragma unroll
  for (int c = 0; c < CT; ++c) b0[c] = (reinterpret_cast<const float4 *>(Bp) + ((size_t)(ct0 + c) * KG) * 64 + lane)[0];
}

template <int RT, int CT, int KG>
__device__ __forceinline__ void gemm_tiles(const float *A, int lda, int rt0, const float *Bp, int ct0, int lane,
                                           const float4 (&b0)[CT], f32x4 (&acc)[RT][CT]) {
  const int col = lane & 15, hi = lane >> 4;
  const float4 *bsrc[CT];
#pragma unroll
  for (int c = 0; c < CT; ++c) bsrc[c] = reinterpret_cast<const float4 *>(Bp) + ((size_t)(ct0 + c) * KG) * 64 + lane;
  const float *arow[RT];
#pragma unroll
  for (int t = 0; t < RT; ++t) arow[t] = A + (16 * (rt0 + t) + col) * lda + 4 * hi;
  float4 bcur[CT], bnext[CT];
#pragma unroll
  for (int c = 0; c < CT; ++c) bcur[c] = b0[c];
#pragma unroll
  for (int g = 0; g < KG; ++g) {
    if (g + 1 < KG) {
#pragma unroll
      for (int c = 0; c < CT; ++c) bnext[c] = bsrc[c][(g + 1) * 64];
    }
    float4 a[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t) a[t] = *reinterpret_cast<const float4 *>(arow[t] + 16 * g);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int t = 0; t < RT; ++t) {
        const float av = j == 0 ? a[t].x : (j == 1 ? a[t].y : (j == 2 ? a[t].z : a[t].w));
#pragma unroll
        for (int c = 0; c < CT; ++c) {
          const float bv = j == 0 ? bcur[c].x : (j == 1 ? bcur[c].y : (j == 2 ? bcur[c].z : bcur[c].w));
          acc[t][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[t][c], 0, 0, 0);
        }
      }
    }
    if (g + 1 < KG) {
#pragma unroll
      for (int c = 0; c < CT; ++c) bcur[c] = bnext[c];
    }
  }
}

template <int RT, int CT> __device__ __forceinline__ void zero_tiles(f32x4 (&acc)[RT][CT]) {
#pragma unroll
  for (int t = 0; t < RT; ++t)
#pragma unroll
    for (int c = 0; c < CT; ++c) acc[t][c] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
}

// this lane's bias values (column l & 15 of each column tile); requested before the layer's MFMAs so that the epilogue
// does not wait for them
template <int CT> __device__ __forceinline__ void load_bias(const float *bias, int ct0, int lane, float (&b)[CT]) {
#pragma unroll
  for (int c = 0; c < CT; ++c) b[c] = bias[16 * (ct0 + c) + (lane & 15)];
}

// O[row][col] = relu(acc + bias[col]); C layout: col = l & 15, row = 4 (l >> 4) + reg
template <int RT, int CT>
__device__ __forceinline__ void store_relu(float *O, int ldo, int rt0, int ct0, const float (&bias)[CT], int lane,
                                           const f32x4 (&acc)[RT][CT]) {
  const int col = lane & 15, hi = lane >> 4;
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    const float b = bias[c];
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg)
        O[(16 * (rt0 + t) + 4 * hi + reg) * ldo + 16 * (ct0 + c) + col] = fmaxf(acc[t][c][reg] + b, 0.0f);
  }
}

// element (k, n) of a SAME convolution [H][W][C] -> [H][W][F] with a [KH][KW][C][F] kernel as a matrix over the NHWC flattenings
template <int H, int W, int C, int F, int KH, int KW>
__device__ __forceinline__ float toeplitz(const float *wt, int k, int n) {
  if (k >= H * W * C || n >= H * W * F) return 0.0f;
  const int pin = k / C, ch = k - C * pin, r = pin / W, c = pin - W * r;
  const int pout = n / F, f = n - F * pout, ro = pout / W, co = pout - W * ro;
  const int dr = r - ro + KH / 2, dc = c - co + KW / 2;       // out[ro][co] += x[ro + dr - KH/2][co + dc - KW/2] w[dr][dc]
  if (dr < 0 || dr >= KH || dc < 0 || dc >= KW) return 0.0f;
  return wt[((dr * KW + dc) * C + ch) * F + f];
}

}  // namespace cm3
