// What the QMIX learners (learner.hip: particle, learner_checkers.hip: Checkers) share: the X^T . Delta weight-gradient kernel per
// chunk of rows, the ascending-chunk reduce kernel that stores the gradients TF-shaped and sums the loss, and the 16-lane DPP sums of
// the mixers' trees.  Both kernels are generic over a table of NJ jobs; a unit instantiates them at the job count it needs.
#pragma once
#include "actor_common.h"

namespace cm3 {
namespace learner {

constexpr int kChunk = 256;     // rows per partial sum of a weight gradient

// moves inside a 16-lane DPP row: lane ^ 1, lane ^ 2, i <-> 7 - i inside each 8 lanes, i <-> 15 - i (mixer.hip's mix_sum16)
template <int CTRL> __device__ __forceinline__ float lrn_dpp(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
__device__ __forceinline__ float lrn_sum16(float v) {
  v = v + lrn_dpp<0xB1>(v);
  v = v + lrn_dpp<0x4E>(v);
  v = v + lrn_dpp<0x141>(v);
  v = v + lrn_dpp<0x140>(v);
  return v;
}
__device__ __forceinline__ float sign_f32(float x) { return x > 0.0f ? 1.0f : (x < 0.0f ? -1.0f : 0.0f); }

// ---- X^T . Delta per chunk of rows ------------------------------------------------------------------------------------------------
// One wave per 16 x 16 output tile and per CHUNK of 256 consecutive rows: A[i][k] = X[row k][16 kt + i], B[k][j] = Delta[row k][16 mt + j],
// one chain from zero over the chunk's rows in ascending order, four rows per instruction.  A bias gradient is one more row tile whose
// A operand is 1 in row 0: the same chain.  The chunk's tile goes to P.  No LDS.
struct XtdJob {
  const float *X, *D;
  float *P;                       // [chunks][(KT + 1) 16][16 MT]
  size_t rows;
  int ldx, Kx, KT, ldd, MT;
  unsigned block0, groups;        // the job's first workgroup; workgroups per chunk: ceil((KT + 1) MT / 4)
};
template <int NJ> struct XtdParams {
  XtdJob job[NJ];
};

template <int NJ> __global__ void CM3_MATRIX_KERNEL k_learner_xtd(const XtdParams<NJ> p) {
  const int tid = threadIdx.x, lane = tid & 63, col = lane & 15, hi = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  int j = 0;
#pragma unroll
  for (int i = 1; i < NJ; ++i) j = blockIdx.x >= p.job[i].block0 ? i : j;
  XtdJob J = p.job[0];
#pragma unroll
  for (int i = 1; i < NJ; ++i)
    if (j == i) J = p.job[i];
  const unsigned local = blockIdx.x - J.block0;
  const unsigned chunk = local / J.groups;
  const int tiles_k = J.KT + 1, tiles = tiles_k * J.MT;
  const int tile = (int)(local - chunk * J.groups) * 4 + w;
  if (tile >= tiles) return;
  const int kt = tile / J.MT, mt = tile - kt * J.MT;
  const bool ones = kt == J.KT;
  const int kx = 16 * kt + col, m = 16 * mt + col;
  const bool kx_ok = !ones && kx < J.Kx;
  const size_t r0 = (size_t)chunk * kChunk;
  const size_t r1 = r0 + kChunk < J.rows ? r0 + kChunk : J.rows;
  f32x4 acc = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  for (size_t r = r0; r < r1; r += 4) {
    const size_t rr = r + hi;
    const bool ok = rr < r1;
    const size_t rc = ok ? rr : r0;
    float av = kx_ok ? J.X[rc * J.ldx + kx] : ((ones && col == 0) ? 1.0f : 0.0f);
    float bv = J.D[rc * J.ldd + m];
    av = ok ? av : 0.0f;
    bv = ok ? bv : 0.0f;
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
  }
  float *out = J.P + ((size_t)chunk * tiles_k * 16 + 16 * kt + 4 * hi) * (size_t)(16 * J.MT) + m;
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) out[(size_t)reg * (16 * J.MT)] = acc[reg];
}

// ---- the chunks' sums, TF-shaped; the loss ----------------------------------------------------------------------------------------
// One thread per gradient element: the chunks' partial sums added in ascending chunk order, from the first, and stored TF-shaped.  The
// last workgroup sums err2: thread t the rows t, t + 256, ... in ascending order from zero, then the 256 partial sums by a halving tree
// in LDS (t with t + 128, then + 64, ...); loss = sum / B.
struct RedSeg {
  int col0, ncols;
  float *w, *b;                   // [Kx][ncols] (or NULL), [ncols] from the ones row (or NULL)
};
struct RedJob {
  const float *P;
  size_t chunks;
  int prow, pcol, Kx, ones_row, nseg;
  unsigned e0;                    // the job's first element in the launch's flat index
  RedSeg seg[5];
};
template <int NJ> struct RedParams {
  RedJob job[NJ];
  unsigned total;
  uint32_t B;
  const float *err2;
  float *loss;
};

template <int NJ> __global__ void __launch_bounds__(256) k_learner_reduce(const RedParams<NJ> p) {
  const int tid = threadIdx.x;
  if (blockIdx.x == gridDim.x - 1) {
    __shared__ float sh[256];
    float s = 0.0f;
    for (uint32_t b = tid; b < p.B; b += 256) s = s + p.err2[b];
    sh[tid] = s;
    __syncthreads();
    for (int stride = 128; stride > 0; stride >>= 1) {
      if (tid < stride) sh[tid] = sh[tid] + sh[tid + stride];
      __syncthreads();
    }
    if (tid == 0) p.loss[0] = sh[0] / (float)p.B;
    return;
  }
  const unsigned idx = blockIdx.x * 256u + tid;
  if (idx >= p.total) return;
  int j = 0;
#pragma unroll
  for (int i = 1; i < NJ; ++i) j = idx >= p.job[i].e0 ? i : j;
  const RedJob &J = p.job[j];
  const unsigned local = idx - J.e0;
  const int kk = (int)(local / (unsigned)J.pcol), m = (int)(local - (unsigned)kk * J.pcol);
  const bool is_ones = kk == J.ones_row;
  if (!(kk < J.Kx || is_ones)) return;
  float *dst = nullptr;
  for (int s = 0; s < J.nseg; ++s) {
    const RedSeg &g = J.seg[s];
    if (m >= g.col0 && m < g.col0 + g.ncols) dst = is_ones ? (g.b ? g.b + (m - g.col0) : nullptr) : (g.w ? g.w + (size_t)kk * g.ncols + (m - g.col0) : nullptr);
  }
  if (!dst) return;
  const size_t stride = (size_t)J.prow * J.pcol;
  const float *src = J.P + (size_t)kk * J.pcol + m;
  float s = src[0];
  for (size_t c = 1; c < J.chunks; ++c) s = s + src[c * stride];
  *dst = s;
}

// One job of both tables: X [rows][ldx] (Kx real columns), Delta [rows][ldd] (ldd a multiple of 16), P the chunks' partial tiles.
// blocks / elems run along as the launch's workgroup and element counts.
inline void learner_job(XtdJob &J, RedJob &Q, unsigned &blocks, unsigned &elems, const float *X, int ldx, int Kx, const float *D, int ldd,
                        size_t rows, size_t chunks, float *P) {
  J.X = X; J.D = D; J.P = P; J.rows = rows; J.ldx = ldx; J.Kx = Kx; J.KT = (Kx + 15) / 16; J.ldd = ldd; J.MT = ldd / 16;
  J.block0 = blocks;
  J.groups = (unsigned)(((J.KT + 1) * J.MT + 3) / 4);
  blocks += (unsigned)chunks * J.groups;
  Q.P = P; Q.chunks = chunks; Q.prow = (J.KT + 1) * 16; Q.pcol = ldd; Q.Kx = Kx; Q.ones_row = J.KT * 16; Q.e0 = elems;
  elems += (unsigned)(Q.prow * Q.pcol);
}
// floats of a job's partial tiles
inline size_t learner_partial_floats(size_t chunks, int Kx, int ldd) { return chunks * (size_t)(((Kx + 15) / 16 + 1) * 16) * (size_t)ldd; }

}  // namespace learner
}  // namespace cm3
