// cm3_episode_route_plan: the routing plan of DeviceDualReplayBuffer.add_rollout (whole episodes into the two rings of
// replay_buffer_dual.py:13-37, their unfinished tails into a pending store) in FIVE fixed-shape launches, nothing read by the host:
//   k_route_lengths       walk 1 of episode_route.h, a lane per env
//   k_route_partials      the sum of every workgroup's 1024 cells
//   k_route_scan_partials ONE workgroup: exclusive scan of those sums, the totals (counts)
//   k_route_apply         every workgroup scans its own 1024 cells on top of its partial: the first rank of every episode
//   k_route_rows          walk 2, a lane per env
// No workgroup waits for another inside a launch and nothing is accumulated with atomics: the sums are integers (both classes in one
// 64-bit word), so the result does not depend on any order.  The arithmetic is episode_route.h's, shared with the host function.
#include <new>

#include "common.h"
#include "episode_route.h"

namespace cm3 {

__global__ void __launch_bounds__(64) k_route_lengths(const RouteShape s, const int32_t *pend_in, int32_t *pend_out, uint64_t *len) {
  const int e = (int)(blockIdx.x * 64 + threadIdx.x);
  if (e >= s.E) return;
  const int p = route_walk_lengths(s, e, s.sync ? 0 : pend_in[e], len);
  if (!s.sync) pend_out[e] = p;
}

__global__ void __launch_bounds__(64) k_route_rows(const RouteShape s, const uint64_t *len, const uint64_t *first, const int64_t *counts,
                                                   const int32_t *pend_new, uint8_t *sel, int64_t *row, int64_t *flush_row) {
  const int e = (int)(blockIdx.x * 64 + threadIdx.x);
  if (e >= s.E) return;
  const int64_t n[2] = {counts[0], counts[1]};
  route_walk_rows(s, e, len, first, n, s.sync ? 0 : pend_new[e], sel, row, flush_row);
}

// the four cells of a lane (cells past the end count 0) and their sum
__device__ __forceinline__ uint64_t route_cells(const uint64_t *len, size_t cells, uint64_t (&w)[4]) {
  const size_t c0 = (size_t)blockIdx.x * kRouteScanCells + (size_t)threadIdx.x * 4;
#pragma unroll
  for (int j = 0; j < 4; ++j) w[j] = c0 + j < cells ? len[c0 + j] : 0;
  return w[0] + w[1] + w[2] + w[3];
}

// inclusive scan over the 256 lanes of a workgroup
__device__ __forceinline__ uint64_t route_block_scan(uint64_t v, uint64_t *sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int off = 1; off < 256; off <<= 1) {
    const uint64_t add = threadIdx.x >= (unsigned)off ? sh[threadIdx.x - off] : 0;
    __syncthreads();
    sh[threadIdx.x] += add;
    __syncthreads();
  }
  return sh[threadIdx.x];
}

__global__ void __launch_bounds__(256) k_route_partials(const uint64_t *len, size_t cells, uint64_t *partial) {
  __shared__ uint64_t sh[256];
  uint64_t w[4];
  const uint64_t incl = route_block_scan(route_cells(len, cells, w), sh);
  if (threadIdx.x == 255) partial[blockIdx.x] = incl;
}

__global__ void __launch_bounds__(256) k_route_scan_partials(uint64_t *partial, size_t nb, int64_t *counts) {
  __shared__ uint64_t sh[256];
  const size_t seg = (nb + 255) / 256, lo = threadIdx.x * seg < nb ? threadIdx.x * seg : nb, hi = lo + seg < nb ? lo + seg : nb;
  uint64_t sum = 0;
  for (size_t b = lo; b < hi; ++b) sum += partial[b];
  const uint64_t incl = route_block_scan(sum, sh);
  uint64_t run = incl - sum;
  for (size_t b = lo; b < hi; ++b) {
    const uint64_t v = partial[b];
    partial[b] = run;
    run += v;
  }
  if (threadIdx.x == 255) {
    counts[0] = route_half(incl, kRouteBad);
    counts[1] = route_half(incl, kRouteGood);
  }
}

__global__ void __launch_bounds__(256) k_route_apply(const uint64_t *len, size_t cells, const uint64_t *partial, uint64_t *first) {
  __shared__ uint64_t sh[256];
  uint64_t w[4];
  const uint64_t sum = route_cells(len, cells, w);
  uint64_t run = partial[blockIdx.x] + route_block_scan(sum, sh) - sum;
  const size_t c0 = (size_t)blockIdx.x * kRouteScanCells + (size_t)threadIdx.x * 4;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (c0 + j < cells) first[c0 + j] = run;
    run += w[j];
  }
}

static int route_shape(const cm3_episode_route_desc *d, RouteShape &s) {
  CM3_REQUIRE(d, "episode_route: null desc");
  CM3_REQUIRE(route_shape_fits(d->n_ticks, d->n_envs, d->pending_depth),
              "episode_route: n_ticks and n_envs must be >= 1, pending_depth >= 0, and (n_ticks + pending_depth) * n_envs below 2^31");
  CM3_REQUIRE(d->done && d->collisions, "episode_route: done and collisions are required");
  CM3_REQUIRE(d->done_stride >= (size_t)d->n_envs && d->collisions_stride >= (size_t)d->n_envs * 4 && d->collisions_stride % 4 == 0 &&
                  (!d->valid || d->valid_stride >= (size_t)d->n_envs),
              "episode_route: a tick stride is smaller than a tick's row");
  for (int c = 0; c < 2; ++c)
    CM3_REQUIRE(d->ring_size[c] >= 1 && d->ring_idx[c] >= 0 && d->ring_idx[c] < d->ring_size[c],
                "episode_route: ring %d: 0 <= ring_idx < ring_size is required", c);
  s.done = d->done; s.st_done = d->done_stride;
  s.coll = d->collisions; s.st_coll = d->collisions_stride;
  s.valid = d->valid; s.st_valid = d->valid_stride;
  s.T = d->n_ticks; s.E = d->n_envs; s.P = d->pending_depth;
  s.sync = d->synchronous ? 1 : 0;
  for (int c = 0; c < 2; ++c) { s.idx[c] = d->ring_idx[c]; s.maxsize[c] = d->ring_size[c]; }
  return CM3_OK;
}

static int route_outputs(const RouteShape &s, const int32_t *pend_in, const int32_t *pend_out, const uint8_t *sel, const int64_t *row,
                         const int64_t *flush_row, const int64_t *counts) {
  CM3_REQUIRE(sel && row && counts, "episode_route: sel, row and counts are required");
  CM3_REQUIRE(s.P == 0 || flush_row, "episode_route: flush_row is required with a pending store");
  CM3_REQUIRE(s.sync || (pend_in && pend_out), "episode_route: a continuous collection needs pend_len (in and out)");
  return CM3_OK;
}

}  // namespace cm3

extern "C" {
size_t cm3_episode_route_scratch_bytes(int32_t n_ticks, int32_t n_envs) {
  if (!cm3::route_shape_fits(n_ticks, n_envs, 0)) return 0;
  return cm3::route_scratch_words((size_t)n_ticks * (size_t)n_envs) * sizeof(uint64_t);
}

int cm3_episode_route_plan(const cm3_episode_route_desc *desc, const int32_t *pend_in, int32_t *pend_out, uint8_t *sel, int64_t *row,
                           int64_t *flush_row, int64_t *counts, void *scratch, size_t scratch_bytes, void *stream) {
  using namespace cm3;
  RouteShape s;
  if (int rc = route_shape(desc, s)) return rc;
  if (int rc = route_outputs(s, pend_in, pend_out, sel, row, flush_row, counts)) return rc;
  const size_t cells = (size_t)s.T * s.E, nb = route_scan_blocks(cells);
  CM3_REQUIRE(scratch && (uintptr_t)scratch % 8 == 0 && scratch_bytes >= route_scratch_words(cells) * sizeof(uint64_t),
              "episode_route: scratch must be 8-byte aligned and hold cm3_episode_route_scratch_bytes()");
  uint64_t *len = (uint64_t *)scratch, *first = len + cells, *partial = first + cells;
  const unsigned lanes = (unsigned)((s.E + 63) / 64);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_route_lengths, dim3(lanes), dim3(64), 0, st, s, pend_in, pend_out, len);
  hipLaunchKernelGGL(k_route_partials, dim3((unsigned)nb), dim3(256), 0, st, len, cells, partial);
  hipLaunchKernelGGL(k_route_scan_partials, dim3(1), dim3(256), 0, st, partial, nb, counts);
  hipLaunchKernelGGL(k_route_apply, dim3((unsigned)nb), dim3(256), 0, st, len, cells, partial, first);
  hipLaunchKernelGGL(k_route_rows, dim3(lanes), dim3(64), 0, st, s, len, first, counts, pend_out, sel, row, flush_row);
  CM3_HIP_CHECK(hipGetLastError());
  return CM3_OK;
}

int cm3_episode_route_plan_host(const cm3_episode_route_desc *desc, const int32_t *pend_in, int32_t *pend_out, uint8_t *sel, int64_t *row,
                                int64_t *flush_row, int64_t *counts) {
  using namespace cm3;
  RouteShape s;
  if (int rc = route_shape(desc, s)) return rc;
  if (int rc = route_outputs(s, pend_in, pend_out, sel, row, flush_row, counts)) return rc;
  uint64_t *scratch = new (std::nothrow) uint64_t[route_scratch_words((size_t)s.T * s.E)];
  CM3_REQUIRE(scratch, "episode_route: out of host memory");
  route_plan_host(s, pend_in, pend_out, sel, row, flush_row, counts, scratch);
  delete[] scratch;
  return CM3_OK;
}
}
