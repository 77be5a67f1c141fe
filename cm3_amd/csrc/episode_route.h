// Where every transition of a vectorised collection goes in the dual replay buffer (replay_buffer_dual.py:13-37 fed with WHOLE
// episodes, train_onpolicy.py:300-356): the arithmetic of cm3_episode_route_plan in one place.  Plain C++17, no HIP: the kernels of
// episode_route.hip call these functions per lane, route_plan_host() calls them in sequence and produces the same outputs, and
// tests/test_episode_route_plan.py compiles this header alone and walks it on a machine without a GPU.
//
// A collection of T ticks over E envs.  Episodes are ordered by (end tick, env): the order in which a host walking `for t: for e:`
// meets the done bytes.  The episode that ends at cell (t, e) is added whole and oldest first -- the transitions an earlier chunk left
// in the PENDING STORE (row k E + e: transition k of env e's running episode) in front of this chunk's -- to the bad ring when
// collisions[t][e] != 0, else to the good ring, each transition one sequential add: ring row (idx + rank) mod maxsize, rank counted
// over all adds of the call to that ring, and a rank below n - maxsize is skipped (a later add of the same call overwrites it).
//   walk 1 (route_walk_lengths, a lane per env, forward)   the length of the episode that ends at each cell, both classes packed
//                                                          into one 64-bit word (bad << 32 | good), 0 elsewhere; the new pend_len
//   exclusive scan of those words in cell order            = the first rank of every episode in its ring; the total = counts
//   walk 2 (route_walk_rows, a lane per env, BACKWARD)     from an end cell back to the episode's start the ranks count down; what
//                                                          is left over at tick 0 is the pending prefix (flush_row); what lies
//                                                          behind the last end is the new pending tail
// Both walks request their loads in groups of kRouteGroup ticks ahead of the serial part (the group's loads are independent, the
// serial part is a few integer instructions per tick), and a lane's loads run along the env index: coalesced.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define CM3_ROUTE_HD __host__ __device__ inline
#else
#define CM3_ROUTE_HD inline
#endif

namespace cm3 {

constexpr uint8_t kRouteBad = 0, kRouteGood = 1, kRoutePending = 2, kRouteSkip = 255;   // the values of `sel`
constexpr int kRouteGroup = 8;              // ticks whose loads a walk requests together
constexpr uint64_t kRouteLow = 0xffffffffull;

struct RouteShape {
  const uint8_t *done;      // [T][E], st_done bytes per tick
  const int32_t *coll;      // [T][E] scenario.collisions after every tick, st_coll bytes per tick
  const uint8_t *valid;     // optional [T][E], st_valid bytes per tick: 0 = the transition does not exist
  size_t st_done, st_coll, st_valid;
  int T, E, P;              // P: depth of the pending store
  int sync;                 // 1: episode-synchronous -- an episode still open at the last tick ends there, nothing pends
  int64_t idx[2], maxsize[2];   // [0] the bad ring, [1] the good ring
};

// T E + P E fits 31 bits (the ranks of one call, pending prefixes included, then fit a half of the packed word)
CM3_ROUTE_HD bool route_shape_fits(int64_t T, int64_t E, int64_t P) {
  return T >= 1 && E >= 1 && P >= 0 && T <= 0x7fffffff && P <= 0x7fffffff && (T + P) * E < ((int64_t)1 << 31);
}
// scratch of the plan in 64-bit words: lengths [T E], first ranks [T E], block partials [ceil(T E / cells per block)]
constexpr int kRouteScanCells = 1024;       // cells per workgroup of the scan launches (256 lanes x 4)
CM3_ROUTE_HD size_t route_scan_blocks(size_t cells) { return (cells + kRouteScanCells - 1) / kRouteScanCells; }
CM3_ROUTE_HD size_t route_scratch_words(size_t cells) { return 2 * cells + route_scan_blocks(cells); }

template <typename T> CM3_ROUTE_HD const T *route_tick(const T *base, size_t stride, int t) {
  return reinterpret_cast<const T *>(reinterpret_cast<const char *>(base) + stride * (size_t)t);
}
CM3_ROUTE_HD uint64_t route_pack(int cls, uint32_t len) { return cls == kRouteBad ? (uint64_t)len << 32 : (uint64_t)len; }
CM3_ROUTE_HD int route_class(uint64_t w) { return (w >> 32) ? kRouteBad : kRouteGood; }
CM3_ROUTE_HD int64_t route_half(uint64_t w, int cls) { return (int64_t)(cls == kRouteBad ? w >> 32 : w & kRouteLow); }

// The ring a call adds n transitions to: the first `skip` ranks are overwritten again by the call itself, rank `skip` lands on `start`.
struct RouteRing {
  int64_t skip, start, maxsize;
};
CM3_ROUTE_HD RouteRing route_ring(int64_t idx, int64_t maxsize, int64_t n) {
  RouteRing r;
  r.maxsize = maxsize;
  r.skip = n > maxsize ? n - maxsize : 0;
  r.start = (idx + r.skip) % maxsize;
  return r;
}
// rank -> ring row (idx + rank) mod maxsize, or -1: skipped
CM3_ROUTE_HD int64_t route_row(const RouteRing &r, int64_t rank) {
  if (rank < r.skip) return -1;
  const int64_t row = r.start + (rank - r.skip);          // (rank - skip < maxsize)
  return row >= r.maxsize ? row - r.maxsize : row;
}

// Walk 1, env e: len[t E + e] = packed length of the episode that ends at (t, e), pending prefix included, 0 where none ends.
// Returns the new pend_len of the env: the transitions behind its last end (with the old ones where nothing ended), at most P.
// (A tail that outgrows P -- the caller keeps P >= the longest episode, so only a misuse of the C ABI gets here -- saturates: walk 2
// then gives the NEWEST transitions rows P - 1 downwards and drops the older ones; the episode is no longer whole, nothing is out of
// bounds.)
CM3_ROUTE_HD int route_walk_lengths(const RouteShape &s, int e, int pend_in, uint64_t *len) {
  constexpr int G = kRouteGroup;
  int run = s.sync ? 0 : pend_in;
  for (int t0 = 0; t0 < s.T; t0 += G) {
    uint8_t d[G], v[G];
    int32_t c[G];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int g = 0; g < G; ++g) {
      const int t = t0 + g < s.T ? t0 + g : s.T - 1;      // (ticks past the end repeat the last one's loads)
      d[g] = route_tick(s.done, s.st_done, t)[e];
      c[g] = route_tick(s.coll, s.st_coll, t)[e];
      v[g] = s.valid ? route_tick(s.valid, s.st_valid, t)[e] : (uint8_t)1;
    }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int g = 0; g < G; ++g) {
      const int t = t0 + g;
      if (t >= s.T) break;
      if (v[g]) ++run;
      bool end = v[g] && d[g];
      if (s.sync && t == s.T - 1 && run > 0) end = true;  // still open at the last tick: ends there, with its count so far
      uint64_t w = 0;
      if (end) {
        w = route_pack(c[g] != 0 ? kRouteBad : kRouteGood, (uint32_t)run);
        run = 0;
      }
      len[(size_t)t * s.E + e] = w;
    }
  }
  return run < s.P ? run : s.P;
}

// Walk 2, env e: sel / row of the chunk's transitions and the two flush_row columns of the env's pending rows.
// first: the exclusive scan of len in cell order; n: the totals per class; pend_new: what walk 1 returned.
CM3_ROUTE_HD void route_walk_rows(const RouteShape &s, int e, const uint64_t *len, const uint64_t *first, const int64_t *n, int pend_new,
                                  uint8_t *sel, int64_t *row, int64_t *flush_row) {
  constexpr int G = kRouteGroup;
  const RouteRing ring[2] = {route_ring(s.idx[0], s.maxsize[0], n[0]), route_ring(s.idx[1], s.maxsize[1], n[1])};
  int cls = -1;                 // the class of the episode the walk is inside (-1: behind the env's last end -- the pending tail)
  int64_t rank = 0, head = 0;   // the rank the next (earlier) transition of that episode takes; the episode's first rank
  int tail_k = pend_new - 1;    // the pending row index the next (earlier) transition of the tail takes
  for (int t1 = s.T - 1; t1 >= 0; t1 -= G) {
    uint64_t L[G], F[G];
    uint8_t v[G];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int g = 0; g < G; ++g) {
      const int t = t1 - g >= 0 ? t1 - g : 0;
      L[g] = len[(size_t)t * s.E + e];
      F[g] = first[(size_t)t * s.E + e];
      v[g] = s.valid ? route_tick(s.valid, s.st_valid, t)[e] : (uint8_t)1;
    }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int g = 0; g < G; ++g) {
      const int t = t1 - g;
      if (t < 0) break;
      if (L[g]) {
        cls = route_class(L[g]);
        head = route_half(F[g], cls);
        rank = head + route_half(L[g], cls) - 1;
      }
      uint8_t to = kRouteSkip;
      int64_t r = -1;
      if (v[g]) {
        if (cls < 0) {
          const int k = tail_k--;
          if (!s.sync && k >= 0 && k < s.P) {
            to = kRoutePending;
            r = (int64_t)k * s.E + e;
          }
        } else {
          r = route_row(ring[cls], rank--);
          if (r >= 0) to = (uint8_t)cls;
        }
      }
      sel[(size_t)t * s.E + e] = to;
      row[(size_t)t * s.E + e] = r;
    }
  }
  // what the env's first episode of this chunk still lacks are the rows an earlier chunk left pending: ranks head .. rank
  const int64_t prefix = cls < 0 ? 0 : rank - head + 1;
  for (int k = 0; k < s.P; ++k) {
    const int64_t r = k < prefix ? route_row(ring[cls], head + k) : -1;
    flush_row[(size_t)k * s.E + e] = cls == kRouteBad ? r : -1;
    flush_row[((size_t)s.P + k) * s.E + e] = cls == kRouteGood ? r : -1;
  }
}

// The whole plan in sequence on the host: the outputs of cm3_episode_route_plan, element for element.
// scratch: route_scratch_words(T E) 64-bit words (the first 2 T E are used).  pend_in and pend_out may be the same array (both
// unused when sync).
inline void route_plan_host(const RouteShape &s, const int32_t *pend_in, int32_t *pend_out, uint8_t *sel, int64_t *row, int64_t *flush_row,
                            int64_t *counts, uint64_t *scratch) {
  const size_t cells = (size_t)s.T * s.E;
  uint64_t *len = scratch, *first = scratch + cells;
  for (int e = 0; e < s.E; ++e) {
    const int p = route_walk_lengths(s, e, s.sync ? 0 : pend_in[e], len);
    if (!s.sync) pend_out[e] = p;
  }
  uint64_t sum = 0;
  for (size_t c = 0; c < cells; ++c) {
    first[c] = sum;
    sum += len[c];
  }
  counts[0] = route_half(sum, kRouteBad);
  counts[1] = route_half(sum, kRouteGood);
  for (int e = 0; e < s.E; ++e) route_walk_rows(s, e, len, first, counts, s.sync ? 0 : pend_out[e], sel, row, flush_row);
}

}  // namespace cm3
