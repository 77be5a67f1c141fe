// Host side of the XCD-aware block order (what it is and what it measured: common.h, next to cm3_xcd_block): the flag bits and the
// grid for a launch of `blocks` workgroups.  Plain C++, no HIP: particle_plan.h plans launches with it on a machine without a GPU.
#pragma once
#include <stdint.h>

constexpr uint32_t kFlagXcdShift = 24, kXcdTiles = 63u;   // internal launch flag bits
static inline uint32_t cm3_xcd_flags(unsigned blocks) {
  if (blocks < 64u) return 0u;
  return (blocks <= 256u ? (blocks + 7u) / 8u : kXcdTiles) << kFlagXcdShift;
}
static inline unsigned cm3_xcd_grid(unsigned blocks) {
  const uint32_t v = cm3_xcd_flags(blocks) >> kFlagXcdShift;
  return v == 0u ? blocks : (v == kXcdTiles ? (blocks + 255u) / 256u * 256u : 8u * v);
}
