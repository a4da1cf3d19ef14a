// Stateless counter hash shared by kernels that draw reproducible random decisions.
//
// The same function as `hash4` of attention.hip (the attention dropout mask), kept here for the
// kernels written after it; ops/image_batch.py carries the Python twin.  Host and device.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define NDP_HASH_HD __host__ __device__ __forceinline__
#else
#define NDP_HASH_HD inline
#endif

namespace ndp {

NDP_HASH_HD uint32_t counter_hash4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  // small avalanche hash (murmur3 finaliser rounds); counter-based, stateless
  uint32_t h = a * 0x9E3779B1u ^ (b + 0x7F4A7C15u) * 0x85EBCA77u;
  h ^= (c + 0x165667B1u) * 0xC2B2AE3Du;
  h = (h ^ (h >> 15)) * 0x2C1B3C6Du;
  h ^= (d + 0x27D4EB2Fu) * 0x9E3779B1u;
  h = (h ^ (h >> 13)) * 0x297A2D39u;
  return h ^ (h >> 16);
}

}  // namespace ndp
