// The keyed draws of include/nsdp_batch.h and include/nsdp_meshbatch.h: the integer mix, the absorption step and the part of a
// key that the host forms (seed, epoch, step) -- one definition for batch_assemble.hip and mesh_sample.hip, so that "the key of
// nsdp_subset_draw" is the same code in both.  A kernel finishes the key with absorb(absorb(base, b), which).
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace nsdp {

// a bijection of 2^32
__host__ __device__ __forceinline__ uint32_t mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7FEB352Du;
  x ^= x >> 15;
  x *= 0x846CA68Bu;
  x ^= x >> 16;
  return x;
}

__host__ __device__ __forceinline__ uint32_t absorb(uint32_t h, uint32_t v) { return mix32((h ^ v) + 0x9E3779B9u); }

// the key after seed, epoch and step
inline uint32_t draw_base_key(uint64_t seed, uint32_t epoch, uint32_t step) {
  uint32_t base = 0x4E534450u;
  base = absorb(base, static_cast<uint32_t>(seed & 0xFFFFFFFFull));
  base = absorb(base, static_cast<uint32_t>(seed >> 32));
  base = absorb(base, epoch);
  return absorb(base, step);
}

}  // namespace nsdp
