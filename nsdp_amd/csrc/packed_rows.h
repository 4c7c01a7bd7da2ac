// One lane per packed row: which shape owns a row of packed(cap, C) with offsets(B+1) int32 on the device.  Shared by the
// per-row kernels over packed sets (handles_ragged.hip: the handle rule; handle_sets.hip: labelled handle sets), so both clamp
// the offsets by one text.  (ragged.h holds the per-TILE walk of the decoder and search kernels.)
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

__device__ __forceinline__ int clamped(int v, int lo, int hi) { return min(max(v, lo), hi); }

// Rows [first, end) of shape b (0 <= b < B): 0 <= first <= end <= cap whatever `offsets` holds.
__device__ __forceinline__ void shape_range(const int32_t *__restrict__ offsets, int b, int cap, int &first, int &end) {
  first = clamped(offsets[b], 0, cap);
  end = clamped(offsets[b + 1], first, cap);
}

// The shape that owns packed row p: the last b in [0, B) whose clamped first row is <= p, if p is below that shape's clamped
// end.  Binary search for the first j in [1, B] with offsets[j] > p (B <= 65535: at most 16 steps).  false: no shape owns p.
__device__ __forceinline__ bool owner_of(const int32_t *__restrict__ offsets, int B, int cap, int p, int &b, int &first, int &end) {
  int lo = 1, hi = B + 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (clamped(offsets[mid], 0, cap) > p)
      hi = mid;
    else
      lo = mid + 1;
  }
  if (lo > B) return false;      // p is at or beyond offsets[B]
  b = lo - 1;
  shape_range(offsets, b, cap, first, end);
  return p >= first && p < end;
}

// The owner of lane's row p < cap, one search per wave where the wave's rows fall in one shape: the wave's first row (lane 0
// is the wave's lowest row, always below cap here) looks its shape up with uniform (scalar) loads; lanes whose row lies outside
// that shape search for themselves.  false: padding, no shape owns the row.
__device__ __forceinline__ bool owner_of_lane(const int32_t *__restrict__ offsets, int B, int cap, long long p, int &b) {
  const int p0 = __builtin_amdgcn_readfirstlane(static_cast<int>(p));
  int first = 0, end = 0;
  b = 0;
  bool owned = owner_of(offsets, B, cap, p0, b, first, end);
  b = __builtin_amdgcn_readfirstlane(b);
  if (!owned || p >= end) owned = owner_of(offsets, B, cap, static_cast<int>(p), b, first, end);
  return owned;
}

}  // namespace
