// Device pieces shared by the farthest-point-sampling kernels (fps.hip: one workgroup per cloud; fps_cluster.hip: a cluster of
// workgroups per cloud): the 64-bit arg-max key {bits(min-dist) : tie priority} and its decoding, the validity rule, the wave
// and workgroup maxima, the per-lane update loop and the shape of one cloud of a packed set.  The key's maximum is a maximum
// over all points whatever the thread partition, so every kernel built from these pieces picks the same winners, ties included.
// Include only from translation units built with -ffp-contract=off.
#pragma once
#include <climits>
#include <cmath>

#include "common.h"
#include "ragged.h"

#pragma clang fp contract(off)

namespace nsdp {
namespace fps {

constexpr int kRankShift = 22;  // low bits: k div BS, high bits: bit-reversed (k mod BS)

template <int CTRL>
__device__ __forceinline__ long long dpp_max_step(long long v) {
  const int lo = __builtin_amdgcn_update_dpp(0, static_cast<int>(v), CTRL, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, static_cast<int>(v >> 32), CTRL, 0xf, 0xf, false);
  const long long o = (static_cast<long long>(hi) << 32) | static_cast<unsigned>(lo);
  return o > v ? o : v;
}

// max over the 64 lanes of a wave, result in every lane.
__device__ __forceinline__ long long wave_max_i64(long long v) {
  v = dpp_max_step<0xB1>(v);   // quad_perm [1,0,3,2]
  v = dpp_max_step<0x4E>(v);   // quad_perm [2,3,0,1]
  v = dpp_max_step<0x141>(v);  // row_half_mirror
  v = dpp_max_step<0x140>(v);  // row_mirror  -> every lane of a 16-lane row holds the row max
  {
    const unsigned lo = static_cast<unsigned>(v), hi = static_cast<unsigned>(v >> 32);
    const auto l = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
    const auto h = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    const long long a = (static_cast<long long>(h[0]) << 32) | l[0];
    const long long b = (static_cast<long long>(h[1]) << 32) | l[1];
    v = a > b ? a : b;
  }
  {
    const unsigned lo = static_cast<unsigned>(v), hi = static_cast<unsigned>(v >> 32);
    const auto l = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
    const auto h = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
    const long long a = (static_cast<long long>(h[0]) << 32) | l[0];
    const long long b = (static_cast<long long>(h[1]) << 32) | l[1];
    v = a > b ? a : b;
  }
  return v;
}

__device__ __forceinline__ unsigned tie_priority(int k, int BS, int log2BS) {
  const unsigned kmod = static_cast<unsigned>(k) & static_cast<unsigned>(BS - 1);
  const unsigned br = log2BS ? (__brev(kmod) >> (32 - log2BS)) : 0u;
  const unsigned rank = (br << kRankShift) | (static_cast<unsigned>(k) >> log2BS);
  return ~rank;  // larger = preferred on a tie
}

__device__ __forceinline__ int decode_winner(long long key, int log2BS) {
  if (key < 0) return 0;  // no valid point at all: reference keeps besti = 0
  const unsigned rank = ~static_cast<unsigned>(key);
  const unsigned br = rank >> kRankShift;
  const unsigned q = rank & ((1u << kRankShift) - 1u);
  const unsigned kmod = log2BS ? (__brev(br) >> (32 - log2BS)) : 0u;
  return static_cast<int>((q << log2BS) | kmod);
}

__device__ __forceinline__ bool point_valid(float x, float y, float z) {
  const float mag = (x * x) + (y * y) + (z * z);  // contraction is off in these files
  return !(static_cast<double>(mag) <= 1e-3);     // sampling_gpu.cu:100-101 (float vs double literal)
}

// One lane's state for point k of a cloud of N: its running distance (1e10, or -1 for a point that never wins and never
// updates: an invalid one, or no point at all) and its tie priority.
__device__ __forceinline__ void init_point(const float *__restrict__ xyz, int k, int N, int BS, int log2BS, float &x, float &y,
                                           float &z, float &t, unsigned &prio) {
  if (k < N) {
    x = xyz[k * 3 + 0]; y = xyz[k * 3 + 1]; z = xyz[k * 3 + 2];
    t = point_valid(x, y, z) ? 1e10f : -1.0f;
    prio = tie_priority(k, BS, log2BS);
  } else {
    x = y = z = 0.f;
    t = -1.0f;
    prio = 0u;
  }
}

// The per-lane step: fold the new centre into the P running distances, return the lane's best key.
template <int P>
__device__ __forceinline__ long long update_points(const float (&px)[P], const float (&py)[P], const float (&pz)[P],
                                                   float (&pt)[P], const unsigned (&prio)[P], float cx, float cy, float cz) {
  long long best = LLONG_MIN;
#pragma unroll
  for (int s = 0; s < P; ++s) {
    const float d = nsdp::sq_dist3(px[s], py[s], pz[s], cx, cy, cz);
    const float t = fminf(d, pt[s]);
    pt[s] = t;
    const long long key = (static_cast<long long>(__float_as_int(t)) << 32) | prio[s];
    best = key > best ? key : best;
  }
  return best;
}

// The LDS hop across the W waves of a workgroup (slots[2][W], parity-double-buffered: one barrier per step): every wave
// passes its wave maximum and gets the workgroup's.
template <int W>
__device__ __forceinline__ long long block_max_i64(long long *slots, int j, int tid, long long best) {
  long long *slot = slots + (j & 1) * W;
  if ((tid & 63) == 0) slot[tid >> 6] = best;
  __syncthreads();
  long long g = slot[0];
#pragma unroll
  for (int w = 1; w < W; ++w) {
    const long long o = slot[w];
    g = o > g ? o : g;
  }
  return g;
}

// One cloud of a packed set (ragged.h): its rows, its size and its tie-rule block size BS = min(512, 2^floor(log2 n)) -- the
// reference's opt_n_threads by integer arithmetic -- all from the offsets on the device.  `n_max` (the host's bound: it sized
// the workgroups) caps the row count on top of the offsets' clamp.  false: the shape has no rows; every slot of `out` (where
// the caller passes one) then holds its (clamped) first-row index.
__device__ __forceinline__ bool fps_ragged_shape(const int32_t *__restrict__ offsets, int shape, int cap, int n_max, int M,
                                             int32_t *__restrict__ out, int &lo, int &N, int &BS, int &log2BS) {
  int hi;
  nsdp::ragged_range(offsets, shape, cap, lo, hi);
  N = min(hi - lo, n_max);
  if (N <= 0) {
    const int fill = min(lo, cap - 1);
    if (out)
      for (int j = threadIdx.x; j < M; j += blockDim.x) out[j] = fill;
    return false;
  }
  log2BS = min(9, 31 - __builtin_clz(static_cast<unsigned>(N)));
  BS = 1 << log2BS;
  return true;
}

// cuda_utils.h:15-19 -- same double arithmetic as the reference host code.
inline int opt_n_threads(int work_size) {
  const int pow_2 = static_cast<int>(std::log(static_cast<double>(work_size)) / std::log(2.0));
  int t = 1 << pow_2;
  if (t > 512) t = 512;
  if (t < 1) t = 1;
  return t;
}

}  // namespace fps
}  // namespace nsdp
