// The fixed-order gather-reduce over ascending inverse lists, once: the backward of every loss whose gradient row is a sum over
// the list of the rows that name it (csrc/chamfer.hip, csrc/rigidity.hip), and the 256-wide double tree of the scalar reductions.
//
// A workgroup of kThreads owns 256 consecutive rows, a lane owns a row: its point p and its list's bounds [lo, hi).  What sets
// the cost is the length T = hi - lo of a row's list, so the sum has three forms, picked per row and all inside the one launch:
//   * T <= 32: the lane walks its own list, entries lo, lo + 1, ... added to 0 in that order -- T - 1 roundings;
//   * 32 < T <= 1024: the wave takes the row's list together, lane t entries lo + t, lo + t + 64, ... added to 0 in that order
//     (each entry index a coalesced read), and a butterfly over strides 32, 16, ... 1 sums the 64 partial sums: ceil(T / 64) + 5
//     additions on a term's way.  The ballot of such rows is walked in ascending lane order;
//   * T > 1024: the workgroup takes it, thread t entries lo + t, lo + t + 256, ..., and a tree in LDS over strides 128, 64, ... 1
//     (slot t += slot t + stride) sums the 256 partial sums: ceil(T / 256) + 7 additions.  The four waves' ballots of such rows go
//     through LDS, so every thread walks the same rows in the same order and the barriers are uniform; the row's bounds are read
//     again there and clamped as the lane's were.
// Every form's order of additions is a function of the list alone, nothing is atomic, and a row's sum does not depend on what
// the rows around it hold.  One workgroup per long list is the bound of this design: a list of 100 000 entries is 391
// dependent-free gathers per thread, where a lane alone would walk all 100 000.
//
// What is summed is the caller's: a term functor with
//     void add(int slot, float px, float py, float pz, float &sx, float &sy, float &sz) const
// that adds the term of entry slot `slot` for the row at p into the running sum.  Compile with contraction off: the bits follow
// from the source order of the term's expression.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nsdp {
namespace lists {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kLaneMax = 32;      // the longest list one lane walks alone
constexpr int kWaveMax = 1024;    // the longest list one wave shares; longer ones take the workgroup

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the LDS of reduce(): the 256 partial sums of a workgroup-form row, the four waves' ballots of such rows
struct Shared {
  float red[3][kThreads];
  unsigned long long big[kWaves];
};

// the terms of entry slots lo + first, lo + first + stride, ... below hi, added in that order
template <class Term>
__device__ __forceinline__ void walk(const Term &term, int lo, int hi, int first, int stride, float px, float py, float pz, float &sx,
                                     float &sy, float &sz) {
#pragma unroll 4
  for (int e = lo + first; e < hi; e += stride) term.add(e, px, py, pz, sx, sy, sz);
}

// (sx, sy, sz) of the calling lane's row = the sum of its list's terms; the lane passes its row's point and bounds (a lane
// without a row: lo == hi).  x: the points of the shape's rows, off: the shape's list offsets, clamped to [0, bound], row0: the
// workgroup's first row -- what the workgroup form reads for a row it shares.  EVERY thread of the workgroup must call it, from
// code the whole workgroup runs through (barriers).
template <class Term>
__device__ __forceinline__ void reduce(const Term &term, const float *__restrict__ x, const int32_t *__restrict__ off, int bound,
                                       int row0, int lo, int hi, float px, float py, float pz, Shared &shared, float &sx, float &sy,
                                       float &sz) {
  const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
  const int len = hi - lo;
  sx = 0.f; sy = 0.f; sz = 0.f;
  if (len <= kLaneMax) walk(term, lo, hi, 0, 1, px, py, pz, sx, sy, sz);
  // rows whose list a wave shares, in lane order (all 64 lanes are here: lanes without a row have len 0)
  unsigned long long todo = __ballot(len > kLaneMax && len <= kWaveMax);
  while (todo) {
    const int src = __ffsll(static_cast<long long>(todo)) - 1;
    todo &= todo - 1;
    float ax = 0.f, ay = 0.f, az = 0.f;
    walk(term, __shfl(lo, src), __shfl(hi, src), lane, 64, __shfl(px, src), __shfl(py, src), __shfl(pz, src), ax, ay, az);
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {      // (a + b == b + a: both partners hold the same bits after every level)
      ax += __shfl_xor(ax, s);
      ay += __shfl_xor(ay, s);
      az += __shfl_xor(az, s);
    }
    if (lane == src) { sx = ax; sy = ay; sz = az; }
  }
  // rows whose list the workgroup shares
  const unsigned long long mine = __ballot(len > kWaveMax);
  if (lane == 0) shared.big[wave] = mine;
  __syncthreads();
  for (int w = 0; w < kWaves; ++w) {
    unsigned long long rows = shared.big[w];
    while (rows) {
      const int r = w * 64 + __ffsll(static_cast<long long>(rows)) - 1;      // (set only for lanes with a row)
      rows &= rows - 1;
      const int ri = row0 + r;
      const float *p = x + static_cast<size_t>(ri) * 3;
      const int rlo = clampi(off[ri], 0, bound), rhi = clampi(off[ri + 1], rlo, bound);
      float ax = 0.f, ay = 0.f, az = 0.f;
      walk(term, rlo, rhi, tid, kThreads, p[0], p[1], p[2], ax, ay, az);
      shared.red[0][tid] = ax; shared.red[1][tid] = ay; shared.red[2][tid] = az;
      __syncthreads();
      for (int s = kThreads / 2; s > 0; s >>= 1) {
        if (tid < s) {
          shared.red[0][tid] += shared.red[0][tid + s];
          shared.red[1][tid] += shared.red[1][tid + s];
          shared.red[2][tid] += shared.red[2][tid + s];
        }
        __syncthreads();
      }
      if (tid == r) { sx = shared.red[0][0]; sy = shared.red[1][0]; sz = shared.red[2][0]; }
      __syncthreads();      // (red is rewritten by the next row)
    }
  }
}

// fixed tree over the 256 partial sums of a workgroup of kThreads; the result in part[0] (every thread must call it)
__device__ __forceinline__ void tree_sum(double *part) {
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (static_cast<int>(threadIdx.x) < s) part[threadIdx.x] += part[threadIdx.x + s];
    __syncthreads();
  }
}

}  // namespace lists
}  // namespace nsdp
