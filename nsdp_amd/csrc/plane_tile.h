// The source tile of the exhaustive point searches, once: csrc/knn.hip (knn_split_queue_scan), csrc/eval_metric.hip (nn_scan)
// and csrc/pointnet2_ops.hip (ball_query_quad_kernel, three_nn_quad_kernel).
//
// Layout: up to kRows source points in LDS as three coordinate planes x[], y[], z[], each 16-byte aligned, so four consecutive
// candidates are three 16-byte reads (the same address in every lane that scans the same candidates: a broadcast) and their
// squared distances two packed fp32 operations per step of the expression.
// Sentinels: load() writes kPad entries x = FLT_MAX, y = z = 0 behind the last row.  For any finite query (FLT_MAX - |qx|)^2
// overflows to +inf, and +inf passes no `d < threshold`, `d < r^2` or `d < best` -- a scan may read past the last row without a
// range check, as far as the pad reaches.
// Required pad: the rows a scan reads behind cnt.  One lane walking the tile four rows at a time reads below
// round_up(cnt, 4) <= cnt + 3: kPad = 4 (nn_scan).  Four lanes that share a query read below round_up(cnt, 16) <= cnt + 15,
// whether each takes every fourth group of four (the quad kernels) or a quarter rounded up to four (knn_split_queue_scan):
// kPad = 16.
// Bits: dist4 is nsdp::sq_dist3 on four candidates, ((dx*dx + dy*dy) + dz*dz) with dx = query - source and one rounding per
// operation, which holds only without contraction -- hence the pragma below, on top of the including file's place in build.py's
// EXACT list.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>

#pragma clang fp contract(off)

namespace nsdp {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int kRows, int kPad>
struct PlaneTile {
  static_assert(kRows % 4 == 0 && kPad % 4 == 0, "the planes stay 16-byte aligned behind one another");
  __attribute__((aligned(16))) float x[kRows + kPad];
  __attribute__((aligned(16))) float y[kRows + kPad];
  __attribute__((aligned(16))) float z[kRows + kPad];

  // rows [0, cnt) of `src` (row r at src + 3 r), cnt <= kRows, and the sentinels, by a workgroup of kThreads.  The caller keeps
  // the barriers: one in front (nobody reads the previous tile any more), one behind.
  template <int kThreads>
  __device__ __forceinline__ void load(const float *__restrict__ src, int cnt) {
    static_assert(kPad <= kThreads, "one thread per sentinel");
    for (int t = threadIdx.x; t < cnt; t += kThreads) {
      const float *p = src + static_cast<size_t>(t) * 3;
      x[t] = p[0]; y[t] = p[1]; z[t] = p[2];
    }
    if (threadIdx.x < kPad) {
      x[cnt + threadIdx.x] = FLT_MAX; y[cnt + threadIdx.x] = 0.f; z[cnt + threadIdx.x] = 0.f;
    }
  }

  // candidates t .. t + 3 (t % 4 == 0, t + 3 < cnt + kPad)
  __device__ __forceinline__ void read4(int t, f32x4 &X, f32x4 &Y, f32x4 &Z) const {
    X = *reinterpret_cast<const f32x4 *>(&x[t]);
    Y = *reinterpret_cast<const f32x4 *>(&y[t]);
    Z = *reinterpret_cast<const f32x4 *>(&z[t]);
  }
};

// squared distances of the query to the four candidates of a read4: d01 = candidates 0 and 1, d23 = candidates 2 and 3
__device__ __forceinline__ void dist4(f32x4 X, f32x4 Y, f32x4 Z, float qx, float qy, float qz, f32x2 &d01, f32x2 &d23) {
  const f32x2 q2x = {qx, qx}, q2y = {qy, qy}, q2z = {qz, qz};
  {
    const f32x2 dx = q2x - f32x2{X[0], X[1]}, dy = q2y - f32x2{Y[0], Y[1]}, dz = q2z - f32x2{Z[0], Z[1]};
    d01 = (dx * dx + dy * dy) + dz * dz;
  }
  {
    const f32x2 dx = q2x - f32x2{X[2], X[3]}, dy = q2y - f32x2{Y[2], Y[3]}, dz = q2z - f32x2{Z[2], Z[3]};
    d23 = (dx * dx + dy * dy) + dz * dz;
  }
}

}  // namespace nsdp
