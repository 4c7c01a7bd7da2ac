// The second stage of every weight gradient, once: a row kernel leaves S partial results in a workspace and a small kernel sums
// them in a FIXED ORDER into dW / db (no atomics: the train step is bit-reproducible, and a captured step replays these sums).
// Used by gemm.hip, gemm_bf16.hip (linear layout), wgrad_bf16x3.hip (fragment layout, one-hot tables) and gemm_bf16x3.hip (K = 4
// tail).  THE ORDER IS THE CONTRACT -- tests/wgrad_reduce_ref.py emulates it from this text and the GPU tests compare bits:
//
//   eight chains (sum8)   chains a0 .. a7 start at zero.  The partials are taken in groups of eight, s = 8 j + u going to chain
//                         u, in rising j; the S % 8 partials behind the last whole group go to chain 0, in rising s.  The
//                         result is ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7)).
//   four chains (sum4)    the same with four: s = first + 4 j + u to chain u, the remainder to chain 0, (a0 + a1) + (a2 + a3).
//   eight ranges          S is cut into eight ranges of ceil(S / 8) partials (the last ones shorter, or empty: their sum is 0);
//                         each range is summed with four chains, and the eight range sums r0 .. r7 combine as
//                         ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)).
//   target                dst = sum, or dst = dst + sum (one more addition) where the descriptor says accumulate.
//
// Linear layout (NsdpWgradB16ReduceDesc: the fp32 and bf16-storage row kernels): workspace [S][N K + N], element e < N K is
// dW[e], the N behind them db; summed with eight chains, one thread per element.
// Fragment layout (NsdpWgradReduceDesc: the bf16x3 row kernels): workspace [column parts][S][nta ktb 256 + nta 16], a partial
// being the row kernel's accumulator tiles as the MFMA leaves them, then its db slots (read from column part 0); summed over
// eight ranges, 32 elements x 8 ranges per workgroup, the range sums meeting in LDS.
#pragma once
#include "common.h"
#include "prof.h"

namespace {

// ---- the two strided sums: partials p[s * stride], s in [first, last) ----
__device__ __forceinline__ float sum8(const float *__restrict__ p, int S, long long stride) {
  float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};      // 8 loads in flight per lane (one dependent chain is latency-bound)
  int s = 0;
  for (; s + 8 <= S; s += 8) {
#pragma unroll
    for (int u = 0; u < 8; ++u) a[u] += p[(s + u) * stride];
  }
  for (; s < S; ++s) a[0] += p[s * stride];
  return ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
}
__device__ __forceinline__ float sum4(const float *__restrict__ p, int first, int last, long long stride) {
  float a[4] = {0.f, 0.f, 0.f, 0.f};
  int s = first;
  for (; s + 4 <= last; s += 4) {
#pragma unroll
    for (int u = 0; u < 4; ++u) a[u] += p[(s + u) * stride];
  }
  for (; s < last; ++s) a[0] += p[s * stride];
  return (a[0] + a[1]) + (a[2] + a[3]);
}

// ---- linear layout: element e of one layer (one thread) ----
__device__ __forceinline__ void reduce_block(const NsdpWgradB16ReduceDesc &d) {
  const long long e = blockIdx.x * 256LL + threadIdx.x;
  const long long nw = static_cast<long long>(d.N) * d.K;
  if (e >= nw + (d.db ? d.N : 0)) return;
  const float t = sum8(d.ws + e, d.S, nw + d.N);
  float *dst = e < nw ? d.dW + e : d.db + (e - nw);
  *dst = d.accumulate ? *dst + t : t;
}
inline unsigned reduce_blocks(const NsdpWgradB16ReduceDesc &d) {
  return static_cast<unsigned>((static_cast<long long>(d.N) * d.K + (d.db ? d.N : 0) + 255) / 256);
}
inline bool reduce_desc_ok(const NsdpWgradB16ReduceDesc &d) { return d.ws && d.dW && d.S > 0 && d.N > 0 && d.K > 0; }

// ---- fragment layout ----
__host__ __device__ inline long long fragment_stride(int nta, int ktb) { return static_cast<long long>(nta) * ktb * 256 + nta * 16; }
// Offset of partial 0 of dW[n][k]: column part k / (16 ktb) (grid.y of the row kernel, S partials each), accumulator tile
// (n / 16, k / 16 within the part), lane 16 ((n % 16) / 4) + k % 16, register n % 4 (C/D layout of the MFMA: row = 4 (lane >> 4)
// + register, column = lane & 15).  db[n]: the slot behind the tiles of a partial of column part 0.
__device__ __forceinline__ long long fragment_offset(int S, int nta, int ktb, int n, int k) {
  const int kpart = k / (ktb * 16), kp = k - kpart * ktb * 16;
  const int nl = n & 15, kl = kp & 15;
  return kpart * S * fragment_stride(nta, ktb) + (static_cast<long long>(n >> 4) * ktb + (kp >> 4)) * 256 + (16 * (nl >> 2) + kl) * 4 +
         (nl & 3);
}
__device__ __forceinline__ long long fragment_db_offset(int nta, int ktb, int n) { return static_cast<long long>(nta) * ktb * 256 + n; }

// 32 elements x 8 ranges per workgroup of 256: a thread sums one range of one element (S / 8 independent loads in flight instead
// of a chain of S), thread (range 0, element) combines the eight.
__device__ __forceinline__ void reduce_block(const NsdpWgradReduceDesc &d) {
  __shared__ float range_sum[8][32];
  const int N = d.N, K = d.K, S = d.S;
  const long long nw = static_cast<long long>(N) * K;
  if (blockIdx.x * 32LL >= nw + (d.db ? N : 0)) return;      // (uniform per workgroup)
  const int el = threadIdx.x & 31, q = threadIdx.x >> 5;
  const long long e = blockIdx.x * 32LL + el;
  const bool valid = e < nw + (d.db ? N : 0);
  float t = 0.f;
  if (valid) {
    const long long first = e < nw ? fragment_offset(S, d.nta, d.ktb, static_cast<int>(e / K), static_cast<int>(e % K))
                                   : fragment_db_offset(d.nta, d.ktb, static_cast<int>(e - nw));
    const int per = (S + 7) / 8, s0 = q * per;
    t = sum4(d.ws + first, s0, s0 + per < S ? s0 + per : S, fragment_stride(d.nta, d.ktb));
  }
  range_sum[q][el] = t;
  __syncthreads();
  if (q == 0 && valid) {
    t = ((range_sum[0][el] + range_sum[1][el]) + (range_sum[2][el] + range_sum[3][el])) +
        ((range_sum[4][el] + range_sum[5][el]) + (range_sum[6][el] + range_sum[7][el]));
    float *dst = e < nw ? d.dW + e : d.db + (e - nw);
    *dst = d.accumulate ? *dst + t : t;
  }
}
inline unsigned reduce_blocks(const NsdpWgradReduceDesc &d) {
  return static_cast<unsigned>((static_cast<long long>(d.N) * d.K + (d.db ? d.N : 0) + 31) / 32);
}
inline bool reduce_desc_ok(const NsdpWgradReduceDesc &d) {
  return d.ws && d.dW && d.S > 0 && d.N > 0 && d.K > 0 && d.nta > 0 && d.ktb > 0;
}

// ---- one kernel per layout and descriptor count: COUNT descriptors by value in the kernel arguments, grid.y = layer, grid.x
// covers the largest layer.  COUNT = 1 is the reduce behind a one-call weight gradient (40-byte arguments), kReduceBatch the
// batched entries' -- the same body, so a gradient does not depend on which of the two reduced it.
constexpr int kReduceBatch = 48;
template <typename Desc, int COUNT>
struct ReduceBatch {
  Desc d[COUNT];
};
template <typename Desc, int COUNT>
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(ReduceBatch<Desc, COUNT> b) {
  reduce_block(b.d[blockIdx.y]);
}

// the reduce of one layer, described as the partials form of its entry would have handed it out
template <typename Desc>
int reduce_one(const Desc &d, hipStream_t st) {
  hipLaunchKernelGGL((wgrad_reduce_kernel<Desc, 1>), dim3(reduce_blocks(d)), dim3(256), 0, st, ReduceBatch<Desc, 1>{{d}});
  return nsdp::launch_status("wgrad_reduce_kernel");
}

// the batched entries: `who` names the entry in its messages (and its trace line, if it has one)
template <typename Desc>
int reduce_batched(const Desc *descs, int count, const char *who, bool trace, hipStream_t st) {
  if (count <= 0) return 0;
  NSDP_REQUIRE(descs, "%s: null descriptor array", who);
  for (int base = 0; base < count; base += kReduceBatch) {
    ReduceBatch<Desc, kReduceBatch> b;
    const int n = count - base < kReduceBatch ? count - base : kReduceBatch;
    unsigned blocks = 1;
    for (int i = 0; i < n; ++i) {
      const Desc &e = descs[base + i];
      NSDP_REQUIRE(reduce_desc_ok(e), "%s: bad descriptor %d", who, base + i);
      b.d[i] = e;
      blocks = reduce_blocks(e) > blocks ? reduce_blocks(e) : blocks;
    }
    for (int i = n; i < kReduceBatch; ++i) b.d[i] = b.d[0];      // never indexed (grid.y = n)
    if (trace) NSDP_TRACE("%s x%d", who, n);
    hipLaunchKernelGGL((wgrad_reduce_kernel<Desc, kReduceBatch>), dim3(blocks, n), dim3(256), 0, st, b);
    const int rc = nsdp::launch_status("wgrad_reduce_kernel (batched)");
    if (rc) return rc;
  }
  return 0;
}

}  // namespace
