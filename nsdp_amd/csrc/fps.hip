// Farthest-point sampling for gfx950 -- replaces furthest_point_sampling_kernel
// (/root/reference/pointnet2_ops_lib/pointnet2_ops/_ext-src/src/sampling_gpu.cu:69-229, host sampling.cpp:66-87).
//
// MI355X design (not the reference's): FPS is a chain of `nsamples` dependent arg-max steps, i.e.
// latency-bound (algorithmic HBM traffic is only N*12 + nsamples*4 bytes per cloud).  So
//   * the whole cloud and the running min-distance live in VGPRs (P points per lane), never re-read
//     from global/L2 as the reference does (it re-reads `dataset` and `temp` every iteration);
//   * one workgroup per cloud, 8 points per lane: T = 256 threads (one wave per SIMD) for N <= 2048,
//     a single wave for N <= 512 (no barrier at all), 512/1024 threads up to N = 8192; clouds of a
//     batch run on different CUs;
//   * the arg-max is a 64-bit key max {bits(min-dist) : tie-priority} done with DPP quad/row mirrors +
//     v_permlane16/32_swap (pure VALU, no LDS round trip), then ONE LDS hop across the 4 waves with
//     parity-double-buffered slots, i.e. one s_barrier per iteration;
//   * the winner's coordinates come from an LDS copy of the cloud (one ds_read_b128).
// Exactness: distances use one fp32 rounding per operation (file built with -ffp-contract=off), and the
// low key word encodes the reference kernel's tie rule -- thread t = k mod BS scans k ascending with a
// strict '>', and the shared-memory tree keeps the entry with the smaller bit-reversed thread id -- so
// the indices are the reference's even on exact ties (BS = opt_n_threads(N), cuda_utils.h:15-19).
#include <climits>
#include <cmath>

#include "common.h"
#include "fps_common.h"
#include "prof.h"
#include "ragged.h"

#pragma clang fp contract(off)

namespace {

using namespace nsdp::fps;  // fps_common.h: the key, the maxima and the shape of a packed cloud

// Register-resident FPS of one cloud by one workgroup: T threads, P points per thread (N <= T*P).  The indices written are
// `base` + the index within the cloud (0 for a rectangular batch, the shape's first row for a packed one).
template <int T, int P, bool LDS_XYZ>
__device__ __forceinline__ void fps_reg_body(char *smem, const float *__restrict__ xyz, int N, int M, int BS, int log2BS,
                                             int32_t *__restrict__ out, int base) {
  constexpr int W = T / 64;
  long long *slots = reinterpret_cast<long long *>(smem);          // [2][W] (padded to 16*W bytes)
  float4 *sxyz = reinterpret_cast<float4 *>(smem + 16 * (W > 1 ? W : 1));
  const int tid = threadIdx.x;

  float px[P], py[P], pz[P], pt[P];
  unsigned prio[P];
#pragma unroll
  for (int s = 0; s < P; ++s) {
    const int k = tid + s * T;
    init_point(xyz, k, N, BS, log2BS, px[s], py[s], pz[s], pt[s], prio[s]);
    if (LDS_XYZ && k < N) sxyz[k] = make_float4(px[s], py[s], pz[s], 0.f);
  }
  if (tid == 0) out[0] = base;
  if (LDS_XYZ) __syncthreads();

  float cx, cy, cz;
  if (LDS_XYZ) {
    const float4 c = sxyz[0];
    cx = c.x; cy = c.y; cz = c.z;
  } else {
    cx = xyz[0]; cy = xyz[1]; cz = xyz[2];
  }

  for (int j = 1; j < M; ++j) {
    long long best = wave_max_i64(update_points<P>(px, py, pz, pt, prio, cx, cy, cz));
    if (W > 1) best = block_max_i64<W>(slots, j, tid, best);
    const int old = decode_winner(best, log2BS);
    if (LDS_XYZ) {
      const float4 c = sxyz[old];
      cx = c.x; cy = c.y; cz = c.z;
    } else {
      cx = xyz[old * 3 + 0]; cy = xyz[old * 3 + 1]; cz = xyz[old * 3 + 2];
    }
    if (tid == 0) out[j] = base + old;
  }
}

template <int T, int P, bool LDS_XYZ>
__global__ __launch_bounds__(T) void fps_reg_kernel(const float *__restrict__ xyz_all, int N, int M,
                                                    int BS, int log2BS,
                                                    int32_t *__restrict__ idx_all) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  fps_reg_body<T, P, LDS_XYZ>(smem, xyz_all + static_cast<size_t>(blockIdx.x) * N * 3, N, M, BS, log2BS,
                              idx_all + static_cast<size_t>(blockIdx.x) * M, 0);
}

template <int T, int P, bool LDS_XYZ>
__global__ __launch_bounds__(T) void fps_reg_ragged_kernel(const float *__restrict__ xyz_packed,
                                                           const int32_t *__restrict__ offsets, int cap, int n_max, int M,
                                                           int32_t *__restrict__ idx_all) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int32_t *out = idx_all + static_cast<size_t>(blockIdx.x) * M;
  int lo, N, BS, log2BS;
  if (!fps_ragged_shape(offsets, static_cast<int>(blockIdx.x), cap, min(n_max, T * P), M, out, lo, N, BS, log2BS)) return;   // (uniform: before any barrier)
  fps_reg_body<T, P, LDS_XYZ>(smem, xyz_packed + static_cast<size_t>(lo) * 3, N, M, BS, log2BS, out, lo);
}

// Generic fallback for very large clouds (N > 8192): running min-distance in global scratch.
template <int T>
__device__ __forceinline__ void fps_big_body(const float *__restrict__ xyz, float *__restrict__ tmp, int N, int M, int BS,
                                             int log2BS, int32_t *__restrict__ out, int base) {
  constexpr int W = T / 64;
  __shared__ long long slots[2 * W];
  const int tid = threadIdx.x;
  for (int k = tid; k < N; k += T)
    tmp[k] = point_valid(xyz[k * 3 + 0], xyz[k * 3 + 1], xyz[k * 3 + 2]) ? 1e10f : -1.0f;
  if (tid == 0) out[0] = base;
  float cx = xyz[0], cy = xyz[1], cz = xyz[2];
  for (int j = 1; j < M; ++j) {
    long long best = LLONG_MIN;
    for (int k = tid; k < N; k += T) {
      const float d = nsdp::sq_dist3(xyz[k * 3 + 0], xyz[k * 3 + 1], xyz[k * 3 + 2], cx, cy, cz);
      const float t = fminf(d, tmp[k]);
      tmp[k] = t;
      const long long key =
          (static_cast<long long>(__float_as_int(t)) << 32) | tie_priority(k, BS, log2BS);
      best = key > best ? key : best;
    }
    const long long g = block_max_i64<W>(slots, j, tid, wave_max_i64(best));
    const int old = decode_winner(g, log2BS);
    cx = xyz[old * 3 + 0]; cy = xyz[old * 3 + 1]; cz = xyz[old * 3 + 2];
    if (tid == 0) out[j] = base + old;
  }
}

template <int T>
__global__ __launch_bounds__(T) void fps_big_kernel(const float *__restrict__ xyz_all,
                                                    float *__restrict__ tmp_all, int N, int M, int BS,
                                                    int log2BS, int32_t *__restrict__ idx_all) {
  fps_big_body<T>(xyz_all + static_cast<size_t>(blockIdx.x) * N * 3, tmp_all + static_cast<size_t>(blockIdx.x) * N, N, M, BS,
                  log2BS, idx_all + static_cast<size_t>(blockIdx.x) * M, 0);
}

// (tmp[cap]: a shape's running distances live at its own rows)
template <int T>
__global__ __launch_bounds__(T) void fps_big_ragged_kernel(const float *__restrict__ xyz_packed,
                                                           const int32_t *__restrict__ offsets, float *__restrict__ tmp, int cap,
                                                           int n_max, int M, int32_t *__restrict__ idx_all) {
  int32_t *out = idx_all + static_cast<size_t>(blockIdx.x) * M;
  int lo, N, BS, log2BS;
  if (!fps_ragged_shape(offsets, static_cast<int>(blockIdx.x), cap, n_max, M, out, lo, N, BS, log2BS)) return;
  fps_big_body<T>(xyz_packed + static_cast<size_t>(lo) * 3, tmp + lo, N, M, BS, log2BS, out, lo);
}

template <int T, int P, bool LDS_XYZ>
int launch_reg(const float *xyz, int B, int N, int M, int BS, int log2BS, int32_t *idx, hipStream_t st) {
  constexpr int W = T / 64;
  const size_t smem = 16 * (W > 1 ? W : 1) + (LDS_XYZ ? static_cast<size_t>(N) * 16 : 0);
  if (smem > 64 * 1024) {
    NSDP_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&fps_reg_kernel<T, P, LDS_XYZ>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(smem)));
  }
  hipLaunchKernelGGL((fps_reg_kernel<T, P, LDS_XYZ>), dim3(B), dim3(T), smem, st, xyz, N, M, BS, log2BS,
                     idx);
  return nsdp::launch_status("fps_reg_kernel");
}

template <int T, int P, bool LDS_XYZ>
int launch_reg_ragged(const float *xyz, const int32_t *offsets, int B, int cap, int n_max, int M, int32_t *idx,
                      hipStream_t st) {
  constexpr int W = T / 64;
  const size_t smem = 16 * (W > 1 ? W : 1) + (LDS_XYZ ? static_cast<size_t>(n_max) * 16 : 0);
  if (smem > 64 * 1024) {
    NSDP_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&fps_reg_ragged_kernel<T, P, LDS_XYZ>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(smem)));
  }
  hipLaunchKernelGGL((fps_reg_ragged_kernel<T, P, LDS_XYZ>), dim3(B), dim3(T), smem, st, xyz, offsets, cap, n_max, M, idx);
  return nsdp::launch_status("fps_reg_ragged_kernel");
}

}  // namespace

extern "C" int nsdp_furthest_point_sampling(const float *xyz, int B, int N, int nsamples, float *tmp,
                                            int32_t *idx_out, void *stream) {
  if (B <= 0 || nsamples <= 0) return 0;
  NSDP_REQUIRE(xyz && idx_out, "fps: null pointer");
  NSDP_REQUIRE(N > 0, "fps: N must be positive (got %d)", N);
  NSDP_REQUIRE((static_cast<long long>(N) >> kRankShift) == 0, "fps: N too large (%d)", N);
  hipStream_t st = nsdp::as_stream(stream);
  nsdp::prof::Scope scope(nsdp::prof::kFps, st, 0.0, static_cast<double>(B) * (12.0 * N + 4.0 * nsamples));
  const int BS = opt_n_threads(N);
  int log2BS = 0;
  while ((1 << log2BS) < BS) ++log2BS;
  if (N <= 512) return launch_reg<64, 8, true>(xyz, B, N, nsamples, BS, log2BS, idx_out, st);
  if (N <= 2048) return launch_reg<256, 8, true>(xyz, B, N, nsamples, BS, log2BS, idx_out, st);
  if (N <= 4096) return launch_reg<512, 8, true>(xyz, B, N, nsamples, BS, log2BS, idx_out, st);
  if (N <= 8192) return launch_reg<1024, 8, false>(xyz, B, N, nsamples, BS, log2BS, idx_out, st);
  NSDP_REQUIRE(tmp, "fps: N=%d > 8192 needs the (B,N) scratch buffer", N);
  hipLaunchKernelGGL((fps_big_kernel<1024>), dim3(B), dim3(1024), 0, st, xyz, tmp, N, nsamples, BS,
                     log2BS, idx_out);
  return nsdp::launch_status("fps_big_kernel");
}

extern "C" int nsdp_furthest_point_sampling_ragged(const float *xyz_packed, const int32_t *offsets, int B, int cap, int n_max,
                                                   int nsamples, float *tmp, int32_t *idx_out, void *stream) {
  if (B <= 0) return 0;
  NSDP_REQUIRE(nsamples > 0, "fps_ragged: nsamples must be positive (got %d)", nsamples);
  NSDP_REQUIRE(xyz_packed && offsets && idx_out, "fps_ragged: null pointer");
  NSDP_REQUIRE(cap > 0 && n_max > 0, "fps_ragged: cap and n_max must be positive (got %d, %d)", cap, n_max);
  NSDP_REQUIRE(B <= 65535, "fps_ragged: batch %d too large for one launch", B);
  n_max = n_max < cap ? n_max : cap;
  NSDP_REQUIRE((static_cast<long long>(n_max) >> kRankShift) == 0, "fps_ragged: n_max too large (%d)", n_max);
  NSDP_REQUIRE(tmp || n_max <= 8192, "fps_ragged: n_max=%d > 8192 needs the (cap) scratch buffer", n_max);
  hipStream_t st = nsdp::as_stream(stream);
  // the number of real rows is known to the device alone: bytes accounted with cap, an upper bound
  nsdp::prof::Scope scope(nsdp::prof::kFps, st, 0.0, 12.0 * cap + 4.0 * static_cast<double>(B) * nsamples);
  if (n_max <= 512) return launch_reg_ragged<64, 8, true>(xyz_packed, offsets, B, cap, n_max, nsamples, idx_out, st);
  if (n_max <= 2048) return launch_reg_ragged<256, 8, true>(xyz_packed, offsets, B, cap, n_max, nsamples, idx_out, st);
  if (n_max <= 4096) return launch_reg_ragged<512, 8, true>(xyz_packed, offsets, B, cap, n_max, nsamples, idx_out, st);
  if (n_max <= 8192) return launch_reg_ragged<1024, 8, false>(xyz_packed, offsets, B, cap, n_max, nsamples, idx_out, st);
  hipLaunchKernelGGL((fps_big_ragged_kernel<1024>), dim3(B), dim3(1024), 0, st, xyz_packed, offsets, tmp, cap, n_max, nsamples,
                     idx_out);
  return nsdp::launch_status("fps_big_ragged_kernel");
}
