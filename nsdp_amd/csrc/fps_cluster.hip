// Farthest-point sampling of a large cloud by a cluster of workgroups (include/nsdp_sampling.h).
//
// fps.hip keeps a cloud of up to 8192 points in the registers of one workgroup (1024 lanes x 8 points); a larger cloud falls
// to a kernel that re-reads 16 bytes per point from memory at every dependent step, on one compute unit.  Here the cloud is
// cut into G slices of 8192 consecutive points, slice g register-resident in workgroup (g, cloud) exactly as fps_reg_body
// holds a whole cloud, and the G workgroups agree on each step's winner by exchanging one 8-byte key each:
//   * the key is fps_common.h's {bits(min-dist) : tie priority} with BS = opt_n_threads(N) of the WHOLE cloud, whose signed
//     maximum is a maximum over all points whatever the partition -- the winners are those of the single-workgroup kernels,
//     ties included, for every G;
//   * exchange (MI355X hand-off by data-tagged granules, 8-byte agent-scope atomics on both sides, no fence): every step j
//     of cloud b has G granules keys[b][j][g] of its own, filled with 0xFF bytes by a memset in front of the launch.  A
//     key's high word is the bits of a non-negative float or of -1.0f, so no key equals the fill.  Workgroup g publishes its
//     maximum with one atomic store; its wave 0 polls the G granules, lane i on granule i, with relaxed agent-scope loads
//     until none holds the fill, takes their maximum and hands it to the other 15 waves through LDS behind a barrier.  No slot
//     is reused within a call: no generation counting, no stale line;
//   * the winner's coordinates are a plain load from the input cloud, which nobody writes.
//
// Residency.  The G workgroups of a cloud wait for each other, so all of them must get a compute unit while the others hold
// theirs.  The host launches at most num_cus() workgroups at a time (a batch of more clouds goes out as consecutive launches
// on the stream) and a workgroup needs 1024 threads, 90 vector registers per lane and 264 bytes of LDS (the compiler's figures
// for gfx950), so every compute unit admits at least one.  The dispatcher places workgroups in order as room appears and a
// resident workgroup never waits for room: whatever else occupies the device (kernels of other streams) finishes without help
// from this launch, after which the launch's not-yet-resident workgroups fit beside its resident ones.  The launch cannot
// wait on itself.  What the argument does not cover is several such launches from different streams at once (the parallel
// branches of a captured step with two encoders at a large batch), each holding part of the device while its remaining
// workgroups wait for room the others hold.  The bound below then ends the waits: the kernel completes about one limit late
// with the status word set and wrong -- in-range -- indices, and never hangs.  Nothing but nsdp_fps_cluster_status reveals
// that, so whoever runs cluster calls concurrently reads it where they synchronise (pointnet2_utils.fps_cluster_status checks
// every stream's latest call; nsdp_amd.infer does so behind its timed loops).
//
// No spin without an end.  A poll that does not find every granule on its first pass sleeps (s_sleep) between passes, reads
// the status word with every pass and the constant-rate clock (100 MHz), and gives up after kWaitTicks = 2 s or as soon as
// the status word is set.  Giving up is latched: the workgroup polls once per step for the rest of the launch and carries on
// with the best key present (its own at least).  Every index written is a decoded key clamped to [0, N).
#include "common.h"
#include "fps_common.h"
#include "prof.h"

#include "../../include/nsdp_sampling.h"

#pragma clang fp contract(off)

namespace {

using namespace nsdp::fps;

constexpr int kThreads = 1024, kPoints = 8, kSlice = kThreads * kPoints;   // one workgroup's slice: 8192 points
constexpr int kMaxGroups = 32;
constexpr int kHeadBytes = 16;                        // the status word's block, in front of the granules
constexpr unsigned kStatusClean = 0xFFFFFFFFu;        // (the one memset fills status word and granules alike)
constexpr unsigned long long kFill = ~0ull;
constexpr long long kWaitTicks = 200000000ll;         // 2 s of wall_clock64()

typedef __attribute__((address_space(1))) unsigned long long gu64;
typedef __attribute__((address_space(1))) unsigned gu32;

__device__ __forceinline__ unsigned long long load_granule(unsigned long long *p) {
  return __hip_atomic_load((gu64 *)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ unsigned load_status(unsigned *p) {
  return __hip_atomic_load((gu32 *)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Wave 0 of workgroup g: publish `mine`, gather the cloud's G keys of this step, return their maximum (in every lane).
// `gave_up` is wave-uniform and latched by the caller's variable.
__device__ __forceinline__ long long exchange_max(unsigned long long *kj, int G, int g, int lane, long long mine,
                                                  unsigned *status, bool &gave_up) {
  // lane g stores and later loads its own granule: a thread sees its own store
  if (lane == g)
    __hip_atomic_store((gu64 *)(kj + g), static_cast<unsigned long long>(mine), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  const bool polls = lane < G && lane != g;
  unsigned long long x = polls ? load_granule(kj + lane) : static_cast<unsigned long long>(mine);
  if (!gave_up && __any(polls && x == kFill)) {
    const long long t0 = wall_clock64();
    for (;;) {
      __builtin_amdgcn_s_sleep(2);
      if (polls) x = load_granule(kj + lane);
      const unsigned word = load_status(status);
      if (!__any(polls && x == kFill)) break;
      if (__any(word != kStatusClean)) { gave_up = true; break; }
      if (wall_clock64() - t0 > kWaitTicks) {
        if (lane == 0)
          __hip_atomic_store((gu32 *)status, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        gave_up = true;
        break;
      }
    }
  }
  // (a granule still unpublished after a give-up does not take part; lanes beyond G hold this workgroup's own key)
  const long long v = (polls && x == kFill) ? mine : static_cast<long long>(x);
  return wave_max_i64(v);
}

// Slice g of one cloud, by one workgroup of the cloud's cluster.  keys: this cloud's [M][G] granules.
__device__ __forceinline__ void fps_cluster_body(const float *__restrict__ xyz, int N, int M, int BS, int log2BS, int G, int g,
                                                 unsigned long long *keys, unsigned *status, int32_t *__restrict__ out,
                                                 int base) {
  constexpr int T = kThreads, P = kPoints, W = T / 64;
  __shared__ long long slots[2 * W];
  __shared__ long long winner;
  const int tid = threadIdx.x;

  float px[P], py[P], pz[P], pt[P];
  unsigned prio[P];
#pragma unroll
  for (int s = 0; s < P; ++s) init_point(xyz, g * kSlice + tid + s * T, N, BS, log2BS, px[s], py[s], pz[s], pt[s], prio[s]);
  if (g == 0 && tid == 0) out[0] = base;
  float cx = xyz[0], cy = xyz[1], cz = xyz[2];
  bool gave_up = false;

  for (int j = 1; j < M; ++j) {
    long long best = wave_max_i64(update_points<P>(px, py, pz, pt, prio, cx, cy, cz));
    best = block_max_i64<W>(slots, j, tid, best);
    if (tid < 64) {   // wave 0
      const long long all = exchange_max(keys + static_cast<size_t>(j) * G, G, g, tid, best, status, gave_up);
      if (tid == 0) winner = all;
    }
    __syncthreads();
    // (the next write of `winner` comes behind the next step's barrier in block_max_i64: every wave has read it by then)
    const int old = max(min(decode_winner(winner, log2BS), N - 1), 0);
    cx = xyz[old * 3 + 0]; cy = xyz[old * 3 + 1]; cz = xyz[old * 3 + 2];
    if (g == 0 && tid == 0) out[j] = base + old;
  }
}

// grid (G, clouds of this launch); b0: the first cloud of this launch within the batch
__global__ __launch_bounds__(kThreads) void fps_cluster_kernel(const float *__restrict__ xyz_all, int b0, int N, int M, int BS,
                                                               int log2BS, void *workspace, int32_t *__restrict__ idx_all) {
  const int G = gridDim.x, g = blockIdx.x;
  const size_t b = static_cast<size_t>(b0) + blockIdx.y;
  unsigned *status = reinterpret_cast<unsigned *>(workspace);
  unsigned long long *keys = reinterpret_cast<unsigned long long *>(static_cast<char *>(workspace) + kHeadBytes) + b * M * G;
  fps_cluster_body(xyz_all + b * N * 3, N, M, BS, log2BS, G, g, keys, status, idx_all + b * M, 0);
}

__global__ __launch_bounds__(kThreads) void fps_cluster_ragged_kernel(const float *__restrict__ xyz_packed,
                                                                      const int32_t *__restrict__ offsets, int b0, int cap,
                                                                      int n_max, int M, void *workspace,
                                                                      int32_t *__restrict__ idx_all) {
  const int G = gridDim.x, g = blockIdx.x;
  const int shape = b0 + static_cast<int>(blockIdx.y);
  int32_t *out = idx_all + static_cast<size_t>(shape) * M;
  int lo, N, BS, log2BS;
  // (every workgroup of the cluster sees the same N: an empty shape ends all of them before any wait; workgroup 0 fills)
  if (!fps_ragged_shape(offsets, shape, cap, min(n_max, G * kSlice), M, g == 0 ? out : nullptr, lo, N, BS, log2BS)) return;
  unsigned *status = reinterpret_cast<unsigned *>(workspace);
  unsigned long long *keys =
      reinterpret_cast<unsigned long long *>(static_cast<char *>(workspace) + kHeadBytes) + static_cast<size_t>(shape) * M * G;
  fps_cluster_body(xyz_packed + static_cast<size_t>(lo) * 3, N, M, BS, log2BS, G, g, keys, status, out, lo);
}

int default_groups(int n_max) {
  if (n_max <= kSlice || n_max > kMaxGroups * kSlice) return 0;
  return (n_max + kSlice - 1) / kSlice;
}

size_t workspace_bytes(long long B, long long M, long long G) {
  const size_t granules = static_cast<size_t>(B) * M * G * 8;
  return kHeadBytes + (granules + 15) / 16 * 16;
}

// clouds per launch: every workgroup of a launch holds a compute unit while it waits for the others
int clouds_per_launch(int G) {
  const int per = nsdp::num_cus() / G;
  return per > 0 ? per : 1;
}

}  // namespace

extern "C" int nsdp_fps_cluster_groups(int n_max) { return default_groups(n_max); }

extern "C" size_t nsdp_fps_cluster_workspace_bytes(int B, int n_max, int nsamples, int groups) {
  const int G = groups ? groups : default_groups(n_max);
  if (B <= 0 || n_max <= 0 || nsamples <= 0 || G < 1 || G > kMaxGroups || n_max > static_cast<long long>(G) * kSlice) return 0;
  return workspace_bytes(B, nsamples, G);
}

extern "C" int nsdp_furthest_point_sampling_cluster(const float *xyz, int B, int N, int nsamples, int groups, void *workspace,
                                                    int32_t *idx_out, void *stream) {
  if (B <= 0 || nsamples <= 0) return 0;
  NSDP_REQUIRE(xyz && idx_out && workspace, "fps_cluster: null pointer");
  NSDP_REQUIRE(N > 0, "fps_cluster: N must be positive (got %d)", N);
  NSDP_REQUIRE(groups >= 0 && groups <= kMaxGroups, "fps_cluster: groups must be 0 (default) or 1..%d (got %d)", kMaxGroups, groups);
  const int G = groups ? groups : default_groups(N);
  NSDP_REQUIRE(G > 0, "fps_cluster: no default cluster for N=%d (served by default: %d < N <= %d); pass groups", N, kSlice,
               kMaxGroups * kSlice);
  NSDP_REQUIRE(N <= G * kSlice, "fps_cluster: groups=%d too small for N=%d (%d points per workgroup)", G, N, kSlice);
  NSDP_REQUIRE(B <= 65535, "fps_cluster: batch %d too large", B);
  hipStream_t st = nsdp::as_stream(stream);
  nsdp::prof::Scope scope(nsdp::prof::kFps, st, 0.0, static_cast<double>(B) * (12.0 * N + 4.0 * nsamples + 16.0 * nsamples * G));
  const int BS = opt_n_threads(N);
  int log2BS = 0;
  while ((1 << log2BS) < BS) ++log2BS;
  NSDP_HIP_TRY(hipMemsetAsync(workspace, 0xFF, workspace_bytes(B, nsamples, G), st));
  const int per = clouds_per_launch(G);
  for (int b0 = 0; b0 < B; b0 += per) {
    const int nb = B - b0 < per ? B - b0 : per;
    hipLaunchKernelGGL(fps_cluster_kernel, dim3(G, nb), dim3(kThreads), 0, st, xyz, b0, N, nsamples, BS, log2BS, workspace,
                       idx_out);
    const int rc = nsdp::launch_status("fps_cluster_kernel");
    if (rc) return rc;
  }
  return 0;
}

extern "C" int nsdp_furthest_point_sampling_cluster_ragged(const float *xyz_packed, const int32_t *offsets, int B, int cap,
                                                           int n_max, int nsamples, int groups, void *workspace,
                                                           int32_t *idx_out, void *stream) {
  if (B <= 0) return 0;
  NSDP_REQUIRE(nsamples > 0, "fps_cluster_ragged: nsamples must be positive (got %d)", nsamples);
  NSDP_REQUIRE(xyz_packed && offsets && idx_out && workspace, "fps_cluster_ragged: null pointer");
  NSDP_REQUIRE(cap > 0 && n_max > 0, "fps_cluster_ragged: cap and n_max must be positive (got %d, %d)", cap, n_max);
  NSDP_REQUIRE(B <= 65535, "fps_cluster_ragged: batch %d too large", B);
  NSDP_REQUIRE(groups >= 0 && groups <= kMaxGroups, "fps_cluster_ragged: groups must be 0 (default) or 1..%d (got %d)", kMaxGroups,
               groups);
  n_max = n_max < cap ? n_max : cap;
  const int G = groups ? groups : default_groups(n_max);
  NSDP_REQUIRE(G > 0, "fps_cluster_ragged: no default cluster for n_max=%d (served by default: %d < n_max <= %d); pass groups",
               n_max, kSlice, kMaxGroups * kSlice);
  NSDP_REQUIRE(n_max <= G * kSlice, "fps_cluster_ragged: groups=%d too small for n_max=%d (%d points per workgroup)", G, n_max,
               kSlice);
  hipStream_t st = nsdp::as_stream(stream);
  nsdp::prof::Scope scope(nsdp::prof::kFps, st, 0.0, 12.0 * cap + static_cast<double>(B) * nsamples * (4.0 + 16.0 * G));
  NSDP_HIP_TRY(hipMemsetAsync(workspace, 0xFF, workspace_bytes(B, nsamples, G), st));
  const int per = clouds_per_launch(G);
  for (int b0 = 0; b0 < B; b0 += per) {
    const int nb = B - b0 < per ? B - b0 : per;
    hipLaunchKernelGGL(fps_cluster_ragged_kernel, dim3(G, nb), dim3(kThreads), 0, st, xyz_packed, offsets, b0, cap, n_max,
                       nsamples, workspace, idx_out);
    const int rc = nsdp::launch_status("fps_cluster_ragged_kernel");
    if (rc) return rc;
  }
  return 0;
}

extern "C" int nsdp_fps_cluster_status(const void *workspace, void *stream) {
  NSDP_REQUIRE(workspace, "fps_cluster_status: null workspace");
  hipStream_t st = nsdp::as_stream(stream);
  unsigned word = 0;
  NSDP_HIP_TRY(hipMemcpyAsync(&word, workspace, sizeof(word), hipMemcpyDeviceToHost, st));
  NSDP_HIP_TRY(hipStreamSynchronize(st));
  if (word == kStatusClean) return 0;
  nsdp::set_error("fps_cluster: a wait between the workgroups of a cloud gave up (status word 0x%08x); the indices of that call "
                  "are not to be trusted", word);
  return NSDP_ETIMEOUT;
}
