// The Chamfer training loss (include/nsdp_chamfer.h): forward = the two nearest-neighbour searches of nsdp_nn_dist2 with
// indices (eval_metric.hip; called, not restated) + the per-shape terms and the scalar loss reduced in double in a fixed order;
// backward = one launch per gradient operand, a gather-reduce over the inverse lists of the opposite direction's index map.
//
// Backward, MI355X design.  A workgroup owns 256 consecutive rows of one shape; a lane owns a row: its point, its nearest
// neighbour's difference and its list's bounds.  What sets the cost is the length T of a row's list -- about 1 for two clouds of
// equal size in general position, every one of the other cloud's rows for collapsed predictions -- so the list sum has three
// forms, picked per row and all inside the one launch:
//   * T <= 32: the lane walks its own list (ascending).  The lanes of a wave diverge by at most 32 iterations;
//   * 32 < T <= 1024: the wave takes the row's list together, lane t entries t, t + 64, ... (each entry index a coalesced read,
//     each point a 12-byte gather) and a butterfly sums the 64 partial sums -- the ballot of such rows is walked in lane order;
//   * T > 1024: the workgroup takes it, thread t entries t, t + 256, ..., and a tree in LDS sums the 256 partial sums; the four
//     waves' ballots of such rows go through LDS, so every thread walks the same rows in the same order (barriers are uniform).
// Every form's order of additions is a function of the list alone (header: the depth of each), nothing is atomic, and a row's
// gradient does not depend on what the rows around it hold.  One workgroup per long list is the bound of this design: a list
// of 100 000 entries is 391 dependent-free gathers per thread, where a lane alone would walk all 100 000.
#include <cfloat>
#include <cmath>

#include "../../include/nsdp_chamfer.h"
#include "../../include/nsdp_eval.h"
#include "common.h"
#include "prof.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kLaneMax = 32;      // the longest list one lane walks alone
constexpr int kWaveMax = 1024;    // the longest list one wave shares; longer ones take the workgroup
constexpr int kMaxBatch = 65535;
constexpr int kMaxPoints = 1 << 20;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// sum over entries [lo, hi) in steps of `stride` from lo + first of (p - y[entry]), in that order
__device__ __forceinline__ void list_sum(const float *__restrict__ y, const int32_t *__restrict__ ent, int n_other, int lo, int hi,
                                         int first, int stride, float px, float py, float pz, float &sx, float &sy, float &sz) {
#pragma unroll 4
  for (int e = lo + first; e < hi; e += stride) {
    const float *q = y + static_cast<size_t>(clampi(ent[e], 0, n_other - 1)) * 3;
    sx += px - q[0];
    sy += py - q[1];
    sz += pz - q[2];
  }
}

// grid (ceil(n_self / 256), B).  offsets_all == NULL: no lists (w_list == 0), the list sum is 0.
__global__ __launch_bounds__(kThreads) void chamfer_backward_kernel(const float *__restrict__ self_all,
                                                                    const float *__restrict__ other_all,
                                                                    const int32_t *__restrict__ idx_all,
                                                                    const int32_t *__restrict__ offsets_all,
                                                                    const int32_t *__restrict__ entries_all,
                                                                    const float *__restrict__ g, int n_self, int n_other,
                                                                    float s_d, float s_l, float *__restrict__ grad_all) {
  __shared__ float red[3][kThreads];
  __shared__ unsigned long long big[kWaves];
  const size_t b = blockIdx.y;
  const float *x = self_all + b * n_self * 3;
  const float *y = other_all + b * n_other * 3;
  const int32_t *off = offsets_all ? offsets_all + b * (static_cast<size_t>(n_self) + 1) : nullptr;
  const int32_t *ent = offsets_all ? entries_all + b * n_other : nullptr;
  const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
  const int row0 = static_cast<int>(blockIdx.x) * kThreads;
  const int i = row0 + tid;
  const bool live = i < n_self;
  float px = 0.f, py = 0.f, pz = 0.f, dx = 0.f, dy = 0.f, dz = 0.f;
  int lo = 0, hi = 0;
  if (live) {
    const float *p = x + static_cast<size_t>(i) * 3;
    px = p[0]; py = p[1]; pz = p[2];
    const float *q = y + static_cast<size_t>(clampi(idx_all[b * n_self + i], 0, n_other - 1)) * 3;
    dx = px - q[0]; dy = py - q[1]; dz = pz - q[2];
    if (off) {
      lo = clampi(off[i], 0, n_other);
      hi = clampi(off[i + 1], lo, n_other);
    }
  }
  const int len = hi - lo;
  float sx = 0.f, sy = 0.f, sz = 0.f;
  if (off) {      // (uniform over the grid)
    if (len <= kLaneMax) list_sum(y, ent, n_other, lo, hi, 0, 1, px, py, pz, sx, sy, sz);
    // rows whose list a wave shares, in lane order (all 64 lanes are here: rows beyond n_self have len 0)
    unsigned long long todo = __ballot(len > kLaneMax && len <= kWaveMax);
    while (todo) {
      const int src = __ffsll(static_cast<long long>(todo)) - 1;
      todo &= todo - 1;
      float ax = 0.f, ay = 0.f, az = 0.f;
      list_sum(y, ent, n_other, __shfl(lo, src), __shfl(hi, src), lane, 64, __shfl(px, src), __shfl(py, src), __shfl(pz, src), ax,
               ay, az);
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
    if (lane == 0) big[wave] = mine;
    __syncthreads();
    for (int w = 0; w < kWaves; ++w) {
      unsigned long long rows = big[w];
      while (rows) {
        const int r = w * 64 + __ffsll(static_cast<long long>(rows)) - 1;      // (set only for rows below n_self)
        rows &= rows - 1;
        const int ri = row0 + r;
        const float *p = x + static_cast<size_t>(ri) * 3;
        const int rlo = clampi(off[ri], 0, n_other), rhi = clampi(off[ri + 1], rlo, n_other);
        float ax = 0.f, ay = 0.f, az = 0.f;
        list_sum(y, ent, n_other, rlo, rhi, tid, kThreads, p[0], p[1], p[2], ax, ay, az);
        red[0][tid] = ax; red[1][tid] = ay; red[2][tid] = az;
        __syncthreads();
        for (int s = kThreads / 2; s > 0; s >>= 1) {
          if (tid < s) {
            red[0][tid] += red[0][tid + s];
            red[1][tid] += red[1][tid + s];
            red[2][tid] += red[2][tid + s];
          }
          __syncthreads();
        }
        if (tid == r) { sx = red[0][0]; sy = red[1][0]; sz = red[2][0]; }
        __syncthreads();      // (red is rewritten by the next row)
      }
    }
  }
  if (live) {
    const float g0 = g[0];
    const float gd = g0 * s_d, gl = g0 * s_l;
    float *out = grad_all + (b * n_self + i) * 3;
    out[0] = gd * dx + gl * sx;
    out[1] = gd * dy + gl * sy;
    out[2] = gd * dz + gl * sz;
  }
}

// fixed tree over the 256 partial sums of a workgroup; the result in part[0] (every thread must call it)
__device__ __forceinline__ void tree_sum(double *part) {
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (static_cast<int>(threadIdx.x) < s) part[threadIdx.x] += part[threadIdx.x + s];
    __syncthreads();
  }
}

// one workgroup per shape: term[b] in double into terms64, rounded once into terms
__global__ __launch_bounds__(kThreads) void chamfer_terms_kernel(const float *__restrict__ dist2_pt, const float *__restrict__ dist2_tp,
                                                                 int n, int m, float w_pt, float w_tp, double *__restrict__ terms64,
                                                                 float *__restrict__ terms) {
  __shared__ double part_pt[kThreads], part_tp[kThreads];
  const size_t b = blockIdx.x;
  const float *a = dist2_pt + b * n, *c = dist2_tp + b * m;
  double acc = 0.0;
  for (int r = threadIdx.x; r < n; r += kThreads) acc += static_cast<double>(a[r]);
  part_pt[threadIdx.x] = acc;
  acc = 0.0;
  for (int r = threadIdx.x; r < m; r += kThreads) acc += static_cast<double>(c[r]);
  part_tp[threadIdx.x] = acc;
  tree_sum(part_pt);
  tree_sum(part_tp);
  if (threadIdx.x == 0) {
    const double t = static_cast<double>(w_pt) * (part_pt[0] / (2.0 * n)) + static_cast<double>(w_tp) * (part_tp[0] / (2.0 * m));
    terms64[b] = t;
    terms[b] = static_cast<float>(t);
  }
}

// one workgroup: the mean of the B doubles, rounded once
__global__ __launch_bounds__(kThreads) void chamfer_loss_kernel(const double *__restrict__ terms64, int B, float *__restrict__ loss) {
  __shared__ double part[kThreads];
  double acc = 0.0;
  for (int b = threadIdx.x; b < B; b += kThreads) acc += terms64[b];
  part[threadIdx.x] = acc;
  tree_sum(part);
  if (threadIdx.x == 0) loss[0] = static_cast<float>(part[0] / static_cast<double>(B));
}

bool finite_weight(float w) { return w == w && std::fabs(w) <= FLT_MAX; }

}  // namespace

extern "C" size_t nsdp_chamfer_forward_workspace_bytes(int B) {
  return B >= 1 && B <= kMaxBatch ? static_cast<size_t>(B) * sizeof(double) : 0;
}

#define CHAMFER_SIZES(name, B, n, m)                                                                                          \
  NSDP_REQUIRE((B) >= 1 && (B) <= kMaxBatch, name ": batch %d must be in [1, %d]", (B), kMaxBatch);                           \
  NSDP_REQUIRE((n) >= 1 && (n) <= kMaxPoints, name ": n=%d points per shape must be in [1, %d]", (n), kMaxPoints);           \
  NSDP_REQUIRE((m) >= 1 && (m) <= kMaxPoints, name ": m=%d points per shape must be in [1, %d]", (m), kMaxPoints);           \
  NSDP_REQUIRE(static_cast<long long>(B) * ((n) > (m) ? (n) : (m)) < (1LL << 31), name ": %d x %d rows too large (B * max(n, m) < 2^31)", \
               (B), (n) > (m) ? (n) : (m))

extern "C" int nsdp_chamfer_forward(const float *pred, const float *target, int B, int n, int m, float w_pt, float w_tp,
                                    void *workspace, float *dist2_pt, int32_t *idx_pt, float *dist2_tp, int32_t *idx_tp,
                                    float *terms, float *loss, void *stream) {
  CHAMFER_SIZES("chamfer_forward", B, n, m);
  NSDP_REQUIRE(finite_weight(w_pt) && finite_weight(w_tp), "chamfer_forward: the weights must be finite");
  NSDP_REQUIRE(pred && target && workspace && dist2_pt && idx_pt && dist2_tp && idx_tp && terms && loss,
               "chamfer_forward: null pointer");
  NSDP_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "chamfer_forward: the workspace must be 8-byte aligned");
  hipStream_t st = nsdp::as_stream(stream);
  int rc;
  if ((rc = nsdp_nn_dist2(pred, target, B, n, m, dist2_pt, idx_pt, stream))) return rc;
  if ((rc = nsdp_nn_dist2(target, pred, B, m, n, dist2_tp, idx_tp, stream))) return rc;
  double *terms64 = static_cast<double *>(workspace);
  hipLaunchKernelGGL(chamfer_terms_kernel, dim3(B), dim3(kThreads), 0, st, dist2_pt, dist2_tp, n, m, w_pt, w_tp, terms64, terms);
  if ((rc = nsdp::launch_status("chamfer_terms_kernel"))) return rc;
  hipLaunchKernelGGL(chamfer_loss_kernel, dim3(1), dim3(kThreads), 0, st, terms64, B, loss);
  return nsdp::launch_status("chamfer_loss_kernel");
}

extern "C" int nsdp_chamfer_backward(const float *self, const float *other, const int32_t *idx_self, const int32_t *offsets,
                                     const int32_t *entries, const float *g, int B, int n_self, int n_other, float w_direct,
                                     float w_list, float *grad, void *stream) {
  CHAMFER_SIZES("chamfer_backward", B, n_self, n_other);
  NSDP_REQUIRE(finite_weight(w_direct) && finite_weight(w_list), "chamfer_backward: the weights must be finite");
  NSDP_REQUIRE(self && other && idx_self && g && grad, "chamfer_backward: null pointer");
  const bool lists = w_list != 0.f;
  NSDP_REQUIRE(!lists || (offsets && entries), "chamfer_backward: null pointer (a non-zero list weight needs offsets and entries)");
  const float s_d = static_cast<float>(static_cast<double>(w_direct) / (static_cast<double>(B) * n_self));
  const float s_l = static_cast<float>(static_cast<double>(w_list) / (static_cast<double>(B) * n_other));
  NSDP_TRACE("chamfer_backward<lists=%d>", lists ? 1 : 0);
  hipLaunchKernelGGL(chamfer_backward_kernel, dim3(nsdp::ceil_div(n_self, kThreads), B), dim3(kThreads), 0, nsdp::as_stream(stream),
                     self, other, idx_self, lists ? offsets : nullptr, lists ? entries : nullptr, g, n_self, n_other, s_d, s_l, grad);
  return nsdp::launch_status("chamfer_backward_kernel");
}
