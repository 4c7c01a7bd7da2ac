// The Chamfer training loss (include/nsdp_chamfer.h): forward = the two nearest-neighbour searches of nsdp_nn_dist2 with
// indices (eval_metric.hip; called, not restated) + the per-shape terms and the scalar loss reduced in double in a fixed order;
// backward = one launch per gradient operand, a gather-reduce over the inverse lists of the opposite direction's index map.
//
// Backward, MI355X design.  A workgroup owns 256 consecutive rows of one shape; a lane owns a row: its point, its nearest
// neighbour's difference and its list's bounds.  The list sum is csrc/list_reduce.h's (its three forms, their operation order and
// depth are documented there); the term of an entry is p - y[entry].
#include "../../include/nsdp_chamfer.h"
#include "../../include/nsdp_eval.h"
#include "common.h"
#include "list_reduce.h"
#include "prof.h"

#pragma clang fp contract(off)

namespace {

using namespace nsdp::lists;      // kThreads, clampi, reduce, tree_sum

constexpr int kMaxBatch = 65535;
constexpr int kMaxPoints = 1 << 20;

// the term of a list entry: p - y[entry]
struct OtherPoint {
  const float *__restrict__ y;
  const int32_t *__restrict__ ent;
  int n_other;
  __device__ __forceinline__ void add(int slot, float px, float py, float pz, float &sx, float &sy, float &sz) const {
    const float *q = y + static_cast<size_t>(clampi(ent[slot], 0, n_other - 1)) * 3;
    sx += px - q[0];
    sy += py - q[1];
    sz += pz - q[2];
  }
};

// grid (ceil(n_self / 256), B).  offsets_all == NULL: no lists (w_list == 0), the list sum is 0.
__global__ __launch_bounds__(kThreads) void chamfer_backward_kernel(const float *__restrict__ self_all,
                                                                    const float *__restrict__ other_all,
                                                                    const int32_t *__restrict__ idx_all,
                                                                    const int32_t *__restrict__ offsets_all,
                                                                    const int32_t *__restrict__ entries_all,
                                                                    const float *__restrict__ g, int n_self, int n_other,
                                                                    float s_d, float s_l, float *__restrict__ grad_all) {
  __shared__ Shared shared;
  const size_t b = blockIdx.y;
  const float *x = self_all + b * n_self * 3;
  const float *y = other_all + b * n_other * 3;
  const int32_t *off = offsets_all ? offsets_all + b * (static_cast<size_t>(n_self) + 1) : nullptr;
  const int32_t *ent = offsets_all ? entries_all + b * n_other : nullptr;
  const int row0 = static_cast<int>(blockIdx.x) * kThreads;
  const int i = row0 + static_cast<int>(threadIdx.x);
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
  float sx = 0.f, sy = 0.f, sz = 0.f;
  if (off)      // (uniform over the grid: every thread of the workgroup calls it)
    reduce(OtherPoint{y, ent, n_other}, x, off, n_other, row0, lo, hi, px, py, pz, shared, sx, sy, sz);
  if (live) {
    const float g0 = g[0];
    const float gd = g0 * s_d, gl = g0 * s_l;
    float *out = grad_all + (b * n_self + i) * 3;
    out[0] = gd * dx + gl * sx;
    out[1] = gd * dy + gl * sy;
    out[2] = gd * dz + gl * sz;
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
  NSDP_REQUIRE(nsdp::finite_weight(w_pt) && nsdp::finite_weight(w_tp), "chamfer_forward: the weights must be finite");
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
  NSDP_REQUIRE(nsdp::finite_weight(w_direct) && nsdp::finite_weight(w_list), "chamfer_backward: the weights must be finite");
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
