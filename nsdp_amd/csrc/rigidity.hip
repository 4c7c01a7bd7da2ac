// The local-rigidity training regulariser (include/nsdp_rigidity.h): forward = the residuals r = |p_i - p_l|^2 - |s_i - s_l|^2 of
// every neighbour edge, the per-shape terms (slice sums, then their sum) and the scalar loss reduced in double in a fixed order;
// backward = one launch, the lane's own K columns plus a gather-reduce over the inverse lists of the neighbour sets.
//
// MI355X design.  Forward: a lane owns a point -- its p, its s, its K indices -- and gathers K rows of either cloud (12-byte
// gathers; a shape's two clouds are 96 KB each at 8192 points, so they are served from L2) and writes its K residuals side by
// side.  Backward: a workgroup owns 256 consecutive rows of one shape, a lane a row.  The own-columns sum is K gathers per lane.
// What sets the cost of the other half is the in-degree T of a row -- about K for a cloud in general position, of the order of m
// for the lowest-index rows of m duplicates -- so the list sum is csrc/list_reduce.h's, the one the Chamfer backward calls (its
// three forms, their operation order and depth are documented there); the term of an entry e is r_e (p - x[e div K]).
#include "../../include/nsdp_rigidity.h"
#include "common.h"
#include "list_reduce.h"
#include "prof.h"

#pragma clang fp contract(off)

namespace {

using namespace nsdp::lists;      // kThreads, clampi, reduce, tree_sum

constexpr int kMaxBatch = 65535;
constexpr int kMaxPoints = 1 << 20;
constexpr int kMaxK = 32;
constexpr int kMaxEntries = 1 << 25;      // n * K: the bound of the list build
constexpr int kMaxSlices = 64;            // workgroups that share the sum of a shape's squared residuals

// grid (ceil(n / 256), B): resid[b,i,j] = |p_i - p_l|^2 - |s_i - s_l|^2, l = idx[b,i,j]
__global__ __launch_bounds__(kThreads) void rigidity_resid_kernel(const float *__restrict__ pred_all, const float *__restrict__ src_all,
                                                                  const int32_t *__restrict__ idx_all, int n, int K,
                                                                  float *__restrict__ resid_all) {
  const size_t b = blockIdx.y;
  const int i = static_cast<int>(blockIdx.x) * kThreads + static_cast<int>(threadIdx.x);
  if (i >= n) return;
  const float *p = pred_all + b * n * 3, *s = src_all + b * n * 3;
  const size_t row = (b * n + i) * K;
  const int32_t *nb = idx_all + row;
  float *out = resid_all + row;
  const float px = p[static_cast<size_t>(i) * 3], py = p[static_cast<size_t>(i) * 3 + 1], pz = p[static_cast<size_t>(i) * 3 + 2];
  const float qx = s[static_cast<size_t>(i) * 3], qy = s[static_cast<size_t>(i) * 3 + 1], qz = s[static_cast<size_t>(i) * 3 + 2];
#pragma unroll 4
  for (int j = 0; j < K; ++j) {
    const size_t l = static_cast<size_t>(clampi(nb[j], 0, n - 1)) * 3;
    const float cur = nsdp::sq_dist3(px, py, pz, p[l], p[l + 1], p[l + 2]);
    const float rest = nsdp::sq_dist3(qx, qy, qz, s[l], s[l + 1], s[l + 2]);
    out[j] = cur - rest;
  }
}

// slices of a shape's rows, each summed by a workgroup of its own: one workgroup per shape walks n K values in a dependent chain
// of double additions (measured: 0.43 ms at 4 x 100 000 x 8, more than the rest of the forward and the backward together)
__host__ __device__ inline int term_slices(int n) {
  const int s = (n + kThreads - 1) / kThreads;
  return s < 1 ? 1 : (s > kMaxSlices ? kMaxSlices : s);
}

// grid (term_slices(n), B): partial[b][s] = sum of r^2 over rows [s R, (s + 1) R) of shape b, R = ceil(n / slices), in double
__global__ __launch_bounds__(kThreads) void rigidity_slice_kernel(const float *__restrict__ resid_all, int n, int K,
                                                                  double *__restrict__ partial) {
  __shared__ double part[kThreads];
  const size_t b = blockIdx.y;
  const int slices = static_cast<int>(gridDim.x), per = (n + slices - 1) / slices;
  const int lo = static_cast<int>(blockIdx.x) * per, hi = lo + per < n ? lo + per : n;
  const float *r = resid_all + b * n * K;
  double acc = 0.0;
  for (int row = lo + static_cast<int>(threadIdx.x); row < hi; row += kThreads) {
    const float *q = r + static_cast<size_t>(row) * K;
    for (int j = 0; j < K; ++j) {
      const double v = static_cast<double>(q[j]);
      acc += v * v;
    }
  }
  part[threadIdx.x] = acc;
  tree_sum(part);
  if (threadIdx.x == 0) partial[b * kMaxSlices + blockIdx.x] = part[0];
}

// one workgroup per shape: term[b] = (sum of the slice sums) / (4 n K) in double into terms64, rounded once into terms; the
// slots of partial beyond the shape's slices are written 0 (every workspace byte is written)
__global__ __launch_bounds__(kThreads) void rigidity_terms_kernel(double *__restrict__ partial, int slices, int n, int K,
                                                                  double *__restrict__ terms64, float *__restrict__ terms) {
  __shared__ double part[kThreads];
  const size_t b = blockIdx.x;
  const int t = static_cast<int>(threadIdx.x);
  double v = 0.0;
  if (t < slices) v = partial[b * kMaxSlices + t];
  else if (t < kMaxSlices) partial[b * kMaxSlices + t] = 0.0;
  part[t] = v;
  tree_sum(part);
  if (t == 0) {
    const double term = part[0] / (4.0 * static_cast<double>(n) * static_cast<double>(K));
    terms64[b] = term;
    terms[b] = static_cast<float>(term);
  }
}

// one workgroup: w * the mean of the B doubles, rounded once
__global__ __launch_bounds__(kThreads) void rigidity_loss_kernel(const double *__restrict__ terms64, int B, float w,
                                                                 float *__restrict__ loss) {
  __shared__ double part[kThreads];
  double acc = 0.0;
  for (int b = threadIdx.x; b < B; b += kThreads) acc += terms64[b];
  part[threadIdx.x] = acc;
  tree_sum(part);
  if (threadIdx.x == 0) loss[0] = static_cast<float>(static_cast<double>(w) * (part[0] / static_cast<double>(B)));
}

// the term of a list entry e: r_e * (p - x[e div K])
struct WeightedEdge {
  const float *__restrict__ x;
  const float *__restrict__ r;
  const int32_t *__restrict__ ent;
  int E, K;
  __device__ __forceinline__ void add(int slot, float px, float py, float pz, float &sx, float &sy, float &sz) const {
    const int e = clampi(ent[slot], 0, E - 1);
    const float re = r[e];
    const float *q = x + static_cast<size_t>(e / K) * 3;
    sx += re * (px - q[0]);
    sy += re * (py - q[1]);
    sz += re * (pz - q[2]);
  }
};

// grid (ceil(n / 256), B)
__global__ __launch_bounds__(kThreads) void rigidity_backward_kernel(const float *__restrict__ pred_all, const int32_t *__restrict__ idx_all,
                                                                     const float *__restrict__ resid_all,
                                                                     const int32_t *__restrict__ offsets_all,
                                                                     const int32_t *__restrict__ entries_all, const float *__restrict__ g,
                                                                     int n, int K, float c, float *__restrict__ grad_all) {
  __shared__ Shared shared;
  const size_t b = blockIdx.y;
  const int E = n * K;      // (<= 2^25)
  const float *x = pred_all + b * n * 3;
  const float *r = resid_all + b * E;
  const int32_t *off = offsets_all + b * (static_cast<size_t>(n) + 1);
  const int32_t *ent = entries_all + b * E;
  const int row0 = static_cast<int>(blockIdx.x) * kThreads;
  const int i = row0 + static_cast<int>(threadIdx.x);
  const bool live = i < n;
  float px = 0.f, py = 0.f, pz = 0.f, ox = 0.f, oy = 0.f, oz = 0.f;
  int lo = 0, hi = 0;
  if (live) {
    const float *p = x + static_cast<size_t>(i) * 3;
    px = p[0]; py = p[1]; pz = p[2];
    const size_t row = static_cast<size_t>(i) * K;
    const int32_t *nb = idx_all + b * E + row;
    const float *rr = r + row;
#pragma unroll 4
    for (int j = 0; j < K; ++j) {      // the own columns, in column order
      const float *q = x + static_cast<size_t>(clampi(nb[j], 0, n - 1)) * 3;
      const float rj = rr[j];
      ox += rj * (px - q[0]);
      oy += rj * (py - q[1]);
      oz += rj * (pz - q[2]);
    }
    lo = clampi(off[i], 0, E);
    hi = clampi(off[i + 1], lo, E);
  }
  float sx, sy, sz;
  reduce(WeightedEdge{x, r, ent, E, K}, x, off, E, row0, lo, hi, px, py, pz, shared, sx, sy, sz);
  if (live) {
    const float gc = g[0] * c;
    float *out = grad_all + (b * n + i) * 3;
    out[0] = gc * (ox + sx);
    out[1] = gc * (oy + sy);
    out[2] = gc * (oz + sz);
  }
}

}  // namespace

extern "C" size_t nsdp_rigidity_forward_workspace_bytes(int B) {
  return B >= 1 && B <= kMaxBatch ? static_cast<size_t>(B) * (1 + kMaxSlices) * sizeof(double) : 0;
}

#define RIGIDITY_SIZES(name, B, n, K)                                                                                         \
  NSDP_REQUIRE((B) >= 1 && (B) <= kMaxBatch, name ": batch %d must be in [1, %d]", (B), kMaxBatch);                           \
  NSDP_REQUIRE((n) >= 1 && (n) <= kMaxPoints, name ": n=%d points per shape must be in [1, %d]", (n), kMaxPoints);           \
  NSDP_REQUIRE((K) >= 1 && (K) <= kMaxK, name ": K=%d neighbours per point must be in [1, %d]", (K), kMaxK);                 \
  NSDP_REQUIRE(static_cast<long long>(n) * (K) <= kMaxEntries, name ": n * K = %lld entries per shape exceed the list build's %d", \
               static_cast<long long>(n) * (K), kMaxEntries);                                                                 \
  NSDP_REQUIRE(static_cast<long long>(B) * (n) * (K) < (1LL << 31), name ": %d x %d x %d entries too large (B * n * K < 2^31)", (B), \
               (n), (K))

extern "C" int nsdp_rigidity_forward(const float *pred, const float *source, const int32_t *idx, int B, int n, int K, float w,
                                     void *workspace, float *resid, float *terms, float *loss, void *stream) {
  RIGIDITY_SIZES("rigidity_forward", B, n, K);
  NSDP_REQUIRE(nsdp::finite_weight(w), "rigidity_forward: the weight must be finite");
  NSDP_REQUIRE(pred && source && idx && workspace && resid && terms && loss, "rigidity_forward: null pointer");
  NSDP_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "rigidity_forward: the workspace must be 8-byte aligned");
  hipStream_t st = nsdp::as_stream(stream);
  int rc;
  NSDP_TRACE("rigidity_forward<K=%d>", K);
  hipLaunchKernelGGL(rigidity_resid_kernel, dim3(nsdp::ceil_div(n, kThreads), B), dim3(kThreads), 0, st, pred, source, idx, n, K, resid);
  if ((rc = nsdp::launch_status("rigidity_resid_kernel"))) return rc;
  double *terms64 = static_cast<double *>(workspace), *partial = terms64 + B;      // terms64[B], partial[B][kMaxSlices]
  const int slices = term_slices(n);
  hipLaunchKernelGGL(rigidity_slice_kernel, dim3(slices, B), dim3(kThreads), 0, st, resid, n, K, partial);
  if ((rc = nsdp::launch_status("rigidity_slice_kernel"))) return rc;
  hipLaunchKernelGGL(rigidity_terms_kernel, dim3(B), dim3(kThreads), 0, st, partial, slices, n, K, terms64, terms);
  if ((rc = nsdp::launch_status("rigidity_terms_kernel"))) return rc;
  hipLaunchKernelGGL(rigidity_loss_kernel, dim3(1), dim3(kThreads), 0, st, terms64, B, w, loss);
  return nsdp::launch_status("rigidity_loss_kernel");
}

extern "C" int nsdp_rigidity_backward(const float *pred, const int32_t *idx, const float *resid, const int32_t *offsets,
                                      const int32_t *entries, const float *g, int B, int n, int K, float w, float *grad, void *stream) {
  RIGIDITY_SIZES("rigidity_backward", B, n, K);
  NSDP_REQUIRE(nsdp::finite_weight(w), "rigidity_backward: the weight must be finite");
  NSDP_REQUIRE(pred && idx && resid && offsets && entries && g && grad, "rigidity_backward: null pointer");
  const float c = static_cast<float>(static_cast<double>(w) / (static_cast<double>(B) * n * K));
  NSDP_TRACE("rigidity_backward<K=%d>", K);
  hipLaunchKernelGGL(rigidity_backward_kernel, dim3(nsdp::ceil_div(n, kThreads), B), dim3(kThreads), 0, nsdp::as_stream(stream), pred,
                     idx, resid, offsets, entries, g, n, K, c, grad);
  return nsdp::launch_status("rigidity_backward_kernel");
}
