// nsdp_adam_multi_f32: the Adam update of EVERY parameter tensor of a model in one launch.
//
// The reference steps `torch.optim.Adam` once per train step (/root/reference/model/__init__.py:10-41 builds it,
// model/deformation_networks.py:63-77 calls optimizer.step() after loss.backward()).  For the ~300 parameter tensors of a
// TDNet PyTorch's own multi-tensor kernels need 8 launches of 40 us each (36 tensors per launch travel in the kernel
// arguments; 126 MB of traffic at 0.4 TB/s) at the very tail of the step, where nothing else is left to run beside them.
// Here the tensor table lives in device memory (it is static across the replays of a captured step): one workgroup per
// 4096-element chunk of one tensor, all chunks of all tensors in one grid; 4 reads + 3 writes of 4 bytes per element,
// HBM-bound.
//
// Arithmetic = torch's single-tensor Adam on fp32 tensors, operation by operation with one rounding each (this file is
// compiled with contraction off; fp32 division and sqrt are correctly rounded):
//   g' = g + wd * p                      (weight_decay != 0;  -g first when maximize)
//   m  = m + (1 - beta1) * (g' - m)      (Tensor.lerp_, weight < 0.5)
//   v  = v * beta2 + ((1 - beta2) * g') * g'
//   p  = p + ((-lr / (1 - beta1^t)) * m) / (sqrt(v) / sqrt(1 - beta2^t) + eps)
// with the scalars formed in double and rounded to fp32 where torch hands them to an fp32 tensor op.
// WHICH torch: the CPU, non-capturable, single-tensor path -- torch.optim.Adam(foreach=False) on CPU tensors -- is the sequence
// restated here and what tests/test_adam_gpu.py compares with (moments to a few ulp of the largest term, parameters to one).
// torch's CUDA / ROCm kernels (foreach, fused, capturable: bias corrections in fp32, addcdiv as a + alpha * (m / denom)) may
// differ from it -- and hence from this kernel -- in the last place: nobody should rely on bit-equality with a GPU torch run.
// The step counter t is one fp32 scalar per tensor in device memory (torch's `capturable` layout: state["step"]); every
// chunk reads it, the LAST chunk of a tensor to finish stores t + 1 (a per-tensor arrival counter that the same workgroup
// resets) -- no second launch, and the value never depends on the order in which the chunks ran.
//
// The entries of include/nsdp_optim.h live here too, over the same tables: the global gradient norm as a fixed-order double sum
// (grad_sumsq_kernel per chunk, grad_clip_finalize_kernel over the partials: clip_grad_norm_'s factor and the decision to skip a
// non-finite step, written to device memory), and nsdp_adam_multi_clipped_f32 -- this file's kernel body instantiated with a
// compile-time flag for the one extra multiplication g * coef.  nsdp_adam_multi_f32 is the instantiation without it.
#include <math.h>

#include "common.h"
#include "../../include/nsdp_optim.h"

namespace {

constexpr int kChunk = 4096;      // elements per workgroup: 256 lanes x 4 float4

struct Scalars {
  float neg_step_size, bc2_sqrt, w1, beta2, w2, eps, wd;
  int maximize;
};

// kClip (nsdp_adam_multi_clipped_f32, include/nsdp_optim.h): g * coef where torch's clip_grad_norm_ scales the gradient before
// Adam sees it -- after the negation, before the weight decay.  coef == 1.0f returns g's own bits.
template <bool kClip>
__device__ __forceinline__ void adam_one(float &p, float g, float &m, float &v, const Scalars &s, float coef) {
  if (s.maximize) g = -g;
  if (kClip) g = g * coef;
  if (s.wd != 0.f) g = g + s.wd * p;
  m = m + s.w1 * (g - m);
  v = v * s.beta2 + (s.w2 * g) * g;
  const float denom = sqrtf(v) / s.bc2_sqrt + s.eps;
  p = p + (s.neg_step_size * m) / denom;
}

template <bool kClip>
__device__ __forceinline__ void adam_multi_body(const NsdpAdamDesc *__restrict__ descs, const int2 *__restrict__ chunks,
                                                int *__restrict__ done, const float *__restrict__ lr_dev, double lr_host,
                                                double beta1, double beta2, double eps, double weight_decay, int maximize,
                                                const NsdpClipState *__restrict__ state) {
  float coef = 1.0f;
  if (kClip) {
    // a skipped step: no parameter, moment or step counter is touched, and `done` (zero on entry) stays at zero
    if (state->apply == 0) return;
    coef = state->coef;
  }
  const int2 c = chunks[blockIdx.x];      // (tensor, chunk of that tensor)
  const NsdpAdamDesc d = descs[c.x];
  const float step_old = *d.step;
  const double t = static_cast<double>(step_old) + 1.0;
  const double lr = lr_dev ? static_cast<double>(*lr_dev) : lr_host;
  const double bc1 = 1.0 - pow(beta1, t), bc2 = 1.0 - pow(beta2, t);
  Scalars s;
  s.neg_step_size = static_cast<float>(-(lr / bc1));
  s.bc2_sqrt = static_cast<float>(sqrt(bc2));
  s.w1 = static_cast<float>(1.0 - beta1);
  s.beta2 = static_cast<float>(beta2);
  s.w2 = static_cast<float>(1.0 - beta2);
  s.eps = static_cast<float>(eps);
  s.wd = static_cast<float>(weight_decay);
  s.maximize = maximize;

  const long long base = static_cast<long long>(c.y) * kChunk;
  const long long left = d.numel - base;
  const int cnt = left < kChunk ? static_cast<int>(left) : kChunk;
  float *__restrict__ p = d.param + base;
  const float *__restrict__ g = d.grad + base;
  float *__restrict__ m = d.exp_avg + base;
  float *__restrict__ v = d.exp_avg_sq + base;
  const bool vec = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) |
                     reinterpret_cast<uintptr_t>(v)) & 15) == 0;
  if (vec) {
    const int n4 = cnt >> 2;
    for (int i = threadIdx.x; i < n4; i += 256) {
      float4 pp = reinterpret_cast<const float4 *>(p)[i];
      const float4 gg = reinterpret_cast<const float4 *>(g)[i];
      float4 mm = reinterpret_cast<const float4 *>(m)[i];
      float4 vv = reinterpret_cast<const float4 *>(v)[i];
      adam_one<kClip>(pp.x, gg.x, mm.x, vv.x, s, coef);
      adam_one<kClip>(pp.y, gg.y, mm.y, vv.y, s, coef);
      adam_one<kClip>(pp.z, gg.z, mm.z, vv.z, s, coef);
      adam_one<kClip>(pp.w, gg.w, mm.w, vv.w, s, coef);
      reinterpret_cast<float4 *>(p)[i] = pp;
      reinterpret_cast<float4 *>(m)[i] = mm;
      reinterpret_cast<float4 *>(v)[i] = vv;
    }
    for (int i = 4 * n4 + threadIdx.x; i < cnt; i += 256) {
      float pp = p[i], mm = m[i], vv = v[i];
      adam_one<kClip>(pp, g[i], mm, vv, s, coef);
      p[i] = pp; m[i] = mm; v[i] = vv;
    }
  } else {
    for (int i = threadIdx.x; i < cnt; i += 256) {
      float pp = p[i], mm = m[i], vv = v[i];
      adam_one<kClip>(pp, g[i], mm, vv, s, coef);
      p[i] = pp; m[i] = mm; v[i] = vv;
    }
  }
  // Every chunk has READ the counter (its value went into the scalars above) by the time it arrives here; the last one
  // to arrive advances it.  No fence: nothing another workgroup WROTE has to be visible to the one that stores t + 1
  // (an agent-scope release per workgroup is what made the last-workgroup finalize of the BatchNorm reductions 2.5x
  // slower).
  __syncthreads();
  if (threadIdx.x == 0) {
    const int nchunks = static_cast<int>((d.numel + kChunk - 1) / kChunk);
    if (atomicAdd(&done[c.x], 1) == nchunks - 1) {
      done[c.x] = 0;
      *d.step = step_old + 1.0f;
    }
  }
}

__global__ __launch_bounds__(256) void adam_multi_kernel(const NsdpAdamDesc *__restrict__ descs,
                                                         const int2 *__restrict__ chunks, int *__restrict__ done,
                                                         const float *__restrict__ lr_dev, double lr_host, double beta1,
                                                         double beta2, double eps, double weight_decay, int maximize) {
  adam_multi_body<false>(descs, chunks, done, lr_dev, lr_host, beta1, beta2, eps, weight_decay, maximize, nullptr);
}

__global__ __launch_bounds__(256) void adam_multi_clipped_kernel(const NsdpAdamDesc *__restrict__ descs,
                                                                 const int2 *__restrict__ chunks, int *__restrict__ done,
                                                                 const float *__restrict__ lr_dev, double lr_host, double beta1,
                                                                 double beta2, double eps, double weight_decay, int maximize,
                                                                 const NsdpClipState *__restrict__ state) {
  adam_multi_body<true>(descs, chunks, done, lr_dev, lr_host, beta1, beta2, eps, weight_decay, maximize, state);
}

// ---- include/nsdp_optim.h: the global gradient norm in a fixed order --------------------------------------------------------
// a[l] += a[l + s] for s = 128 ... 1 over the 256 lanes' values; the sum is returned in thread 0 (others: unspecified).  The
// strides 128 and 64 go through LDS; from 32 down the pairs lie inside wave 0, where lane l reads lane l + s's register -- the
// same pairing (lane l + s < 2 s holds a[l + s] as the previous stride left it).
__device__ __forceinline__ double halving_sum_256(double acc, double *sh) {
  const int l = threadIdx.x;
  sh[l] = acc;
  __syncthreads();
  if (l < 128) sh[l] = sh[l] + sh[l + 128];
  __syncthreads();
  if (l < 64) acc = sh[l] + sh[l + 64];
  if (l < 64) {
    for (int s = 32; s >= 1; s >>= 1) acc = acc + __shfl_down(acc, s, 64);
  }
  return acc;
}

__device__ __forceinline__ double sq(float x) { return static_cast<double>(x) * static_cast<double>(x); }

__global__ __launch_bounds__(256) void grad_sumsq_kernel(const NsdpAdamDesc *__restrict__ descs, const int2 *__restrict__ chunks,
                                                         double *__restrict__ partials) {
  __shared__ double sh[256];
  const int2 c = chunks[blockIdx.x];
  const float *__restrict__ grad = descs[c.x].grad;
  const long long numel = descs[c.x].numel;
  const long long base = static_cast<long long>(c.y) * kChunk;
  const long long left = numel - base;
  const int cnt = left < kChunk ? static_cast<int>(left) : kChunk;
  const float *__restrict__ g = grad + base;
  const bool vec = (reinterpret_cast<uintptr_t>(g) & 15) == 0;
  // lane l: elements 4 (l + 256 j) .. + 3, ascending -- whole groups of four first, the chunk's last (partial) group last
  double acc = 0.0;
  for (int i = threadIdx.x; 4 * i < cnt; i += 256) {
    const int e = 4 * i;
    if (e + 4 <= cnt) {
      float4 gg;
      if (vec) {
        gg = reinterpret_cast<const float4 *>(g)[i];
      } else {
        gg.x = g[e]; gg.y = g[e + 1]; gg.z = g[e + 2]; gg.w = g[e + 3];
      }
      acc = acc + sq(gg.x);
      acc = acc + sq(gg.y);
      acc = acc + sq(gg.z);
      acc = acc + sq(gg.w);
    } else {
      for (int k = e; k < cnt; ++k) acc = acc + sq(g[k]);
    }
  }
  acc = halving_sum_256(acc, sh);
  if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}

__global__ __launch_bounds__(256) void grad_clip_finalize_kernel(const double *__restrict__ partials, int n_chunks, double max_norm,
                                                                 int skip_nonfinite, NsdpClipState *__restrict__ state) {
  __shared__ double sh[256];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n_chunks; i += 256) acc = acc + partials[i];
  const double S = halving_sum_256(acc, sh);
  if (threadIdx.x != 0) return;
  const double norm = sqrt(S);
  const double c = max_norm / (norm + 1e-6);
  // min(c, 1) that keeps a NaN, as torch.clamp(max=1) does
  const float coef = (c < 1.0 || c != c) ? static_cast<float>(c) : 1.0f;
  const bool finite = S == S && fabs(S) <= DBL_MAX;
  const int apply = (skip_nonfinite && !finite) ? 0 : 1;
  state->sumsq = S;
  state->norm = static_cast<float>(norm);
  state->coef = coef;
  state->apply = apply;
  state->steps = state->steps + 1;
  if (apply && coef < 1.0f) state->clipped = state->clipped + 1;
  if (!apply) state->skipped = state->skipped + 1;
}

}  // namespace

extern "C" int nsdp_adam_chunk_elems(void) { return kChunk; }

static int adam_args_ok(const char *who, const void *descs_dev, const void *chunks_dev, const void *done_dev, const float *lr_dev,
                        double lr, double beta1, double beta2, double eps) {
  NSDP_REQUIRE(descs_dev && chunks_dev && done_dev, "%s: null table pointer", who);
  NSDP_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0,
               "%s: betas must be in [0, 1), eps >= 0 (beta1=%g beta2=%g eps=%g)", who, beta1, beta2, eps);
  NSDP_REQUIRE(lr_dev || lr >= 0.0, "%s: negative learning rate %g", who, lr);
  return 0;
}

extern "C" int nsdp_adam_multi_f32(const NsdpAdamDesc *descs_dev, const int32_t *chunks_dev, int n_chunks,
                                   int32_t *done_dev, const float *lr_dev, double lr, double beta1, double beta2,
                                   double eps, double weight_decay, int maximize, void *stream) {
  if (n_chunks <= 0) return 0;
  if (int rc = adam_args_ok("adam_multi_f32", descs_dev, chunks_dev, done_dev, lr_dev, lr, beta1, beta2, eps)) return rc;
  hipStream_t st = nsdp::as_stream(stream);
  hipLaunchKernelGGL(adam_multi_kernel, dim3(static_cast<unsigned>(n_chunks)), dim3(256), 0, st, descs_dev,
                     reinterpret_cast<const int2 *>(chunks_dev), done_dev, lr_dev, lr, beta1, beta2, eps, weight_decay,
                     maximize);
  return nsdp::launch_status("adam_multi_kernel");
}

extern "C" int nsdp_adam_multi_clipped_f32(const NsdpAdamDesc *descs_dev, const int32_t *chunks_dev, int n_chunks,
                                           int32_t *done_dev, const float *lr_dev, double lr, double beta1, double beta2,
                                           double eps, double weight_decay, int maximize, const NsdpClipState *state_dev,
                                           void *stream) {
  if (n_chunks <= 0) return 0;
  if (int rc = adam_args_ok("adam_multi_clipped_f32", descs_dev, chunks_dev, done_dev, lr_dev, lr, beta1, beta2, eps)) return rc;
  NSDP_REQUIRE(state_dev, "adam_multi_clipped_f32: null clip state");
  hipStream_t st = nsdp::as_stream(stream);
  hipLaunchKernelGGL(adam_multi_clipped_kernel, dim3(static_cast<unsigned>(n_chunks)), dim3(256), 0, st, descs_dev,
                     reinterpret_cast<const int2 *>(chunks_dev), done_dev, lr_dev, lr, beta1, beta2, eps, weight_decay,
                     maximize, state_dev);
  return nsdp::launch_status("adam_multi_clipped_kernel");
}

extern "C" size_t nsdp_grad_sumsq_workspace_bytes(int n_chunks) {
  return n_chunks > 0 ? sizeof(double) * static_cast<size_t>(n_chunks) : 0;
}

extern "C" int nsdp_grad_sumsq_f32(const NsdpAdamDesc *descs_dev, const int32_t *chunks_dev, int n_chunks, double *partials_dev,
                                   void *stream) {
  if (n_chunks <= 0) return 0;
  NSDP_REQUIRE(descs_dev && chunks_dev, "grad_sumsq_f32: null table pointer");
  NSDP_REQUIRE(partials_dev && (reinterpret_cast<uintptr_t>(partials_dev) & 7) == 0,
               "grad_sumsq_f32: the partials buffer must be a non-null, 8-byte-aligned pointer");
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3(static_cast<unsigned>(n_chunks)), dim3(256), 0, nsdp::as_stream(stream), descs_dev,
                     reinterpret_cast<const int2 *>(chunks_dev), partials_dev);
  return nsdp::launch_status("grad_sumsq_kernel");
}

extern "C" int nsdp_grad_clip_finalize(const double *partials_dev, int n_chunks, double max_norm, int skip_nonfinite,
                                       NsdpClipState *state_dev, void *stream) {
  NSDP_REQUIRE(n_chunks >= 0, "grad_clip_finalize: n_chunks = %d is negative", n_chunks);
  NSDP_REQUIRE(max_norm > 0.0, "grad_clip_finalize: max_norm must be positive (+inf allowed), got %g", max_norm);
  NSDP_REQUIRE(n_chunks == 0 || (partials_dev && (reinterpret_cast<uintptr_t>(partials_dev) & 7) == 0),
               "grad_clip_finalize: the partials buffer must be a non-null, 8-byte-aligned pointer");
  NSDP_REQUIRE(state_dev && (reinterpret_cast<uintptr_t>(state_dev) & 7) == 0,
               "grad_clip_finalize: the clip state must be a non-null, 8-byte-aligned pointer");
  hipLaunchKernelGGL(grad_clip_finalize_kernel, dim3(1), dim3(256), 0, nsdp::as_stream(stream), partials_dev, n_chunks, max_norm,
                     skip_nonfinite, state_dev);
  return nsdp::launch_status("grad_clip_finalize_kernel");
}
