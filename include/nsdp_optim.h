/*
 * nsdp_optim.h -- the optimizer step's guard rails of libnsdp_hip.so (ABI version 25): a bound on the GLOBAL gradient norm and
 * the skipping of a step whose gradient is not finite, both decided on the device (nsdp_amd/hip_adam.py:
 * HipAdam(max_grad_norm=, skip_nonfinite=)).
 *
 * The rule is torch.nn.utils.clip_grad_norm_(parameters, max_norm, norm_type=2) followed by Adam.  With G every element of
 * every gradient of the tables (all parameter groups):
 *
 *   S    = sum over G of g^2          accumulated in DOUBLE in the fixed order below
 *   norm = sqrt(S)                    in double
 *   c    = max_norm / (norm + 1e-6)   in double
 *   coef = fp32(c) if c < 1, c if c is NaN, else 1.0f          (NaN-propagating, as torch.clamp(max=1))
 *
 * and the Adam update of nsdp_adam_multi_f32 (nsdp_hip.h) runs on g * coef in place of g: one fp32 multiplication, after the
 * `maximize` negation and before `+ wd * p`.  coef == 1.0f is the identity: a step within the bound gives the bits of
 * nsdp_adam_multi_f32.  The gradients are NOT rewritten (torch scales them in place; here they keep their values and the
 * scale is in NsdpClipState).  S cannot overflow from finite fp32 values (at most 2^63 elements of at most 2^256), so a
 * non-finite S means that some g is inf or NaN; with skip_nonfinite such a step changes no parameter, no moment and no step
 * counter.  Without it the result is torch's: an inf gives coef = 0 and 0 * inf = NaN in that element, a NaN gives NaN everywhere.
 *
 * The order of S -- a function of the gradient VALUES alone: not of the schedule, the streams, eager or replayed execution, or
 * the alignment of a tensor.  Chunks are those of the Adam chunk table (nsdp_adam_chunk_elems() = 4096 elements of one tensor,
 * one 256-lane workgroup each).
 *   in a chunk     lane l owns the elements 4 (l + 256 j) .. + 3 of the chunk, j = 0, 1, ..., and adds their squares (exact in
 *                  double) to its accumulator, starting from 0, in ascending element order.  A 16-byte-aligned chunk is
 *                  loaded as float4, any other with scalar loads of the same elements in the same order.
 *   across lanes   a[l] += a[l + s] for s = 128, 64, ..., 1; a[0] is the chunk's partial
 *   across chunks  one workgroup: lane l adds the partials l, l + 256, ... of the whole buffer (groups one after the other, table
 *                  order) in ascending order, starting from 0, then the same halving.
 * No floating-point atomics and no last-workgroup finalize: the counters have a single writer.
 *
 * Conventions: those of nsdp_rigidity.h -- device pointers + sizes, `stream` a hipStream_t passed as void*, 0 / negative NSDP_E* /
 * positive hipError_t as the return value, the message in nsdp_last_error(); arguments are judged before anything is launched;
 * no entry reads device memory on the host, so every call is capturable and a captured call is one kernel node.  Only the bytes
 * declared here are touched.
 */
#ifndef NSDP_OPTIM_H_
#define NSDP_OPTIM_H_

#include <stddef.h>
#include <stdint.h>

#include "nsdp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 32 bytes of device memory, 8-byte aligned.  The first four fields are written whole by every nsdp_grad_clip_finalize; the three
 * counters are running sums that the caller zeroes once (one thread reads and rewrites them). */
typedef struct {
  double sumsq;     /* S */
  float norm;       /* fp32(sqrt(S)) */
  float coef;       /* the factor the update multiplies every gradient element by */
  int32_t apply;    /* 0: this step is skipped (skip_nonfinite and S not finite), else 1 */
  int32_t steps;    /* + 1 per finalize */
  int32_t clipped;  /* + 1 per finalize with apply != 0 and coef < 1 */
  int32_t skipped;  /* + 1 per finalize with apply == 0 */
} NsdpClipState;

/* Bytes of the partials buffer for n_chunks chunks: one double each.  0 for n_chunks <= 0.  Host only. */
size_t nsdp_grad_sumsq_workspace_bytes(int n_chunks);

/* partials[c] = the sum of squares of chunk c of the Adam tables (descs / chunks as nsdp_adam_multi_f32 takes them), c in
 * [0, n_chunks): a grid of n_chunks workgroups.  Reads `grad` and `numel` of the descriptors only; writes every partial
 * (partials may be uninitialised on entry, 8-byte aligned).  n_chunks <= 0 launches nothing. */
int nsdp_grad_sumsq_f32(const NsdpAdamDesc *descs_dev, const int32_t *chunks_dev, int n_chunks, double *partials_dev, void *stream);

/* One workgroup: S from partials[0 .. n_chunks) (n_chunks == 0: S = 0, partials may be NULL), then the rule above into *state.
 * max_norm > 0, +inf allowed (coef is then 1 whenever it is not NaN: the guard alone); max_norm <= 0 or NaN is refused. */
int nsdp_grad_clip_finalize(const double *partials_dev, int n_chunks, double max_norm, int skip_nonfinite, NsdpClipState *state_dev,
                            void *stream);

/* nsdp_adam_multi_f32 on g * state->coef: the same kernel body, arguments and launch.  state->apply == 0: nothing but the
 * state is read and nothing is written -- parameters, moments and step counters keep their bits, `done` stays at zero. */
int nsdp_adam_multi_clipped_f32(const NsdpAdamDesc *descs_dev, const int32_t *chunks_dev, int n_chunks, int32_t *done_dev,
                                const float *lr_dev, double lr, double beta1, double beta2, double eps, double weight_decay,
                                int maximize, const NsdpClipState *state_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NSDP_OPTIM_H_ */
