/*
 * nsdp_chamfer.h -- the Chamfer training loss of libnsdp_hip.so (ABI version 18): a correspondence-free loss between a
 * predicted cloud and a target cloud, forward and backward (nsdp_amd/chamfer.py wraps both in a torch.autograd.Function).
 *
 * For predictions P(B,n,3) and targets Q(B,m,3), fp32, m not tied to n,
 *
 *   L = (1/B) sum_b term[b],   term[b] = w_pt * (1/n) sum_i min_j |p_i - q_j|^2 / 2  +  w_tp * (1/m) sum_j min_i |q_j - p_i|^2 / 2
 *
 * (squared distances; the "/ 2" is compute_l2_error's: where every point's nearest neighbour is its correspondent and
 * w_tp = 0, L is the l2 loss up to rounding).
 *
 * The conventions are those of nsdp_eval.h: device pointers + sizes, dense row-major tensors, outputs and the workspace
 * allocated by the caller and possibly UNINITIALISED on entry, `stream` a hipStream_t passed as void*, 0 / negative NSDP_E* /
 * positive hipError_t as the return value, the message in nsdp_last_error().  Sizes are judged before pointers and pointers
 * before anything is launched.  No entry reads device memory on the host (the upstream gradient is read by the kernel), so
 * every call is capturable and a captured call is kernel nodes alone.  Only the bytes declared here are touched; every byte
 * of the workspace is written before it is read.  No floating-point atomics anywhere: two runs give the same bits.
 *
 * Limits (those of the entries this rests on): 1 <= B <= 65535, 1 <= n, m <= 1 048 576, B * max(n, m) < 2^31; index products
 * are formed in 64 bits.  The weights are taken as fp32 values.  inf / NaN coordinates are out of contract, as for nsdp_knn.
 *
 * tests/test_chamfer_arena_gpu.py holds the launching entries to this inside the poisoned arena;
 * tools/chamfer_host_check.cpp runs the bad-argument table on the host.
 */
#ifndef NSDP_CHAMFER_H_
#define NSDP_CHAMFER_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace of nsdp_chamfer_forward for B shapes (one double per shape: the unrounded per-shape terms).  0 for a B
 * the entry refuses. */
size_t nsdp_chamfer_forward_workspace_bytes(int B);

/* Forward: pred(B,n,3), target(B,m,3) ->
 *   dist2_pt(B,n) f32 / idx_pt(B,n) i32: squared distance and index of the nearest target of every prediction,
 *   dist2_tp(B,m) f32 / idx_tp(B,m) i32: squared distance and index of the nearest prediction of every target,
 *   terms(B) f32, loss(1) f32.
 * The two searches ARE nsdp_nn_dist2(..., idx_out != NULL) (nsdp_eval.h; this entry calls it): the distance bits of nsdp_knn,
 * the smallest index among exact ties.  term[b]: one workgroup per shape, thread t sums rows t, t + 256, ... of each direction
 * in double, a fixed tree over the 256 partial sums, then (w_pt * S_pt / (2 n) + w_tp * S_tp / (2 m)) in double -- a function
 * of that shape's rows alone; the double goes into the workspace and, rounded once, into terms.  loss: one workgroup sums the
 * B doubles the same way (thread t: shapes t, t + 256, ...; the same tree), divides by B and rounds once.  Exactly 0 for
 * pred == target.  workspace: 8-byte aligned, nsdp_chamfer_forward_workspace_bytes(B) bytes. */
int nsdp_chamfer_forward(const float *pred, const float *target, int B, int n, int m, float w_pt, float w_tp, void *workspace,
                         float *dist2_pt, int32_t *idx_pt, float *dist2_tp, int32_t *idx_tp, float *terms, float *loss,
                         void *stream);

/* Backward for ONE operand, one kernel launch: the gradient of L with respect to `self`(B,n_self,3), `other`(B,n_other,3)
 * being the other cloud:
 *
 *   grad[b,i] = (g * s_d) * (x_i - y_{a(i)})  +  (g * s_l) * sum_{l in list(i)} (x_i - y_l),
 *   s_d = fp32(w_direct / (B * n_self)),  s_l = fp32(w_list / (B * n_other))       (formed in double on the host, rounded once)
 *
 * x = self, y = other; a = idx_self(B,n_self), the nearest `other` row of every `self` row; list(i) = entries[b][offsets[b][i]
 * .. offsets[b][i+1]), the `other` rows whose nearest `self` row is i -- offsets(B,n_self+1), entries(B,n_other): the inverse
 * lists of the opposite direction's index (nsdp_knn_invert where no list exceeds 1024 entries, nsdp_knn_invert_wide anywhere:
 * ASCENDING lists); g(1) is the upstream gradient, read from device memory by the kernel.  d(pred): self = pred, idx_self =
 * idx_pt, lists of idx_tp, w_direct = w_pt, w_list = w_tp; d(target): the roles and the weights swapped.
 *
 * Operation order (every operation rounds once, no contraction), T = the list's length:
 *   T <= 32             one lane adds the T differences in ascending list order                         (depth T - 1)
 *   32 < T <= 1024      a wave: lane t adds entries t, t + 64, ... in ascending order, then a butterfly over the 64 lanes
 *                       (strides 32, 16, 8, 4, 2, 1)                                                    (depth ceil(T/64) + 5)
 *   T > 1024            the workgroup: thread t adds entries t, t + 256, ..., then a tree in LDS over the 256 threads
 *                       (strides 128 ... 1)                                                             (depth ceil(T/256) + 7)
 * then grad = (g * s_d) * d + (g * s_l) * S.  The order is a function of the list alone; an empty list adds exactly 0, so a row
 * with x_i == y_{a(i)} and an empty list gets exactly 0.  Per element |grad - exact| <= (5 + depth) * 2^-24 * sum |terms|, to
 * first order.  With w_list == 0 offsets and entries are not read and may be NULL.  Indices and offsets are clamped into their
 * ranges before they form an address: a stale index tensor gives wrong numbers, never an access outside the operands. */
int nsdp_chamfer_backward(const float *self, const float *other, const int32_t *idx_self, const int32_t *offsets,
                          const int32_t *entries, const float *g, int B, int n_self, int n_other, float w_direct, float w_list,
                          float *grad, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NSDP_CHAMFER_H_ */
