/*
 * nsdp_rigidity.h -- the local-rigidity training regulariser of libnsdp_hip.so (ABI version 20): an as-isometric-as-possible
 * energy over the neighbour edges of the query set, forward and backward (nsdp_amd/rigidity.py wraps both in a
 * torch.autograd.Function).
 *
 * For predictions P(B,n,3) and sources S(B,n,3), fp32, row i of P the image of row i of S, and neighbour sets idx(B,n,K) int32
 * with entries in [0, n) of their own shape, l = idx[b,i,j]:
 *
 *   rest_ij = |s_i - s_l|^2,  cur_ij = |p_i - p_l|^2,  r_ij = cur_ij - rest_ij
 *   term[b] = (1 / (n K)) sum_i sum_j r_ij^2 / 4,      L = w * (1/B) sum_b term[b]
 *
 * (squared lengths: |p_i - p_l| has no gradient where the predictions collapse, the case this term is for; the "/ 4" leaves the
 * gradient free of factors: edge (i -> l) gives r_ij (p_i - p_l) to p_i and r_ij (p_l - p_i) to p_l).  No gradient flows to S or
 * idx.
 *
 * The conventions are those of nsdp_chamfer.h: device pointers + sizes, dense row-major tensors, outputs and the workspace
 * allocated by the caller and possibly UNINITIALISED on entry, `stream` a hipStream_t passed as void*, 0 / negative NSDP_E* /
 * positive hipError_t as the return value, the message in nsdp_last_error().  Sizes are judged before pointers and pointers
 * before anything is launched.  No entry reads device memory on the host (the upstream gradient is read by the kernel), so
 * every call is capturable and a captured call is kernel nodes alone.  Only the bytes declared here are touched; every byte
 * of the workspace is written before it is read.  No floating-point atomics anywhere: two runs give the same bits.
 *
 * Limits: 1 <= B <= 65535, 1 <= n <= 1 048 576, 1 <= K <= 32, n * K <= 33 554 432 (the bound of the list build),
 * B * n * K < 2^31; index products are formed in 64 bits.  The weight is taken as an fp32 value and must be finite.  inf / NaN
 * coordinates are out of contract, as for nsdp_knn.
 *
 * tests/test_rigidity_arena_gpu.py holds the launching entries to this inside the poisoned arena;
 * tools/rigidity_host_check.cpp runs the bad-argument table on the host.
 */
#ifndef NSDP_RIGIDITY_H_
#define NSDP_RIGIDITY_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace of nsdp_rigidity_forward for B shapes: 65 doubles per shape -- first the B unrounded per-shape terms, then
 * 64 slice sums for every shape.  0 for a B the entry refuses. */
size_t nsdp_rigidity_forward_workspace_bytes(int B);

/* Forward: pred(B,n,3), source(B,n,3), idx(B,n,K) ->  resid(B,n,K) f32, terms(B) f32, loss(1) f32.
 *
 * resid: one lane per point; every squared length is formed as nsdp_knn forms a distance, ((dx*dx + dy*dy) + dz*dz) of the
 * rounded differences dx = a_x - b_x ..., one rounding per operation and no contraction, and r = cur - rest rounds once:
 * |r - exact| <= 6 * 2^-24 * (cur + rest) to first order (five roundings in either squared length, one in the subtraction).  An
 * entry naming its own row gives 0 - 0; pred == source gives r = 0 everywhere (the same bits on either side).
 * term[b]: the scheme of nsdp_chamfer_forward, with the rows of a shape cut into slices(n) = min(64, ceil(n / 256)) runs of
 * R = ceil(n / slices) consecutive rows, a workgroup each (one workgroup per shape would walk n K values as one dependent chain
 * of double additions).  In a slice thread t takes its rows t, t + 256, ... and adds double(r) * double(r) (exact in double) in
 * column order, then a fixed tree over the 256 partial sums (strides 128 ... 1); one workgroup per shape then holds slice s in
 * thread s, sums them by the same tree and forms S / (4 n K) in double -- a function of that shape's rows alone; the double
 * goes into the workspace and, rounded once, into terms.  loss: one workgroup sums the
 * B doubles the same way (thread t: shapes t, t + 256, ...; the same tree), then w * (sum / B) in double, rounded once.
 * Indices are clamped into [0, n) before they form an address.
 * workspace: 8-byte aligned, nsdp_rigidity_forward_workspace_bytes(B) bytes. */
int nsdp_rigidity_forward(const float *pred, const float *source, const int32_t *idx, int B, int n, int K, float w, void *workspace,
                          float *resid, float *terms, float *loss, void *stream);

/* Backward, one kernel launch: the gradient of L with respect to pred,
 *
 *   grad[b,i] = (g * c) * ( sum_j r_ij (p_i - p_{idx[i,j]})  +  sum_{e in list(i)} r_e (p_i - p_{e div K}) ),
 *   c = fp32(w / (B * n * K))                                                    (formed in double on the host, rounded once)
 *
 * resid(B,n,K) as the forward wrote it; list(i) = entries[b][offsets[b][i] .. offsets[b][i+1]), the positions e of idx viewed as
 * (B, n*K) that name row i -- offsets(B,n+1), entries(B,n*K): the ASCENDING inverse lists of idx (nsdp_knn_invert where no list
 * exceeds 1024 entries, nsdp_knn_invert_wide anywhere); r_e = resid[b][e], e div K the row that names i; g(1) is the upstream
 * gradient, read from device memory by the kernel.
 *
 * Operation order (every operation rounds once, no contraction).  A term is r * (p_i - p_l): the difference, then the product.
 *   own columns         the lane adds its K terms in column order, starting from 0                      (depth K - 1)
 *   list, T its length:
 *   T <= 32             one lane adds the T terms in ascending list order                               (depth T - 1)
 *   32 < T <= 1024      a wave: lane t adds entries t, t + 64, ... in ascending order, then a butterfly over the 64 lanes
 *                       (strides 32, 16, 8, 4, 2, 1)                                                    (depth ceil(T/64) + 5)
 *   T > 1024            the workgroup: thread t adds entries t, t + 256, ..., then a tree in LDS over the 256 threads
 *                       (strides 128 ... 1)                                                             (depth ceil(T/256) + 7)
 * then grad = (g * c) * (own + list).  The order is a function of idx alone; an empty list adds exactly 0, a term with r = 0
 * adds exactly 0.  A term passes c (1), g * c (1), the difference (1), the product with r (1), its sum's additions (depth), own +
 * list (1) and the final product (1): per element |grad - exact| <= (6 + max(K - 1, depth(T))) * 2^-24 * sum |terms|, to first
 * order, with the residuals as given.  Indices, offsets and entries are clamped into their ranges before they form an address:
 * a stale tensor gives wrong numbers, never an access outside the operands. */
int nsdp_rigidity_backward(const float *pred, const int32_t *idx, const float *resid, const int32_t *offsets, const int32_t *entries,
                           const float *g, int B, int n, int K, float w, float *grad, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NSDP_RIGIDITY_H_ */
