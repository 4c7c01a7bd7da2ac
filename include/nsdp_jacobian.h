/*
 * nsdp_jacobian.h -- the deformation gradient of libnsdp_hip.so (ABI version 19): the fused fp32 decoder forward of
 * nsdp_hip.h (nsdp_decoder_fused_fwd) together with its per-point 3x3 Jacobian J = d out / d xyz_q, in one launch
 * (csrc/decoder_jacobian.hip: the register-resident chain differentiated in forward mode, value and three tangents as four
 * MFMA columns per query; nsdp_amd/hip_decoder.py wraps both entries).
 *
 * The decoder's output is the deformed position itself, so J is the deformation gradient (no "I +" correction).  The neighbour
 * indices `idx` are held fixed: J is the derivative of the function the forward entry evaluates for these indices.  ReLU has
 * derivative 0 at exactly 0 (torch's convention).
 *
 * Arguments: those of nsdp_decoder_fused_fwd / nsdp_decoder_fused_fwd_ragged (nsdp_hip.h: the per-shape tables, the 17 packed
 * fp32 weight pointers in fragment-major order, sizes) plus
 *   jac (B,NQ,3,3) or (cap,3,3), row-major:  jac[.., i, j] = d out[.., i] / d xyz_q[.., j].
 * `out` has the BITS nsdp_decoder_fused_fwd (or its ragged form) writes for the same operands: asking for the Jacobian does not
 * move a point.  A row's results do not depend on the rows around it, and a row gets the same bits in either form.
 *
 * Conventions of nsdp_hip.h: device pointers + sizes, dense row-major tensors, outputs allocated by the caller and possibly
 * UNINITIALISED on entry, `stream` a hipStream_t passed as void*, 0 / negative NSDP_E* / positive hipError_t as the return
 * value, the message in nsdp_last_error().  The argument checks are those of the forward entries and come before any launch;
 * B * NQ <= 0 (B * cap <= 0) returns 0 without a launch.  Nothing is read on the host: both calls are capturable.
 *
 * Packed form: xyz_q (cap,3), idx (cap,KN), out (cap,3), jac (cap,3,3), offsets (B+1) on the device.  A 4-query wave tile
 * belongs to one shape; a shape's last tile is partial (lanes clamped to the shape's last row, not stored).  Rows at or beyond
 * offsets[B] are not written.  Anchor indices are clamped to [0, A).
 *
 * tests/test_decoder_jacobian_gpu.py holds both entries to this inside the poisoned arena.
 */
#ifndef NSDP_JACOBIAN_H_
#define NSDP_JACOBIAN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int nsdp_decoder_jacobian_fwd(const float *xyz_q, const float *anchors, const int32_t *idx, const float *qk,
                              const float *vtab, const float *a_g, const float *v_g, const float *const *weights,
                              int n_weights, int B, int NQ, int A, int KN, int D, int H, float *out, float *jac,
                              void *stream);

int nsdp_decoder_jacobian_fwd_ragged(const float *xyz_q, const int32_t *offsets, const float *anchors, const int32_t *idx,
                                     const float *qk, const float *vtab, const float *a_g, const float *v_g,
                                     const float *const *weights, int n_weights, int B, int cap, int A, int KN, int D,
                                     int H, float *out, float *jac, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NSDP_JACOBIAN_H_ */
