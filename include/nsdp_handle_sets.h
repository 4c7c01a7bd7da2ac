/*
 * nsdp_handle_sets.h -- labelled handle sets: several handles per shape, each with a motion of its own, per-point targets, and
 * T poses of one source in one launch (libnsdp_hip.so, ABI version 17).
 *
 * nsdp_handles.h and nsdp_handles_ragged.h write the deformation network's input rows for the reference's drag: ONE region,
 * picked by the bounding-box rule or one mask, moved by ONE translation.  The network itself takes any set of handle points, each
 * with a target of its own (columns 3..6 of its input rows).  The two entries here write those columns from
 *
 *   labels    one byte per point: 0 = a free point, h in 1..H = a point of handle h.  A label ABOVE H IS A FREE POINT: the byte
 *             indexes the motion table, and whatever it holds nothing is read outside the table;
 *   motions   per (pose, shape, handle) a row-major 3 x 4 matrix [A | t], twelve floats: rigid or affine, a rotation about a
 *             pivot c being [R | c - R c] (the pivot is folded into t by whoever composes the motion);
 *   targets   instead of motions: a target per point, copied.  Every non-zero label is then a handle; H is not read.
 *
 * For a handle point (x, y, z) of label h, M = its (pose, shape)'s motions[h - 1]:
 *     tgt_c = ((M[c][0] * x + M[c][1] * y) + M[c][2] * z) + M[c][3]          c = 0, 1, 2
 * every product and every sum rounded once, in this order, no fused multiply-add.  The target of a free point is its src row,
 * copied, not computed.  With h = handle as 0.0f / 1.0f the outputs are
 *     tgt             the targets
 *     rows            columns 3..5 = tgt * h, a literal product (-0 and NaN come out as the array expression gives them),
 *                     column 6 = h; COLUMNS 0..2 ARE NEVER WRITTEN
 *     handle_out      0 / 1 per point of the source; it does not depend on the pose, the lanes of pose 0 write it.
 *
 * Conventions (those of the two headers above): device pointers plus sizes; outputs may be uninitialised on entry; sizes are
 * checked before any pointer is looked at, pointers (null, 4-byte alignment of the 32-bit operands) before anything is launched;
 * 0 / negative NSDP_E* / positive hipError_t comes back, the message in nsdp_last_error().  `stream` is a hipStream_t passed as
 * void*; under a capture there is one kernel node.  No atomics of any kind; no workgroup waits for another; plain vector stores.
 * Index products are formed in 64 bits.
 *
 * tests/test_handle_sets_arena_gpu.py holds both entries inside the poisoned arena.
 */
#ifndef NSDP_HANDLE_SETS_H_
#define NSDP_HANDLE_SETS_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Rectangular sets, one lane per (pose, shape, point).  Inputs: src(B,n,3) f32, labels(B,n) u8, and exactly one of
 * motions(T,B,H,12) f32 and targets(T,B,n,3) f32 (the other null; with targets H is not read and may be 0).
 * Outputs (rows is required, the others may be null): rows(T,B,n,7), tgt(T,B,n,3), handle_out(B,n) u8.
 * Limits: 1 <= B, 1 <= T, T * B <= 65535, 1 <= n <= 1 048 576, 1 <= H <= 255 with motions.
 */
int nsdp_handle_set_rows(const float *src, const uint8_t *labels, const float *motions, const float *targets, int B, int n, int H,
                         int T, float *rows, float *tgt, uint8_t *handle_out, void *stream);

/*
 * The same row body over a packed set, one pose: src(cap,3), labels(cap), offsets(B+1) i32 on the device, and exactly one of
 * motions(B,H,12) and targets(cap,3).  Outputs: rows(cap,7), tgt(cap,3), handle_out(cap).  The offsets are clamped as
 * nsdp_handle_rows_ragged clamps them (a shape's first row to [0, cap], its end to [first row, cap]); the host never reads them.
 * Rows at or beyond the clamped total (and before offsets[0]) are never read or written.  A row carries the bits the rectangular
 * entry gives it on its shape alone.
 * Limits: 1 <= B <= 65535, 1 <= cap, 1 <= H <= 255 with motions.
 */
int nsdp_handle_set_rows_ragged(const float *src, const int32_t *offsets, const uint8_t *labels, const float *motions,
                                const float *targets, int B, int cap, int H, float *rows, float *tgt, uint8_t *handle_out,
                                void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NSDP_HANDLE_SETS_H_ */
