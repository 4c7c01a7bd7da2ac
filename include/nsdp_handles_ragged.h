/*
 * nsdp_handles_ragged.h -- user-handle drags over a PACKED batch of meshes of different sizes (libnsdp_hip.so, ABI version 16).
 *
 * nsdp_handles.h holds the rule for rectangular (B, n, .) sets.  The reference's batch loop (run.py, "Run-batch-processing")
 * walks meshes whose cloud is their own vertex set, every mesh with a vertex count of its own; the entries here are the same two
 * kernels over the packed layout of nsdp_hip.h: packed(cap, C) rows with offsets(B+1) int32 ON THE DEVICE, shape b owning rows
 * offsets[b] .. offsets[b+1], offsets[B] = total <= cap.
 *
 *   nsdp_handle_bounds_ragged   per-shape bounding box of each shape's own rows (once per batch of source meshes);
 *   nsdp_handle_rows_ragged     per packed row: the predicates, the dragged target and columns 3..6 of the (cap, 7) rows the
 *                               deformation network's encoder reads, with the drag of the row's shape.
 *
 * The words of params(B,8), the part numbers and the rule are those of nsdp_handles.h (include it for NSDP_HANDLE_*).  A row gets
 * the bits nsdp_handle_rows gives it on its shape alone (B = 1, n = n_b), and bounds[b] the bits of nsdp_handle_bounds on shape b
 * alone: the arithmetic is the same literal products and sums, one rounding per operation, and the extremes are taken in the same
 * total order of the fp32 bit patterns, which does not depend on how the rows are split.
 *
 * Conventions (nsdp_hip.h's packed entries): the host passes B, cap and -- where a grid needs it -- n_max, an upper bound of the
 * largest shape; it never reads `offsets`.  Every offset is clamped as it is read: a shape's first row to [0, cap], its end to
 * [first row, cap], and where n_max is used its row count to n_max.  A corrupt `offsets` or a too-small n_max gives wrong
 * numbers, never an access outside the buffers.  Sizes are checked before any pointer is looked at, pointers (null, 4-byte
 * alignment of the 32-bit operands) before anything is launched.  0 / negative NSDP_E* / positive hipError_t comes back, the
 * message in nsdp_last_error().  `stream` is a hipStream_t passed as void*; under a capture there are kernel nodes only.  No
 * atomics of any kind; no workgroup waits for another.  Index products are formed in 64 bits.
 *
 * Limits: 1 <= B <= 65535, 1 <= cap, 1 <= n_max <= 1 048 576.
 *
 * tests/test_handles_ragged_arena_gpu.py holds both launching entries inside the poisoned arena.
 */
#ifndef NSDP_HANDLES_RAGGED_H_
#define NSDP_HANDLES_RAGGED_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* bounds(b, 0..2) and bounds(b, 3..5) of a shape WITHOUT rows: the identities of the two reductions, as fp32 bit patterns
 * (the last pattern of the total order for the minimum, a positive NaN; the first for the maximum, a negative NaN). */
#define NSDP_HANDLE_BOUNDS_EMPTY_MIN_BITS 0x7fffffffu
#define NSDP_HANDLE_BOUNDS_EMPTY_MAX_BITS 0xffffffffu

/* Bytes of workspace nsdp_handle_bounds_ragged uses: B * ceil(n_max / 4096) * 6 words.  0 for arguments the entry refuses. */
size_t nsdp_handle_bounds_ragged_workspace_bytes(int B, int cap, int n_max);

/*
 * cano(cap,3) f32, offsets(B+1) i32 -> bounds(B,6) f32: min x, min y, min z, max x, max y, max z of each shape's own rows.
 *
 * A (ceil(n_max / 4096), B) grid of workgroups writes partial extremes into the workspace, each reading its shape's range from
 * the offsets; a workgroup whose share of the shape is empty writes the identities, so every word of the declared size is
 * written by the call itself, stream-ordered, before it is read.  One workgroup per shape reduces the partials: two launches.
 * The order is nsdp_handle_bounds': -0.0 sorts below +0.0, a NaN sorts beyond the infinity of its sign.  A shape without rows
 * gets the identities above.  Rows of a shape beyond its first n_max are not looked at.  The workspace (4-byte aligned) must not
 * be shared by calls that may run at the same time.
 */
int nsdp_handle_bounds_ragged(const float *cano, const int32_t *offsets, int B, int cap, int n_max, void *workspace,
                              float *bounds, void *stream);

/*
 * One lane per packed row.  Inputs: cano(cap,3), src(cap,3) f32; offsets(B+1) i32; bounds(B,6) f32; params(B,8), one drag per
 * shape; handle_mask, move_mask (cap) u8, both null (the rule of nsdp_handle_rows decides) or both non-null (non-zero bytes are
 * the handle / the moved rows; cano and bounds are then not read and may be null).
 *
 * Outputs (rows is required, the others may be null), m = move and h = handle as 0.0f / 1.0f:
 *     tgt(cap,3)      = src + d * m
 *     rows(cap,7)     columns 3..5 = tgt * h, column 6 = h; COLUMNS 0..2 ARE NEVER WRITTEN
 *     handle_out, move_out (cap) u8 = 0 / 1
 * Rows at or beyond offsets[B] (and before offsets[0]) are never written in any output.  A lane finds its shape by a binary
 * search of the clamped offsets (at most 16 steps; one search per wave where the wave's rows fall in one shape).  Plain vector
 * stores.
 */
int nsdp_handle_rows_ragged(const float *cano, const float *src, const int32_t *offsets, const float *bounds,
                            const uint32_t *params, const uint8_t *handle_mask, const uint8_t *move_mask, int B, int cap,
                            float *rows, float *tgt, uint8_t *handle_out, uint8_t *move_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NSDP_HANDLES_RAGGED_H_ */
