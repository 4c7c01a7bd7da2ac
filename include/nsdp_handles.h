/*
 * nsdp_handles.h -- user-handle drags on the device (libnsdp_hip.so, ABI version 15).
 *
 * The reference's interactive editing (dataset/utils.py: cano_handle_user_define) marks head, tail and feet of a mesh as handles by
 * a bounding-box rule, translates one of them and lets the network deform every vertex.  The two entries here are that rule as
 * kernels whose drag parameters live in DEVICE memory: a captured graph that contains them serves every drag -- the host writes
 * eight words per shape and replays.
 *
 *   nsdp_handle_bounds   per-shape bounding box of a cloud (once per source mesh);
 *   nsdp_handle_rows     per point: the handle / move predicates, the dragged target and columns 3..6 of the [n, 7] rows the
 *                        deformation network's encoder reads (nsdp_amd/edit.py keeps columns 0..2, which no drag changes).
 *
 * The conventions are those of nsdp_search.h / nsdp_scatter.h: device pointers + sizes, outputs and the workspace allocated by
 * the caller and possibly UNINITIALISED on entry, `stream` a hipStream_t passed as void*, 0 / negative NSDP_E* / positive
 * hipError_t as the return value, the message in nsdp_last_error().  Sizes are checked before any pointer is looked at, pointers
 * (null, 4-byte alignment of the 32-bit operands) before anything is launched.  Index products are formed in 64 bits.  No
 * atomics of any kind; no workgroup waits for another.
 *
 * Limits: 1 <= B <= 65535, 1 <= n <= 1 048 576.
 *
 * tests/test_handles_arena_gpu.py holds both launching entries inside the poisoned arena.
 */
#ifndef NSDP_HANDLES_H_
#define NSDP_HANDLES_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Words of a shape's drag parameters: params(B,8), 32-bit each. */
enum {
  NSDP_HANDLE_PART = 0,     /* i32: which region moves, NSDP_HANDLE_HEAD .. NSDP_HANDLE_BEHINDRIGHTFOOT; any other value: none */
  NSDP_HANDLE_CLIPTAIL = 1, /* i32: non-zero = the tail also needs z > -partial_range */
  NSDP_HANDLE_RANGE = 2,    /* f32: partial_range */
  NSDP_HANDLE_DX = 3,       /* f32 x 3: the translation of the moved region */
  NSDP_HANDLE_DY = 4,
  NSDP_HANDLE_DZ = 5,
  NSDP_HANDLE_PARAM_WORDS = 8 /* (words 6 and 7: zero, not read) */
};

/* The parts, in the priority order of the reference's if / elif chain. */
enum {
  NSDP_HANDLE_HEAD = 0,
  NSDP_HANDLE_TAIL = 1,
  NSDP_HANDLE_FRONTLEFTFOOT = 2,
  NSDP_HANDLE_FRONTRIGHTFOOT = 3,
  NSDP_HANDLE_BEHINDLEFTFOOT = 4,
  NSDP_HANDLE_BEHINDRIGHTFOOT = 5
};

/* Bytes of workspace nsdp_handle_bounds uses for B shapes of n points.  0 for arguments the entry refuses. */
size_t nsdp_handle_bounds_workspace_bytes(int B, int n);

/*
 * cano(B,n,3) f32 -> bounds(B,6) f32: per shape min x, min y, min z, max x, max y, max z.
 *
 * Many workgroups per shape write partial extremes into the workspace (every word of the declared size is written by the call
 * itself, stream-ordered, before it is read), one workgroup per shape reduces them: two launches, kernel nodes alone under a
 * capture.  The comparison is the total order of the fp32 bit patterns (sign-magnitude made monotonic), so the result is the
 * exact extreme and does not depend on how the points were split: -0.0 sorts below +0.0 (a shape that holds both as its
 * extreme gets -0.0 as the minimum and +0.0 as the maximum); a NaN sorts beyond the infinity of its sign and so becomes the
 * bound it touches.  The workspace (4-byte aligned) must not be shared by calls that may run at the same time.
 */
int nsdp_handle_bounds(const float *cano, int B, int n, void *workspace, float *bounds, void *stream);

/*
 * One lane per point.  Inputs: cano(B,n,3), src(B,n,3), bounds(B,6) f32; params(B,8) as above; handle_mask, move_mask (B,n) u8,
 * both null (the rule below decides) or both non-null (non-zero bytes are the handle / the moved points; the rule, cano and
 * bounds are then not read and cano / bounds may be null).
 *
 * The rule, in fp32 with one rounding per operation (the file is built without contraction), lo / hi = the shape's bounds,
 * r = partial_range, (x, y, z) = the point's cano row:
 *     head = y < lo.y + r          tail = y > hi.y - r   [cliptail: and z > -r]          foot = z < lo.z + r
 *     handle = head | tail | foot
 *     frontleftfoot = foot & x > 0 & y < 0     frontrightfoot = foot & x < 0 & y < 0
 *     behindleftfoot = foot & x > 0 & y > 0    behindrightfoot = foot & x < 0 & y > 0
 *     move = the region `part` names
 * All comparisons are strict; a NaN compares false.
 *
 * Outputs (rows is required, the others may be null), with m = move as 0.0f / 1.0f and h = handle as 0.0f / 1.0f, computed as
 * these literal products and sums -- so that signed zeros and NaNs come out as the array expressions src + d * m and tgt * h
 * give them:
 *     tgt(B,n,3)      = src + d * m
 *     rows(B,n,7)     columns 3..5 = tgt * h, column 6 = h; COLUMNS 0..2 ARE NEVER WRITTEN
 *     handle_out, move_out (B,n) u8 = 0 / 1
 * Only rows of the B shapes are touched.  Plain vector stores.
 */
int nsdp_handle_rows(const float *cano, const float *src, const float *bounds, const uint32_t *params,
                     const uint8_t *handle_mask, const uint8_t *move_mask, int B, int n, float *rows, float *tgt,
                     uint8_t *handle_out, uint8_t *move_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NSDP_HANDLES_H_ */
