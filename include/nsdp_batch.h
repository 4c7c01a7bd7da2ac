/*
 * nsdp_batch.h -- training batches from a device-resident data set, libnsdp_hip.so (ABI version 22): the random row subsets of
 * a batch without a sort, and the reference's per-sample tensor contract (dataset/dataset_deform4d_flow.py:174-246) for a whole
 * batch in one launch that reads only the rows it keeps (nsdp_amd/datastore.py is the store and the loader around them).
 *
 * The conventions are those of nsdp_eval.h: device pointers + sizes, outputs allocated by the caller and possibly
 * UNINITIALISED on entry, `stream` a hipStream_t passed as void*, 0 / negative NSDP_E* / positive hipError_t as the return
 * value, the message in nsdp_last_error().  Sizes are judged before pointers and pointers before any launch; the host reads no
 * device memory; a call touches exactly the bytes declared here and there is no workspace.  Every frame id, row offset, row
 * count and row index is clamped as the kernels read it, so a stale tensor gives wrong numbers and never an access outside the
 * operands.  tests/test_datastore_arena_gpu.py holds both entries to this inside the poisoned arena.
 *
 * ---------------------------------------------------------------------------------------------------------------------------
 * The draw.  Row j of sample b is pi(j), pi a keyed bijection of [0, n): distinct rows without sorting n random keys.  All
 * arithmetic is on unsigned 32-bit integers, modulo 2^32 (tests/subset_ref.py is the numpy emulation, bit for bit):
 *
 *   mix32(x):      x ^= x >> 16;  x *= 0x7FEB352D;  x ^= x >> 15;  x *= 0x846CA68B;  x ^= x >> 16          (a bijection of 2^32)
 *   absorb(h, v) = mix32((h ^ v) + 0x9E3779B9)
 *   key          = absorb(absorb(absorb(absorb(absorb(absorb(0x4E534450, seed & 0xFFFFFFFF), seed >> 32), epoch), step), b), which)
 *   rk[r]        = mix32(key + 0x85EBCA6B * (r + 1)),  r = 0 .. 7
 *   n            = min(max(n_full[b], 1), 2^20)
 *   h            = max(1, ceil(w / 2)),  w the smallest integer with 2^w >= n;  mask = 2^h - 1            (h <= 10)
 *   E(x), 0 <= x < 2^(2h):  L = x >> h, R = x & mask;  eight times, r = 0 .. 7:  (L, R) = (R, L ^ (mix32(R ^ rk[r]) >> (32 - h)));
 *                           E(x) = (L << h) | R
 *   pi(j), 0 <= j < n:      x = E(j);  while x >= n: x = E(x);  pi(j) = x
 *   rows_out[b, j] = pi(j mod n)
 *
 * E is a balanced Feistel network, a bijection of [0, 2^(2h)) whatever its round function is (every round is undone by
 * (L, R) = (R ^ F(L), L)); 2^(2h) is the smallest power of FOUR that holds n, so n <= 2^(2h) < 4 n.  Walking E's cycle from j < n
 * until it re-enters [0, n) ends (the cycle returns to j at the latest) and maps [0, n) onto itself one to one: two starting
 * points that met in one x would share the walk backwards through E^-1 to its first element below n.  So for n_keep <= n the
 * rows are distinct, and n_keep == n gives a full permutation.  One lane per output row, fewer than four evaluations of E on
 * average.  n_keep > n_full[b] is outside the contract (rows repeat from j = n on) but stays inside [0, n).
 */
#ifndef NSDP_BATCH_H_
#define NSDP_BATCH_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NSDP_BATCH_MAX_ROWS (1 << 20)  /* rows of one frame the draw addresses, and the largest n_keep / n / m */
#define NSDP_DRAW_SURFACE 0            /* `which`: the stream of the surface rows */
#define NSDP_DRAW_SPACE 1              /* ... and of the space rows */

/* n_full(B) i32 -> rows_out(B, n_keep) i32, as written out above; `which` is NSDP_DRAW_SURFACE or NSDP_DRAW_SPACE.
 * B == 0 or n_keep == 0: nothing to do, 0.  B < 0, B > 65535, n_keep < 0, n_keep > NSDP_BATCH_MAX_ROWS, B * n_keep >= 2^31 or an
 * unknown `which`: NSDP_EINVAL.  Every element of rows_out is written. */
int nsdp_subset_draw(const int32_t *n_full, int B, int n_keep, uint64_t seed, uint32_t epoch, uint32_t step, int which,
                     int32_t *rows_out, void *stream);

/* The store.  Frames live in two packed arenas of RECORDS, in the files' own number format (`*_f16` != 0: IEEE binary16, else
 * binary32; the conversion to fp32 is exact):
 *   surface arena (surface_rows, 6):  point x y z | normal x y z of one surface sample   (12 or 24 bytes: one row, one record)
 *   space arena   (space_rows, 4):    point x y z | 0                                    ( 8 or 16 bytes, naturally aligned)
 * so a kept surface row costs one piece of memory for its point AND its normal, and no record of either arena straddles a 64-byte
 * line more than its size forces (space records never do).  Both arenas must be 16-byte aligned.
 * frame_table (n_frames, 6) i64, per frame:
 *   [0] first surface record   [1] first space record   [2] surface rows | space rows << 32
 *   [3] bits of bbox_min.x | bbox_min.y << 32   [4] bbox_min.z | bbox_max.x << 32   [5] bbox_max.y | bbox_max.z << 32
 * the bounding box (fp32) of the frame's FULL surface cloud -- what the handle mask of a canonical frame needs, so that a batch
 * needs no reduction.  As read: a frame id is clamped to [0, n_frames); a row count to [0, arena rows]; a first record to
 * [0, arena rows - count]; a row index to [0, max(count, 1)); the record address to the arena.
 *
 * frame_ids (3, B) i32: the canonical, source and target frame of every sample (the caller has applied `inverse`);
 * surf_idx (B, n) i32 rows within a frame's surface records, the same row of all three frames (correspondences);
 * space_idx (B, m) i32 or NULL (rows 0 .. m-1); noise (B, n, 3) f32 or NULL.  Outputs, all written whole:
 *   surface_out (6, B, n, 3) f32:  samples cano, src, tgt | normals cano, src, tgt
 *   handle_out  (B, n) u8:         1 where cano.y < bbox_min.y + partial_range or cano.y > bbox_max.y - partial_range or
 *                                  cano.z < bbox_min.z + partial_range (fp32, one rounding per operation), else 0
 *   inputs_out  (B, n, 7) f32:     src' xyz | tgt xyz * mask | mask, mask = 0.f or 1.f (one multiply: -x * 0 = -0)
 *   space_out   (3, B, m, 3) f32:  samples cano, src, tgt
 * src' = src + noise_level * noise (one rounding per operation; also what surface_out holds as the source samples), src where
 * noise is NULL.  B == 0, or n == 0 and m == 0: nothing to do, 0.  Negative sizes, B > 65535, n or m > NSDP_BATCH_MAX_ROWS,
 * B * max(n, m) >= 2^27, n_frames < 1, arena rows < 1 (of an arena that is read: n > 0 / m > 0), a partial_range or noise_level
 * that is not finite: NSDP_EINVAL; then null and misaligned pointers (those of a part with no rows may be NULL). */
int nsdp_batch_assemble(const void *surface_arena, long long surface_rows, int surface_f16, const void *space_arena,
                        long long space_rows, int space_f16, const int64_t *frame_table, int n_frames, const int32_t *frame_ids,
                        int B, const int32_t *surf_idx, int n, const int32_t *space_idx, int m, float partial_range,
                        const float *noise, float noise_level, float *surface_out, uint8_t *handle_out, float *inputs_out,
                        float *space_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NSDP_BATCH_H_ */
