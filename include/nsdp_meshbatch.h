/*
 * nsdp_meshbatch.h -- training batches sampled from device-resident MESH sequences, libnsdp_hip.so (ABI version 23): what the
 * reference's preprocessing writes once per template (an area-weighted face, a barycentric weight and a normal offset per row,
 * applied to every frame) is drawn afresh for every row of every batch, inside the launch that writes nsdp_batch_assemble's four
 * tensors (nsdp_amd/meshstore.py is the store and the loader around it).
 *
 * The conventions are those of nsdp_batch.h: device pointers + sizes, outputs allocated by the caller and possibly
 * UNINITIALISED on entry, `stream` a hipStream_t passed as void*, 0 / negative NSDP_E* / positive hipError_t as the return
 * value, the message in nsdp_last_error().  Sizes are judged before pointers and pointers before the launch; the host reads no
 * device memory; a call touches exactly the bytes declared here and there is no workspace.  Every frame id, topology id, first
 * record, count, vertex index taken from the face arena and the result of the search is clamped as the kernel reads it, so a
 * stale table or face gives wrong numbers and never an access outside the operands.  tests/test_mesh_store_arena_gpu.py holds
 * the entry to this inside the poisoned arena.
 *
 * ---------------------------------------------------------------------------------------------------------------------------
 * The store.  Three arenas of RECORDS and two tables:
 *   vertex arena    (vert_rows, 4) f32:  x y z 0 of one vertex                         (16 bytes: one load, never across a line)
 *   face arena      (face_rows, 4) i32:  a b c 0, vertex indices LOCAL to the frame    (16 bytes)
 *   threshold arena (thr_rows)     u32:  the area thresholds T of every frame that is a canonical frame, one per face
 *   frame_table (n_frames, 6) i64, per frame:
 *     [0] first vertex record   [1] vertex count | topology id << 32   [2] first threshold row, or -1: the frame has none
 *     [3] bits of bbox_min.x | bbox_min.y << 32   [4] bbox_min.z | bbox_max.x << 32   [5] bbox_max.y | bbox_max.z << 32
 *   the bounding box (fp32) of the frame's VERTICES (a surface sample never leaves it, up to the roundings of its three products)
 *   topo_table (n_topos, 2) i64, per topology:  [0] first face record   [1] face count
 * Frames of one topology share one block of faces; the three frames of a sample must share a topology (a face index is the
 * correspondence), and the kernel takes the faces of the CANONICAL frame's topology for all three.
 * As read: a frame id is clamped to [0, n_frames); a vertex count to [0, min(vert_rows, 2^21)]; a first vertex record to
 * [0, vert_rows - count]; a topology id to [0, n_topos); a face count F to [0, min(face_rows, thr_rows, 2^21)]; a first face
 * record to [0, face_rows - F]; a first threshold row to [0, thr_rows - F] (so -1 reads row 0 on); a face f to [0, max(F - 1, 0)]
 * and its record to [0, face_rows); a vertex index to [0, max(count - 1, 0)] and its record to [0, vert_rows).
 *
 * Thresholds (built on the host, nsdp_amd/meshstore.py:area_thresholds):  area[f] = |cross(b - a, c - a)| in float64 from the
 * stored fp32 vertices, cdf = cumsum(area), T[f] = floor(cdf[f] / cdf[F-1] * 2^31), and T[f] = 2^31 from the last face of positive
 * area onwards: non-decreasing, T[f] == T[f-1] (T[0] == 0) at a face of zero area.
 *
 * ---------------------------------------------------------------------------------------------------------------------------
 * The rule per row j of sample b.  All arithmetic is on unsigned 32-bit integers modulo 2^32, or fp32 with ONE rounding per
 * operation (no fused multiply-add, no reciprocal, no rsqrt; sqrtf and / correctly rounded).  tests/mesh_sample_ref.py is the
 * numpy emulation, bit for bit.  mix32 and absorb are nsdp_batch.h's.
 *
 *   key      = nsdp_subset_draw's key, with `which` = NSDP_DRAW_MESH_SURFACE for surface rows, NSDP_DRAW_MESH_SPACE for space rows
 *   rk[c]    = mix32(key + 0x85EBCA6B * (c + 1)),  c = 0 .. 3
 *   word(c)  = mix32(mix32(j ^ rk[c]) + rk[c])
 *   face:      r = word(0) >> 1;  lo = 0, hi = F;  while lo < hi: mid = (lo + hi) >> 1;  T[mid] > r ? hi = mid : lo = mid + 1;
 *              f = min(lo, F - 1): the first face with T[f] > r over the CANONICAL frame's thresholds (it exists: T[F-1] = 2^31 > r;
 *              a face of zero area has T[f] == T[f-1] and is never the first).  At most 22 probes.
 *   weights:   iu = word(1) >> 8, iv = word(2) >> 8;  if iu + iv > 2^24: iu = 2^24 - iu, iv = 2^24 - iv;  iw = 2^24 - iu - iv;
 *              w0 = iw * 2^-24, u = iu * 2^-24, v = iv * 2^-24  -- that is u = (word(1) >> 8) * 2^-24, v likewise, reflected to
 *              (1 - u, 1 - v) where u + v > 1, w0 = (1 - u) - v, with the comparison made on the integers (fp32 would round
 *              1 + 2^-24 to 1); every value is exact in fp32, (w0 + u) + v == 1 exactly, uniform on the triangle.
 *   per frame (canonical, source, target), with the same face (a, b, c) and weights, per component:
 *     p      = ((w0 * a) + (u * b)) + (v * c)
 *     e1 = b - a, e2 = c - a;  cr = (e1.y * e2.z - e1.z * e2.y,  e1.z * e2.x - e1.x * e2.z,  e1.x * e2.y - e1.y * e2.x)
 *     len    = sqrtf((cr.x * cr.x + cr.y * cr.y) + cr.z * cr.z);   nrm = cr / len per component, (0, 0, 0) when len == 0
 *   space rows: t = 2 * ((word(3) >> 8) * 2^-24) - 1 (exact);  d = t * sigma, sigma = sigma1 for j < m / 2 (integer division),
 *     else sigma2;  q = p + nrm * d per component, with that frame's own normal.  Only q is written, no normals.
 *   surface rows, as nsdp_batch_assemble:  src' = src + noise_level * noise (src where noise is NULL);  the handle rule on the
 *     canonical p and the canonical frame's box;  inputs = src' | tgt * mask | mask.
 * The reference's preprocessing draws Dirichlet(1,1,1) weights and offsets uniform in [-sigma, sigma) once per template; this rule
 * draws the same distributions afresh per (seed, epoch, step, b, j).
 */
#ifndef NSDP_MESHBATCH_H_
#define NSDP_MESHBATCH_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NSDP_MESH_MAX_ELEMS (1 << 21)  /* vertices of a frame, and faces of a topology */
#define NSDP_DRAW_MESH_SURFACE 2       /* `which` of the key: beside NSDP_DRAW_SURFACE (0) and NSDP_DRAW_SPACE (1) of nsdp_batch.h, */
#define NSDP_DRAW_MESH_SPACE 3         /* so the draws of one step never share a stream with the row subsets */

/* frame_ids (3, B) i32: the canonical, source and target frame of every sample (the caller has applied `inverse`);
 * noise (B, n, 3) f32 or NULL.  Outputs, all written whole, with nsdp_batch_assemble's layout:
 *   surface_out (6, B, n, 3) f32:  samples cano, src', tgt | normals cano, src, tgt
 *   handle_out  (B, n) u8:         1 where cano.y < bbox_min.y + partial_range or cano.y > bbox_max.y - partial_range or
 *                                  cano.z < bbox_min.z + partial_range (fp32, one rounding per operation), else 0
 *   inputs_out  (B, n, 7) f32:     src' xyz | tgt xyz * mask | mask, mask = 0.f or 1.f (one multiply: -x * 0 = -0)
 *   space_out   (3, B, m, 3) f32:  samples cano, src, tgt
 * B == 0, or n == 0 and m == 0: nothing to do, 0.  Negative sizes, B > 65535, n or m > 2^20, B * max(n, m) >= 2^27,
 * n_frames < 1, n_topos < 1, vert_rows / face_rows / thr_rows < 1, a partial_range, noise_level, sigma1 or sigma2 that is not
 * finite: NSDP_EINVAL; then null and misaligned pointers (the outputs of a part with no rows may be NULL; the arenas 16-byte,
 * the tables 8-byte, everything else 4-byte aligned). */
int nsdp_mesh_batch_sample(const float *vert_arena, long long vert_rows, const int32_t *face_arena, long long face_rows,
                           const uint32_t *thr_arena, long long thr_rows, const int64_t *frame_table, int n_frames,
                           const int64_t *topo_table, int n_topos, const int32_t *frame_ids, int B, int n, int m, uint64_t seed,
                           uint32_t epoch, uint32_t step, float partial_range, float sigma1, float sigma2, const float *noise,
                           float noise_level, float *surface_out, uint8_t *handle_out, float *inputs_out, float *space_out,
                           void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NSDP_MESHBATCH_H_ */
