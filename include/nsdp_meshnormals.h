/*
 * nsdp_meshnormals.h -- per-vertex normals of packed triangle meshes, libnsdp_hip.so (ABI version 26): the area-weighted vertex
 * normal of every vertex of B meshes of DIFFERENT vertex and face counts, for P poses of the one topology, without a floating-
 * point atomic: a vertex's normal is the fixed-order sum of its incident faces' normals over its ascending list of corners.
 * The lists depend on the topology alone and are built once (nsdp_mesh_corner_lists); a pose then costs two launches
 * (nsdp_mesh_vertex_normals).  nsdp_amd/mesh_normals.py holds the calls around them (MeshTopology, vertex_normals).
 *
 * The conventions are those of nsdp_meshwhole.h: device pointers + sizes, outputs and the workspace allocated by the caller and
 * possibly UNINITIALISED on entry, every byte of every output written by the call, `stream` a hipStream_t passed as void*,
 * 0 / negative NSDP_E* / positive hipError_t as the return value, the message in nsdp_last_error().  Sizes are judged before
 * values, values before pointers, pointers before alignment, all of it before the launch; the host reads no device memory; a
 * call touches exactly the bytes declared here.  Integer atomics only (the counting sort's), nothing of any result depends on the
 * order in which they retire; no workgroup waits for another; under a capture a call is kernel nodes alone.
 * tests/test_mesh_normals_arena_gpu.py holds both launching entries inside the poisoned arena.
 *
 * The mesh layout is the one nsdp_mesh_batch_whole writes: faces (fcap, 3) i32 with indices LOCAL to the shape, face_offsets
 * (B + 1) and vert_offsets (B + 1) i32 on the device, non-decreasing from 0 and within the capacities; rows at or beyond the
 * totals (face_offsets[B] <= q < fcap, vert_offsets[B] <= r < vcap) belong to nobody.  Offsets are clamped as they are read
 * (csrc/packed_rows.h, the text the packed handle kernels use), so offsets that are not of that form give wrong numbers and
 * never an access outside the operands.
 *
 * ---------------------------------------------------------------------------------------------------------------------------
 * The rule.  tests/mesh_normals_ref.py is the numpy emulation, bit for bit.
 *
 * Corners.  Face row q is LIVE when a shape b owns it (face_offsets[b] <= q < face_offsets[b + 1]), DEAD otherwise.  With
 * n_b = vert_offsets[b + 1] - vert_offsets[b], corner c = 3 q + j of a live face names packed vertex row
 *     row(c) = min(vert_offsets[b] + clamp(faces[q][j], 0, max(n_b - 1, 0)), vcap - 1):
 * a stale index is clamped into its shape.  (A shape with faces and no vertex is malformed: its corners name the row behind
 * it, whoever owns that.  The Python wrapper refuses such a mesh.)
 *
 * Lists.  list_entries[list_offsets[r] .. list_offsets[r + 1]) is the ASCENDING list of the live corners c with row(c) == r.
 * Corners of dead faces are in no list, rows r >= vert_offsets[B] have empty lists, list_offsets[vcap] = 3 * face_offsets[B] is
 * the number of live corners, and list_entries[list_offsets[vcap] .. 3 fcap) is written as zeros.  The lists are the stable sort
 * of the live corners by row: unique.
 *
 * Faces.  For pose p and a live face q whose corners name rows a, b, c, with the positions P = verts[p]:
 *     e1 = P_b - P_a,  e2 = P_c - P_a                                            (component-wise, one rounding each)
 *     N_q = (e1y e2z - e1z e2y,  e1z e2x - e1x e2z,  e1x e2y - e1y e2x)          (each product rounded, then the difference)
 * the area-weighted normal, twice the face's area long, outward for counter-clockwise faces.  face_normals[p][q] = N_q,
 * unnormalised; dead face rows are written as +0.
 *
 * Vertices.  s_r = the sum of N_{c / 3} over the corner list of row r in csrc/list_reduce.h's documented order -- what
 * tests/list_order_ref.ordered_sum gives for the terms in ascending corner order: one lane up to 32 entries, a wave up to 1024,
 * the workgroup beyond.  sums[p][r] = s_r where `sums` is given.  With m = max(|sx|, |sy|, |sz|):
 *     m == 0, or a component of s is not finite:   normals[p][r] = (+0, +0, +0)
 *         (an isolated vertex, a vertex whose faces are all degenerate, faces that cancel, an overflow);
 *     otherwise   t = s / m,   qn = (tx tx + ty ty) + tz tz,   normals[p][r] = t / sqrtf(qn)
 *         (IEEE division and square root, one rounding per operation; qn lies in [1, 3]).
 * Dividing by m first keeps tiny and huge meshes away from under- and overflow, and a mesh scaled by a power of two keeps its
 * normals' bits.  Rows r >= vert_offsets[B] have empty lists: +0 in sums and normals.  Subnormal inputs and intermediates
 * follow the translation unit's build flags; they are not part of the contract.
 *
 * Other weightings (by angle, uniform) are not built.
 */
#ifndef NSDP_MESHNORMALS_H_
#define NSDP_MESHNORMALS_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Limits of both entries (nsdp_knn_invert_wide's, whose phases build the lists): 1 <= B <= 65535, 1 <= vcap <= 1 048 576,
 * 1 <= fcap, 3 fcap <= 33 554 432. */

/* Bytes of workspace nsdp_mesh_corner_lists uses.  0 for arguments the entry refuses. */
size_t nsdp_mesh_corner_lists_workspace_bytes(int B, int vcap, int fcap);

/* faces (fcap, 3) i32, face_offsets (B + 1) i32, vert_offsets (B + 1) i32 -> list_offsets (vcap + 1) i32, list_entries (3 fcap)
 * i32, both written whole.  The workspace (16-byte aligned, the byte count of the query above) is initialised by the call
 * itself, stream-ordered; it must not be shared by calls that may run at the same time.  A size outside the limits:
 * NSDP_EINVAL, by name; then null pointers; then misaligned ones (4-byte: everything but the workspace). */
int nsdp_mesh_corner_lists(const int32_t *faces, const int32_t *face_offsets, const int32_t *vert_offsets, int B, int vcap, int fcap,
                           void *workspace, int32_t *list_offsets, int32_t *list_entries, void *stream);

/* verts (P, vcap, 3) f32: P >= 1 poses of the one topology (P <= 65535) -- the T poses of a track; a rectangular [B, V, 3] batch
 * over one shared face table, taken as B = 1 and P = B; a single mesh.  list_offsets / list_entries: what nsdp_mesh_corner_lists
 * wrote for these faces and offsets (read clamped: stale lists give wrong numbers, never an access outside the operands).
 * Outputs, written whole: face_normals (P, fcap, 3) f32, sums (P, vcap, 3) f32 or NULL, normals (P, vcap, 3) f32.  Two kernel
 * launches: the faces, then the vertices.  Sizes outside the limits: NSDP_EINVAL, by name; then null pointers (sums may be
 * null); then misaligned ones (4-byte). */
int nsdp_mesh_vertex_normals(const float *verts, int P, const int32_t *faces, const int32_t *face_offsets, const int32_t *vert_offsets,
                             int B, int vcap, int fcap, const int32_t *list_offsets, const int32_t *list_entries, float *face_normals,
                             float *sums, float *normals, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NSDP_MESHNORMALS_H_ */
