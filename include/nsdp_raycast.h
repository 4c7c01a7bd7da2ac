/*
 * nsdp_raycast.h -- rays against packed triangle meshes, libnsdp_hip.so (ABI version 28): for every ray the first face it
 * meets (its parameter t, the face and, optionally, the barycentric weights) and, optionally, the number of faces it crosses.
 * nsdp_amd/ray_cast.py wraps it (cast_rays, contains, volume_iou).
 *
 * The conventions are those of nsdp_surface.h: device pointers + sizes, dense row-major tensors, outputs and the workspace
 * allocated by the caller and possibly UNINITIALISED on entry, `stream` a hipStream_t passed as void*, 0 / negative NSDP_E* /
 * positive hipError_t as the return value, the message in nsdp_last_error().  Sizes are judged before pointers and pointers
 * before anything is launched.  One layout, the packed one: rows(cap,3) + offsets(B+1) i32 on the device for the rays, the
 * vertices and the faces; every offsets entry is clamped to [previous entry, cap] as the kernels read it and every vertex index
 * is clamped into its mesh's range before it forms an address, so a stale tensor gives wrong numbers and never an access
 * outside the operands.  The host reads no device memory: the grid is sized from B and the capacities, and a captured launch
 * is valid for any offsets.  Only the bytes declared here are touched; every byte of the workspace that is read was written by
 * the same call.  Integer atomics only: two runs give the same bits.
 *
 * Limits (those of nsdp_mesh_closest): 1 <= B <= 65535 and up to 1 048 576 rays, vertices and faces per shape; the entry sees
 * the capacities alone and refuses qcap, vcap or fcap outside 1 .. 1 048 576 * B (all below 2^31), and flags other than bit 0.
 * inf / NaN coordinates are out of contract, as for nsdp_knn.
 *
 * tests/ray_cast_ref.py is the rule below in numpy, operation by operation; tests/test_ray_cast_arena_gpu.py holds the
 * launching entry inside the poisoned arena; tools/raycast_host_check.cpp runs the bad-argument table on the host.
 */
#ifndef NSDP_RAYCAST_H_
#define NSDP_RAYCAST_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* flags of nsdp_mesh_ray_cast */
#define NSDP_RAYCAST_NO_CULL 1 /* bit 0: the plain scan -- every ray tests every face of its mesh */

/* Bytes of workspace of nsdp_mesh_ray_cast: one 8-byte key per ray row, one 4-byte count per ray row, then 6 floats (a
 * bounding box) per block of 64 faces -- fcap / 64 + B + 1 blocks, a mesh's blocks start at its first face:
 * 12 * qcap + 24 * (fcap / 64 + B + 1).  0 for sizes the entry refuses.  Host only. */
size_t nsdp_mesh_ray_cast_workspace_bytes(int B, int qcap, int fcap);

/* origins(qcap,3) f32, dirs(qcap,3) f32 + ray_offsets(B+1), verts(vcap,3) f32 + vert_offsets(B+1), faces(fcap,3) i32 +
 * face_offsets(B+1), the vertex indices of a face LOCAL to its mesh; the rays of shape b meet the mesh of shape b  ->
 * t_out(qcap) f32, face_out(qcap) i32 (a PACKED face row; -1 with t = FLT_MAX where the ray meets nothing), bary_out(qcap,3)
 * f32 or NULL (0 without a face), count_out(qcap) i32 or NULL.  Rows at or beyond ray_offsets[B] are not written.  The point
 * of a hit is o + t d: t is in units of d, which need not be normalised.
 *
 * THE RULE.  fp32 and fp64 as named, every operation rounds once, no contraction.
 *
 *   Ray frame (fp32).  kz = the axis of the largest |d|, the lowest axis on ties; kx = (kz + 1) % 3, ky = (kz + 2) % 3, the
 *   two swapped where d[kz] < 0.  Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz] (correctly rounded divisions).  A ray
 *   whose largest |d| is 0 misses everything (count 0).
 *
 *   Corner (fp32).  For a corner c:  C = c - o,  x = C[kx] - Sx * C[kz],  y = C[ky] - Sy * C[kz],  z = Sz * C[kz].  A function
 *   of the ray and the corner's coordinates alone: faces that share a vertex see the same (x, y, z).
 *
 *   Edge sign.  For the ORDERED pair (P, Q): compare the products Qx * Py and Qy * Px, both exact in fp64 (two 24-bit
 *   significands).  s = +1 where the first is larger, -1 where it is smaller; on equality s = sign(Qy - Py), if that is 0
 *   s = sign(Px - Qx), if that is 0 too s = 0.  This is the sign of the edge function (Qx - px)(Py - py) - (Qy - py)(Px - px)
 *   = (Qx Py - Qy Px) + e (Qy - Py) + e^2 (Px - Qx) at the point p = (e, e^2) for every small enough e > 0: the ray displaced
 *   symbolically.  s(P, Q) = -s(Q, P) always.  The displaced ray is generic: it meets no projected edge and no vertex.
 *
 *   Covered.  Face (a, b, c) is covered where s(b, c), s(c, a), s(a, b) are all +1 or all -1 (both orientations count).  A
 *   face that projects to zero area is never covered: a generic point is strictly inside no segment.
 *
 *   Depth, for a covered face, in fp64:  U = cx * by - cy * bx,  V = ax * cy - ay * cx,  W = bx * ay - by * ax  (the products
 *   exact, each difference rounds once),  det = (U + V) + W,  T = (U * za + V * zb) + W * zc.  The face is HIT where T and det
 *   have strictly the same sign;  t = fp32(T / det),  bary = fp32(U / det), fp32(V / det), fp32(W / det), the weights of a, b, c.
 *   det != 0 on a covered face: U, V, W carry the signs s(b, c), s(c, a), s(a, b) wherever they are not zero (a rounded
 *   difference of two doubles has the sign of the exact one), so they do not cancel; and they are not all zero, because on a
 *   tie s(P, Q) = +1 says Q comes after P in the strict order by (y, then -x), and b < c < a < b is no order.
 *
 *   Results.  count = the number of hit faces of the ray's mesh.  The reported hit is the minimum of the 64-bit keys
 *   (t bits << 32 | packed face row) over the hit faces and the start key (FLT_MAX bits, no face), by integer minima: the
 *   smallest face row wins among equal t bits, whatever the order of the visit.  bary is recomputed for the winner by the same
 *   operations.
 *
 * WHAT FOLLOWS.  Coverage is the EXACT coverage of the projected fp32 corners by a generic point: no rounding enters a sign.
 * So for a closed mesh (every edge used by two faces) the number of covered faces is even for every ray, whatever it is aimed
 * at -- through a vertex, along an edge, in a face's plane.  Only the split of the covered faces by depth (t > 0) rounds.
 * Envelopes, to first order:
 *   t against the exact quotient t* of the same sheared corners:  |t - t*| <= 2^-24 |t*| + 2^-50 max(|za|, |zb|, |zc|)
 *       (U, V, W one fp64 rounding each, a product and at most two sums on every term of T, two sums on det, the quotient: 8
 *       roundings of 2^-53 on terms that do not cancel in det and are at most |det| max|z| in T; then one fp32 rounding);
 *   the sheared corners against the exact shear of c - o by the exact d:  |x - x*|, |y - y*| <= 6 * 2^-24 * R,
 *       |z - z*| <= 3 * 2^-24 * |z*|,  R the largest |component| of c - o (|Sx|, |Sy| <= 1: kz is the largest axis).
 * DESIGN.md 4r derives both.
 *
 * THE SEARCH.  One bounding box per block of 64 consecutive faces (a mesh's blocks start at its first face); one wave per 64
 * rays of a mesh and per part of the mesh's blocks; a visited block's corners are staged once in LDS and every lane tests
 * every staged face.  A block is visited where, for some live lane, the box pushed through the corner's own fp32 operations
 * as intervals contains 0 in x and in y (rounding is monotone, so the intervals hold every sheared corner of the block; no
 * margin).  Without count_out a block is skipped as well where its z interval ends below 0 (no face of it can be hit: its T
 * and det cannot agree in sign) or begins above the lane's best t (every hit of it has larger t bits: the fp64 error is far
 * below half an fp32 ulp); with count_out every block on the ray's line is visited.  NSDP_RAYCAST_NO_CULL visits every block:
 * the same bytes in every form.  Per lane and part one 64-bit integer atomic minimum and one i32 atomic add.
 *
 * workspace: 8-byte aligned, nsdp_mesh_ray_cast_workspace_bytes(B, qcap, fcap) bytes. */
int nsdp_mesh_ray_cast(const float *origins, const float *dirs, const int32_t *ray_offsets, const float *verts,
                       const int32_t *vert_offsets, const int32_t *faces, const int32_t *face_offsets, int B, int qcap, int vcap,
                       int fcap, int flags, void *workspace, float *t_out, int32_t *face_out, float *bary_out, int32_t *count_out,
                       void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NSDP_RAYCAST_H_ */
