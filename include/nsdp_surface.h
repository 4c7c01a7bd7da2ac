/*
 * nsdp_surface.h -- exact point-to-mesh distance of libnsdp_hip.so (ABI version 21): for every query point the closest point of
 * a triangle mesh -- its squared distance, its face and (optionally) its barycentric coordinates.  nsdp_amd/surface_distance.py
 * wraps it; nsdp_amd/eval_metric.scan_metrics_batch scores a prediction against a scan with it.
 *
 * The conventions are those of nsdp_eval.h: device pointers + sizes, dense row-major tensors, outputs and the workspace
 * allocated by the caller and possibly UNINITIALISED on entry, `stream` a hipStream_t passed as void*, 0 / negative NSDP_E* /
 * positive hipError_t as the return value, the message in nsdp_last_error().  Sizes are judged before pointers and pointers
 * before anything is launched.  One layout, the packed one of nsdp_nn_dist2_ragged: rows(cap,3) + offsets(B+1) i32 on the device
 * for the queries, the vertices and the faces; every offsets entry is clamped to [previous entry, cap] as the kernels read it
 * and every vertex index is clamped into its mesh's range before it forms an address, so a stale tensor gives wrong numbers and
 * never an access outside the operands.  The host reads no device memory: the grid is sized from B and the capacities, and a
 * captured launch is valid for any offsets.  Only the bytes declared here are touched; every byte of the workspace that is read
 * was written by the same call.  No floating-point atomics: two runs give the same bits.
 *
 * Limits: 1 <= B <= 65535 and up to 1 048 576 queries, vertices and faces per shape; the entry sees the capacities alone and
 * refuses qcap, vcap or fcap outside 1 .. 1 048 576 * B (all below 2^31), and flags other than bits 0 and 1.  inf / NaN
 * coordinates are out of contract, as for nsdp_knn.
 *
 * tests/test_surface_distance_arena_gpu.py holds the launching entry inside the poisoned arena;
 * tools/surface_host_check.cpp runs the bad-argument table on the host.
 */
#ifndef NSDP_SURFACE_H_
#define NSDP_SURFACE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* flags of nsdp_mesh_closest */
#define NSDP_SURFACE_NO_CULL 1  /* bit 0: the plain scan -- every query tests every face of its mesh */
#define NSDP_SURFACE_NO_BOUND 2 /* bit 1: culling without the bound pass -- every query starts from FLT_MAX (the measured form) */

/* Bytes of workspace of nsdp_mesh_closest: one 8-byte key per query row, then 6 floats (a bounding box) per block of 64
 * faces -- fcap / 64 + B + 1 blocks, a mesh's blocks start at its first face: 8 * qcap + 24 * (fcap / 64 + B + 1).  0 for
 * sizes the entry refuses.  Host only. */
size_t nsdp_mesh_closest_workspace_bytes(int B, int qcap, int fcap);

/* query(qcap,3) f32 + query_offsets(B+1), verts(vcap,3) f32 + vert_offsets(B+1), faces(fcap,3) i32 + face_offsets(B+1), the
 * vertex indices of a face LOCAL to its mesh ->  dist2_out(qcap) f32, face_out(qcap) i32 (a PACKED face row), bary_out(qcap,3)
 * f32 or NULL.  Rows at or beyond query_offsets[B] are not written.  A shape without faces (or without vertices) gives
 * FLT_MAX, face -1 and bary 0.
 *
 * Arithmetic (every operation rounds once, no contraction), for query p and a face with corners a, b, c, in the query's frame:
 *   A = a - p, B = b - p, C = c - p                                   (so the error follows the triangle as seen from the query,
 *                                                                      not the size of the coordinates)
 *   edge (P, Q), for (A,B), (A,C), (B,C):  e = Q - P, ee = (e.x e.x + e.y e.y) + e.z e.z, tn = -((P.x e.x + P.y e.y) + P.z e.z),
 *       t = 0 where ee == 0 or tn <= 0, 1 where tn >= ee, else tn / ee;   X = P + t e;   d = (X.x X.x + X.y X.y) + X.z X.z
 *   interior, with ab, ac the first two edge vectors: g11 = ab.ab, g12 = ab.ac, g22 = ac.ac, r1 = -(A.ab), r2 = -(A.ac),
 *       det = g11 g22 - g12 g12,  v = g22 r1 - g12 r2,  w = g11 r2 - g12 r1;   taken where det > 2^-20 (g11 g22), v > 0, w > 0
 *       and v + w < det:   b1 = v / det, b2 = w / det,   X = (A + b1 ab) + b2 ac,   d as above
 *   dist2 = the smallest d, candidates in the order AB, AC, BC, interior, a later one replacing an earlier only where smaller.
 * Every candidate is a point of the triangle, so the seven regions (three corners as t = 0 / 1, three edges, the interior) are
 * covered without a region test that could pick a wrong formula; a face with two or three equal corners or collinear corners
 * is the segment or point it is (ee == 0 gives t = 0, det fails its test), no division by zero is formed and no NaN reaches an
 * output.  A query that is bitwise a corner of a face gets exactly 0 (P = 0 gives tn = 0, Q = 0 gives tn = ee exactly).
 * Envelope, to first order, R2 the largest squared distance from the query to the face's corners:
 *   |dist2 - exact| <= 17 * 2^-24 * R2        (DESIGN.md 4k derives it).
 *
 * The minimum is over the 64-bit key (dist2 bits << 32 | packed face row), by integer minima only (in registers, then one
 * 64-bit atomic minimum per query and part of the face range): the result does not depend on how the faces are split over
 * workgroups or in which order they are visited; among faces whose dist2 bits tie the smallest face row wins.
 *
 * bary_out: recomputed for the winning face alone by the same operations: (1 - t, t, 0) placed on the edge's corners, or
 * (max(0, (1 - b1) - b2), b1, b2); entries >= 0, sum 1 within rounding.
 *
 * The search: one bounding box per block of 64 consecutive faces (a mesh's blocks start at its first face); every query
 * starts from the smallest, over blocks, of the largest squared distance to a box, raised by 2^-19 of itself and rounded up
 * (some whole face lies inside each box); a wave of 64 queries visits a block only where, for some query of the wave,
 * lo2 - 2^-19 hi2 <= best (lo2 / hi2 the smallest / largest squared distance to the box as computed) -- a block it skips
 * holds no face whose computed dist2 could reach the best.  NSDP_SURFACE_NO_CULL starts from FLT_MAX and visits
 * every block; NSDP_SURFACE_NO_BOUND starts from FLT_MAX and votes: the same bits in every form.
 *
 * workspace: 8-byte aligned, nsdp_mesh_closest_workspace_bytes(B, qcap, fcap) bytes. */
int nsdp_mesh_closest(const float *query, const int32_t *query_offsets, const float *verts, const int32_t *vert_offsets,
                      const int32_t *faces, const int32_t *face_offsets, int B, int qcap, int vcap, int fcap, int flags,
                      void *workspace, float *dist2_out, int32_t *face_out, float *bary_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NSDP_SURFACE_H_ */
