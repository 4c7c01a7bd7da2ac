/*
 * nsdp_selfintersect.h -- self-intersections of packed triangle meshes, libnsdp_hip.so (ABI version 27): for every face of B
 * meshes of DIFFERENT vertex and face counts, for P poses of the one topology, how many faces of its own mesh it passes
 * through.  nsdp_amd/self_intersect.py holds the calls around the entry (SelfIntersectionPlan, self_intersections).
 *
 * The conventions are those of nsdp_surface.h: device pointers + sizes, outputs and the workspace allocated by the caller and
 * possibly UNINITIALISED on entry, `stream` a hipStream_t passed as void*, 0 / negative NSDP_E* / positive hipError_t as the
 * return value, the message in nsdp_last_error().  Sizes are judged before pointers and pointers before anything is launched.
 * The layout is the packed one of nsdp_mesh_batch_whole: verts (P, vcap, 3) f32, faces (fcap, 3) i32 with indices LOCAL to the
 * mesh, vert_offsets / face_offsets (B + 1) i32 on the device; every offsets entry is clamped to [previous entry, cap] as the
 * kernels read it and every vertex index into its mesh before it forms an address, so a stale tensor gives wrong numbers and
 * never an access outside the operands.  The host reads no device memory: the grid follows from P, B and the capacities, and a
 * captured launch is valid for any offsets.  Only the bytes declared here are touched; every byte of the workspace that is read
 * was written by the same call.  Integer atomics only (two counters per pose and mesh): two runs give the same bytes.
 * tests/test_self_intersect_arena_gpu.py holds the launching entry inside the poisoned arena;
 * tools/selfintersect_host_check.cpp runs the bad-argument table on the host.
 *
 * Limits, those of nsdp_mesh_closest: 1 <= B <= 65535, vcap and fcap in 1 .. 1 048 576 * B (all below 2^31); 1 <= P <= 65535;
 * budget >= 0; flags other than bit 0 are refused.  inf / NaN coordinates are out of contract.
 *
 * ---------------------------------------------------------------------------------------------------------------------------
 * The rule.  This text is the definition; tests/self_intersect_ref.py is its numpy emulation, operation by operation.
 *
 * A face row q is LIVE when a mesh b owns it (face_offsets[b] <= q < face_offsets[b + 1], clamped) and that mesh has at least
 * one vertex.  Its corners c0, c1, c2 are the positions of vertex rows vert_offsets[b] + clamp(faces[q][k], 0, n_b - 1).
 * Two live faces i != j of ONE mesh INTERSECT when (a), (b) and (c) hold.
 *
 * (a) They are not adjacent: no corner of i equals a corner of j AS COORDINATES (all three floats compare equal, so -0 == +0).
 *     Equal vertex indices give equal coordinates, so faces that share a vertex are adjacent; so are faces that meet in a
 *     duplicated seam vertex of an .obj file, and the faces of a bitwise coincident copy of a mesh.  None of these is reported.
 * (b) Their face boxes overlap.  The box of a face is the per-axis minimum and maximum of its three corners; the intervals are
 *     closed and the comparisons exact: lo_i <= hi_j and lo_j <= hi_i on every axis.  This is part of the rule, not only a
 *     speed-up: every form of culling by boxes that contain the face boxes is sound by definition.
 * (c) Some edge of one pierces the other.  Six sub-tests: the segments (c0, c1), (c1, c2), (c2, c0) of i against the triangle
 *     j, and the same with the roles swapped.  A sub-test is a function of (the segment in its face's own corner order, the
 *     triangle in its own corner order) alone, so test(i, j) == test(j, i).  Segment (p, q) pierces triangle (a, b, c) where
 *         sp = (p - a) . ((b - a) x (c - a))   and   sq = (q - a) . ((b - a) x (c - a))   have strictly opposite signs
 *             (sp > 0 and sq < 0, or sp < 0 and sq > 0), and
 *         t1 = (q - p) . ((a - p) x (b - p)),  t2 = (q - p) . ((b - p) x (c - p)),  t3 = (q - p) . ((c - p) x (a - p))
 *             are all > 0 or all < 0.
 *     Arithmetic: fp32; every subtraction, product and sum rounds once, no contraction; u x v = (u.y v.z - u.z v.y,
 *     u.z v.x - u.x v.z, u.x v.y - u.y v.x); u . v = (u.x v.x + u.y v.y) + u.z v.z.
 *
 * The signs are strict: touching, coplanar and zero-area configurations are NOT intersections (a zero-area face is pierced
 * by nothing: sp = sq = 0 as a triangle; its edges are ordinary segments and may still pierce another face).
 * Envelope, to first order, R the largest coordinate difference among the corners involved: each of the five determinants is within 46 * 2^-24 * R^3 of its exact value
 * (DESIGN.md 4q derives it); a sub-test whose exact determinants all exceed that bound is decided as in exact arithmetic.
 *
 * THE LIMIT.  Two faces that share a corner can still fold through each other; (a) excludes them and the rule does not report
 * that.  Telling such a fold from the ordinary contact of neighbours needs another test, which is not built.
 *
 * cand(i) = the number of faces j that satisfy (a) and (b) with i.  The work guard: with budget > 0 a face whose cand exceeds
 * budget is SKIPPED; a pair is tested and counted only where BOTH faces are within the budget.  budget = 0: no guard.  The
 * result stays symmetric and a function of the input whatever the visiting order.  (A collapsed prediction puts every face
 * into every other's box: F^2 narrow tests, minutes at the face limit.)
 *
 * Reported rows.  face_ids (fcap) i32, or NULL for the identity: the row under which packed face row q is reported, so that
 * a caller may reorder a mesh's faces for locality and still get answers in its own numbering.  face_ids[q] is clamped into
 * its own mesh's range of packed face rows as it is read; it must be one-to-one on every mesh's live rows (a table that is
 * not gives wrong numbers, never an access outside the operands).
 */
#ifndef NSDP_SELFINTERSECT_H_
#define NSDP_SELFINTERSECT_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* flags of nsdp_mesh_self_intersections */
#define NSDP_SELFINT_NO_CULL 1 /* bit 0: no culling by blocks of faces -- every block of the mesh is visited; the same bytes out */

/* Bytes of workspace of nsdp_mesh_self_intersections: per pose 9 floats (the corners) and one i32 (cand in packed order) per
 * face row and 6 floats (a bounding box) per block of 64 faces -- fcap / 64 + B + 1 blocks, a mesh's blocks start at its first
 * face: 4 * P * (10 * fcap + 6 * (fcap / 64 + B + 1)).  0 for sizes the entry refuses.  Host only. */
size_t nsdp_mesh_self_intersections_workspace_bytes(int P, int B, int fcap);

/* verts (P, vcap, 3) f32, vert_offsets (B + 1), faces (fcap, 3) i32, face_offsets (B + 1), face_ids (fcap) i32 or NULL ->
 *   cand_out (P, fcap) i32     at the reported row of a live face: cand
 *   hits_out (P, fcap) i32     ... the number of faces it intersects (both within the budget); -1 for a skipped face
 *   partner_out (P, fcap) i32  ... the smallest reported row (a PACKED face row) among those faces, or -1
 *   pairs_out (P, B) i64       unordered intersecting pairs of every mesh (both faces within the budget)
 *   skipped_out (P, B) i32     skipped faces of every mesh
 * Every element of every output is written; rows nobody owns (and the rows of a mesh without vertices) get 0 / 0 / -1.
 *
 * The search: one bounding box per block of 64 consecutive faces and pose (a mesh's blocks start at its first face); a
 * workgroup of 1 .. 8 waves owns a block, a lane of each wave a face; a block of the mesh is visited, by one of the waves, only
 * where the two blocks' boxes overlap (closed, exact -- a face box lies inside its block's box, so (b) fails for every pair of
 * a block that is skipped): the wave stages its corners, face boxes, cand and reported rows in LDS and every lane tests its
 * face against each staged face.  Every face finds all of its partners itself: no atomics on rows.  Pass 1 writes cand, pass 2 the rest; budget = 0 needs one pass.  NSDP_SELFINT_NO_CULL visits
 * every block.
 *
 * workspace: 16-byte aligned, nsdp_mesh_self_intersections_workspace_bytes(P, B, fcap) bytes; everything else 4-byte aligned
 * (pairs_out 8-byte).  Refused, by name, in this order: P, B, vcap, fcap, budget, flags; then null pointers (face_ids may be
 * null); then misaligned ones. */
int nsdp_mesh_self_intersections(const float *verts, int P, const int32_t *vert_offsets, const int32_t *faces,
                                 const int32_t *face_offsets, const int32_t *face_ids, int B, int vcap, int fcap, int budget, int flags,
                                 void *workspace, int32_t *cand_out, int32_t *hits_out, int32_t *partner_out, int64_t *pairs_out,
                                 int32_t *skipped_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NSDP_SELFINTERSECT_H_ */
