/*
 * nsdp_geodesic.h -- geodesic distances over the edge graph of packed triangle meshes, libnsdp_hip.so (ABI version 29): for
 * every vertex of B meshes of DIFFERENT vertex and face counts, for P poses of the one topology, the length of the shortest
 * path along mesh edges from a set of seed vertices, optionally cut off at a radius.  The edge table depends on the topology
 * (its neighbours) and on the pose (its lengths) and is built in one launch (nsdp_mesh_edge_lengths) over the corner lists of
 * nsdp_meshnormals.h; the distances are the fixed point of a relaxation that a caller runs a number of rounds at a time
 * (nsdp_mesh_geodesic_relax).  nsdp_amd/geodesic.py holds the calls around them (GeodesicPlan, geodesic_distances,
 * geodesic_ball, edge_lengths).
 *
 * The conventions are those of nsdp_meshnormals.h: device pointers + sizes, outputs allocated by the caller and possibly
 * UNINITIALISED on entry (ONE exception: `dist` of nsdp_mesh_geodesic_relax, below), every byte of every output written by the
 * call, `stream` a hipStream_t passed as void*, 0 / negative NSDP_E* / positive hipError_t as the return value, the message in
 * nsdp_last_error().  Sizes are judged before values, values before pointers, pointers before alignment, all of it before the
 * launch; the host reads no device memory; a call touches exactly the bytes declared here.  Integer atomics only (one counter,
 * relaxed loads and stores of the distances' bits); nothing of the fixed point depends on the order in which they retire; no
 * workgroup waits for another; under a capture a call is kernel nodes alone.  tests/test_geodesic_arena_gpu.py holds both
 * launching entries inside the poisoned arena.
 *
 * The mesh layout, the corners, row(c) and the ascending corner lists are nsdp_meshnormals.h's: faces (fcap, 3) i32 with
 * indices LOCAL to the shape, face_offsets / vert_offsets (B + 1) i32 on the device, clamped as they are read;
 * list_offsets (vcap + 1) / list_entries (3 fcap) what nsdp_mesh_corner_lists wrote for them.
 *
 * ---------------------------------------------------------------------------------------------------------------------------
 * The rule.  tests/geodesic_ref.py is the numpy emulation, bit for bit.
 *
 * Edges.  Position e < list_offsets[vcap] of the lists holds the corner list_entries[e] = c = 3 q + j of a live face q.  With
 * a = row(3 q + j), n1 = row(3 q + (j + 1) % 3), n2 = row(3 q + (j + 2) % 3):
 *     nbr[2 e] = n1,  nbr[2 e + 1] = n2                                             (packed vertex rows)
 *     len[p][2 e] = |P_a - P_n1|,  len[p][2 e + 1] = |P_a - P_n2|                    for pose p, P = verts[p], where
 *     |P_a - P_n| = sqrtf((dx dx + dy dy) + dz dz),  d = P_a - P_n component-wise    (one rounding per operation, IEEE sqrt)
 * so positions list_offsets[r] .. list_offsets[r + 1] list every edge of row r once per face that has it.  The length is
 * symmetric in its ends by construction ((-d)(-d) = d d); duplicated edges are kept, a minimum does not mind them.  Positions
 * at or beyond list_offsets[vcap] (clamped to 3 fcap) are written as row 0 and +0.
 *
 * Fixed point.  The limit satisfies limit >= +0, +inf allowed.  A value is SANITISED by its bits as a uint32: a value whose
 * bits exceed the bits of `limit` becomes +inf -- negatives, -0, NaN and everything farther than the limit; call the map S.
 * The result D is the LARGEST array with
 *     D[r] = min( S(dist_in[r]),  min over the entries (u, w) of r's list of S(fl(D[u] + w)) )     for the live rows r,
 * and +inf for the rows at or beyond vert_offsets[B].  fl(d + w) is monotone in d, so the fixed point is unique, is what an
 * fp32 Dijkstra computes when candidates beyond the limit are pruned, and its bits do not depend on the order of relaxation,
 * the block size, the vertex numbering or how many rounds a call runs: every vertex's distance is the minimum over paths from a
 * seed of the left-to-right fp32 sum of the start value and the edge lengths.
 *
 * Termination.  Values only fall and are compared as integers, so a NaN or inf coordinate can never make the iteration run
 * on; every launch is bounded by construction: the inner loop of a workgroup has a fixed cap (NSDP_GEODESIC_BLOCK passes) and
 * an entry runs exactly the number of rounds it is told.  At most (vertices of the largest mesh) rounds lower anything.
 *
 * Exact polyhedral geodesics (through faces), a backward pass, bf16 and soft falloff weights are not built.
 */
#ifndef NSDP_GEODESIC_H_
#define NSDP_GEODESIC_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Limits of both entries (nsdp_mesh_corner_lists's): 1 <= P <= 65535, 1 <= B <= 65535, 1 <= vcap <= 1 048 576, 1 <= fcap,
 * 3 fcap <= 33 554 432. */

/* The vertex rows one workgroup of nsdp_mesh_geodesic_relax owns (a multiple of 256; a build may override it to measure another:
 * the fixed point does not depend on it, nsdp_mesh_geodesic_block() answers what the library was built with). */
#ifndef NSDP_GEODESIC_BLOCK
#define NSDP_GEODESIC_BLOCK 256
#endif
/* flags of nsdp_mesh_geodesic_relax */
#define NSDP_GEODESIC_NO_LOCAL 1      /* one relaxation per round instead of a block relaxed to convergence: the same fixed point */
#define NSDP_GEODESIC_MAX_ROUNDS 1024

/* Elements of nbr and of one pose of len: 2 * 3 * fcap.  0 for sizes the entries refuse. */
size_t nsdp_mesh_edge_table_entries(int B, int vcap, int fcap);
/* Vertex rows per workgroup (NSDP_GEODESIC_BLOCK), for callers that do not read this header. */
int nsdp_mesh_geodesic_block(void);

/* verts (P, vcap, 3) f32, the mesh and its corner lists -> nbr (2 * 3 fcap) i32 or NULL, len (P, 2 * 3 fcap) f32, both written
 * whole.  One launch.  Sizes outside the limits: NSDP_EINVAL, by name; then null pointers (nbr may be null); then misaligned
 * ones (nbr and len 8-byte: they are read as pairs; 4-byte everything else). */
int nsdp_mesh_edge_lengths(const float *verts, int P, const int32_t *faces, const int32_t *face_offsets, const int32_t *vert_offsets,
                           int B, int vcap, int fcap, const int32_t *list_offsets, const int32_t *list_entries, int32_t *nbr, float *len,
                           void *stream);

/* `rounds` rounds of the relaxation over P poses.  dist (P, vcap) f32 is INPUT AND OUTPUT -- the one exception to "outputs may
 * be uninitialised": on entry the seeds (any non-negative value within the limit is a start value, everything else counts as
 * +inf), on return the state after `rounds` rounds, EVERY row written (rows at or beyond vert_offsets[B]: +inf).  Every
 * intermediate state lies between the seeds and the fixed point and sanitising is idempotent, so calling again on the returned
 * dist continues the iteration: no flag.  changed_out (1) i32 is written by the call: the number of (pose, vertex) pairs the
 * LAST round lowered; the fixed point is reached if and only if it is 0.  list_offsets and nbr are read clamped: stale tables
 * give wrong numbers, never an access outside the operands.  rounds + 1 launches: the counter's, then one per round; a vertex
 * has one writer per launch, other workgroups' values are read with relaxed atomic loads and a stale one is a valid upper
 * bound -- correctness rests on the kernel boundary alone.  Refused with NSDP_EINVAL, by name: sizes outside the limits; then
 * a NaN or negative limit (-0 too), rounds outside [1, 1024], unknown flag bits; then null pointers; then misaligned ones (nbr
 * and len 8-byte, 4-byte the rest). */
int nsdp_mesh_geodesic_relax(const int32_t *list_offsets, const int32_t *nbr, const float *len, const int32_t *vert_offsets, int B,
                             int vcap, int fcap, int P, float limit, int rounds, int flags, float *dist, int32_t *changed_out,
                             void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NSDP_GEODESIC_H_ */
