/*
 * nsdp_meshwhole.h -- WHOLE meshes of a batch out of the device-resident mesh store, libnsdp_hip.so (ABI version 24): what the
 * reference's loader returns with `load_mesh` (every vertex of the canonical, source and target mesh of a sample, the handle mask
 * of the canonical vertices, the 7-wide input rows and the faces), for B samples of DIFFERENT vertex and face counts, packed
 * back to back with offsets -- the layout the packed decoder, the packed metrics and the packed editing session take
 * (nsdp_amd/meshstore.py: MeshStore.whole_meshes is the call around it, nsdp_amd/evaluate.py the loop that uses it).
 *
 * The conventions are those of nsdp_meshbatch.h, and the store is the one that header lays out: the vertex arena, the face arena,
 * frame_table and topo_table are read as they are; the threshold arena is not needed.  Device pointers + sizes, outputs
 * allocated by the caller and possibly UNINITIALISED on entry, `stream` a hipStream_t passed as void*, 0 / negative NSDP_E* /
 * positive hipError_t as the return value, the message in nsdp_last_error().  Sizes are judged before values, values before
 * pointers, pointers before alignment, all of it before the launch; the host reads no device memory; a call touches exactly the
 * bytes declared here and there is no workspace.  Two kernel launches and nothing else (under a capture: two kernel nodes), no
 * atomics, and no workgroup waits for another.  Every frame id, topology id, first record, count and vertex index is clamped as
 * the kernel reads it, so a stale table or face gives wrong numbers and never an access outside the operands.
 * tests/test_mesh_whole_arena_gpu.py holds the entry to this inside the poisoned arena.
 *
 * ---------------------------------------------------------------------------------------------------------------------------
 * The rule.  tests/mesh_whole_ref.py is the numpy emulation, bit for bit.  frame_ids (3, B) i32 names the canonical, source and
 * target frame of every shape b (the caller has applied `inverse`); each id is clamped to [0, n_frames).
 *
 *   V_b  = the vertex count of the CANONICAL frame (the low 32 bits of its word [1], as a signed number), clamped to
 *          [0, min(vert_rows, 2^21)];
 *   F_b  = the face count of the canonical frame's topology (its id clamped to [0, n_topos)), clamped to
 *          [0, min(face_rows, 2^21)] -- nsdp_mesh_batch_sample's clamps, without the threshold arena's term;
 *   the source and the target frame are read with the canonical frame's count V_b (the three frames of a sample share a topology,
 *   so their own counts are the same number in a store that is in order); each of the three frames' own first vertex record is
 *   clamped to [0, vert_rows - V_b], the topology's first face record to [0, face_rows - F_b].
 *
 *   vert_offsets[0] = 0,  vert_offsets[b + 1] = min(vert_offsets[b] + V_b, vcap)      (sums in 64 bits)
 *   face_offsets[0] = 0,  face_offsets[b + 1] = min(face_offsets[b] + F_b, fcap)
 * A batch that does not fit its capacities is TRUNCATED: the shape that crosses the capacity keeps its first rows, the shapes
 * behind it are empty.  That gives wrong numbers (a face of a truncated shape may name a vertex that was cut) and never an access
 * outside the operands; a caller that knows the counts refuses such a batch before the launch (the Python wrapper does, from the
 * host copy of the tables).
 *
 * Vertex row r in [vert_offsets[b], vert_offsets[b + 1]) belongs to shape b; with i = r - vert_offsets[b]:
 *   verts_out[0][r], [1][r], [2][r]  = x y z of record (first record + i) of the canonical, source and target frame
 *   handle_out[r]                    = 1 where cano.y < bbox_min.y + partial_range or cano.y > bbox_max.y - partial_range or
 *                                      cano.z < bbox_min.z + partial_range, with the box of the CANONICAL frame (fp32, one
 *                                      rounding per operation: nsdp_meshbatch.h's handle rule, one definition for both), else 0
 *   inputs_out[r]                    = src xyz | tgt xyz * mask | mask,  mask = 0.f or 1.f (one multiply: -x * 0 = -0)
 * Face row q in [face_offsets[b], face_offsets[b + 1]), with i = q - face_offsets[b]:
 *   faces_out[q]                     = a b c of record (first face record + i), each clamped to [0, max(V_b - 1, 0)], as a
 *                                      12-byte row.  The indices stay LOCAL to the shape, as the packed metrics take them.
 * Rows at or beyond the totals (vert_offsets[B] <= r < vcap, face_offsets[B] <= q < fcap) are written as zeros: every byte of
 * every output is written by the call.
 */
#ifndef NSDP_MESHWHOLE_H_
#define NSDP_MESHWHOLE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Outputs, all written whole:
 *   vert_offsets (B + 1) i32, face_offsets (B + 1) i32
 *   verts_out  (3, vcap, 3) f32:  the canonical, source and target plane
 *   handle_out (vcap) u8
 *   inputs_out (vcap, 7) f32
 *   faces_out  (fcap, 3) i32
 * B == 0: nothing to do, 0 (nothing is written).  B outside [0, 65535], vcap or fcap outside [1, 2^27), n_frames < 1,
 * n_topos < 1, vert_rows / face_rows < 1, a partial_range that is not finite: NSDP_EINVAL; then null pointers; then misaligned
 * ones (the arenas 16-byte, the tables 8-byte, everything else but handle_out 4-byte aligned). */
int nsdp_mesh_batch_whole(const float *vert_arena, long long vert_rows, const int32_t *face_arena, long long face_rows,
                          const int64_t *frame_table, int n_frames, const int64_t *topo_table, int n_topos,
                          const int32_t *frame_ids, int B, int vcap, int fcap, float partial_range, int32_t *vert_offsets,
                          int32_t *face_offsets, float *verts_out, uint8_t *handle_out, float *inputs_out, int32_t *faces_out,
                          void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NSDP_MESHWHOLE_H_ */
