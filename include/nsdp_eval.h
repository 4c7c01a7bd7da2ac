/*
 * nsdp_eval.h -- the evaluation-metric entries of libnsdp_hip.so (ABI version 11): what the dense-inference metrics of a
 * whole batch of meshes need on the device (nsdp_amd/eval_metric.py, the mirror of the reference's utils/eval_metric.py).
 *
 * The conventions are those of nsdp_hip.h: device pointers + sizes, dense row-major tensors, outputs allocated by the
 * caller and possibly UNINITIALISED on entry, `stream` a hipStream_t passed as void*, 0 / negative NSDP_E* / positive
 * hipError_t as the return value, the message in nsdp_last_error().  A call touches exactly the bytes declared here; there
 * is no workspace.  Packed sets are laid out as nsdp_hip.h describes them for nsdp_knn_ragged: rows(cap,C) + offsets(B+1)
 * i32 on the device, every entry clamped to [previous entry, cap] as the kernels read it, so a corrupt offsets tensor gives
 * wrong numbers and never an access outside the buffers; the host reads only B and the capacities, and a captured launch is
 * valid for any offsets.  tests/test_eval_batch_arena_gpu.py holds the three entries to this inside the poisoned arena.
 */
#ifndef NSDP_EVAL_H_
#define NSDP_EVAL_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Squared distance of every query point to the nearest source point of its shape, and (idx_out != NULL) that point's
 * index: query(B,n,3), source(B,m,3) -> dist2_out(B,n) f32, idx_out(B,n) i32 or NULL.  dist2_out has the bits of
 * nsdp_knn(..., k = 1)'s distance -- ((dx*dx + dy*dy) + dz*dz), dx = query - source, one rounding per operation -- and
 * idx_out is nsdp_knn's index, the smallest among exact ties.  inf / NaN coordinates are out of contract, as for nsdp_knn.
 * m < 1: NSDP_EINVAL; B * n <= 0: nothing to do, 0.  Without an index the source range is split over workgroups and the
 * partial minima are combined by an integer minimum on the distance bits (exact and order-independent; no floating-point
 * atomics); dist2_out is initialised by the call itself.  With an index one workgroup scans the whole source of its
 * queries, or -- where that would leave most of the chip idle -- a second split pass finds the smallest index at exactly the
 * minimum's bits, by an integer minimum into idx_out (initialised by the call as well). */
int nsdp_nn_dist2(const float *query, const float *source, int B, int n, int m, float *dist2_out, int32_t *idx_out,
                  void *stream);

/* The same search with both sets packed: query(qcap,3) + query_offsets(B+1), source(scap,3) + source_offsets(B+1) ->
 * dist2_out(qcap), idx_out(qcap) or NULL, the index a PACKED source row.  Element for element the result of
 * nsdp_knn_ragged_source at k = 1.  Rows at or beyond query_offsets[B] are not written.  A shape without source rows gets
 * FLT_MAX and min(its first source row, scap - 1).  scap < 1: NSDP_EINVAL; B <= 0 or qcap <= 0: nothing to do, 0. */
int nsdp_nn_dist2_ragged(const float *query, const int32_t *query_offsets, const float *source, const int32_t *source_offsets,
                         int B, int qcap, int scap, float *dist2_out, int32_t *idx_out, void *stream);

/* Per-shape mean of a packed column: values(cap) f32, offsets(B+1) -> out(B) f32, the mean over shape b's rows of v
 * (transform 0) or of sqrtf(fmaxf(v, 0)) (transform 1).  One workgroup per shape, a fixed thread-to-row assignment
 * relative to the shape's first row, double accumulation and a fixed-order combine: out[b] is a function of that shape's
 * rows alone -- the same bits whatever else the set holds, wherever the shape sits, and from run to run.  A shape without
 * rows gives NaN (the mean of nothing). */
int nsdp_segment_mean_f32(const float *values, const int32_t *offsets, int B, int cap, int transform, float *out,
                          void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NSDP_EVAL_H_ */
