/*
 * nsdp_scatter.h -- inverse neighbour lists of large index sets, built by many workgroups (libnsdp_hip.so, ABI version 14).
 *
 * A scatter-add by index (the backward of a gather: an attention block's d(kf) / d(vf), index_points' gradient) is a sum over
 * the INVERSE of the index map.  nsdp_knn_invert (nsdp_hip.h) builds that inverse with one workgroup per shape and its counters
 * in LDS, for up to 32 768 sources; the entry here builds the same lists as a counting sort in global memory -- count, scan,
 * fill, order, each a launch of its own over the whole chip -- for up to 1 048 576 sources and 33 554 432 entries per shape.
 * The consumers (nsdp_segment_sum_rows*, nsdp_scatter_cm_lists, nsdp_three_interpolate_grad_lists) take its output unchanged.
 *
 * Output: entries[b][offsets[b][s] .. offsets[b][s+1]) is the ascending list of the e in [0, E) with idx[b][e] == s, and
 * offsets[b][N] == E.  EVERY list is ascending, whatever its length (nsdp_knn_invert leaves lists of more than 1024 entries in
 * the order its atomics retired), so the result is unique: the stable sort of e by idx[b][e].  Only integer atomics are used,
 * and nothing of the result depends on the order in which they retire.
 *
 * The conventions are those of nsdp_search.h: device pointers + sizes, outputs and the workspace allocated by the caller and
 * possibly UNINITIALISED on entry, `stream` a hipStream_t passed as void*, 0 / negative NSDP_E* / positive hipError_t as the
 * return value, the message in nsdp_last_error().  A call touches exactly offsets, entries and the first
 * nsdp_knn_invert_wide_workspace_bytes(...) bytes of the workspace (4-byte aligned).  It initialises the workspace itself,
 * stream-ordered (a zeroing launch in front of the others): a captured call is kernel nodes alone and correct on every replay.  No workgroup waits for
 * another inside a kernel.  A workspace must not be shared by calls that may run at the same time; it may be freed (stream-
 * ordered) as soon as the call has been enqueued.
 *
 * Limits: 1 <= N <= 1 048 576, 1 <= E <= 33 554 432 (the cell-grid search's largest cloud at k = 32), 1 <= B <= 65535; index
 * products are formed in 64 bits.  An index outside [0, N) is clamped into the range before it forms an address (it counts
 * for source 0 or N - 1): a stale or poisoned index tensor cannot make the call write outside its outputs and workspace.
 *
 * tests/test_invert_wide_arena_gpu.py holds the launching entry to this inside the poisoned arena.
 */
#ifndef NSDP_SCATTER_H_
#define NSDP_SCATTER_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace a call uses for B shapes of E entries over N sources.  0 for arguments the entry refuses. */
size_t nsdp_knn_invert_wide_workspace_bytes(int B, int E, int N);

/* idx(B,E) i32 -> offsets(B,N+1) i32, entries(B,E) i32 as described above. */
int nsdp_knn_invert_wide(const int32_t *idx, int B, int E, int N, void *workspace, int32_t *offsets, int32_t *entries,
                         void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NSDP_SCATTER_H_ */
