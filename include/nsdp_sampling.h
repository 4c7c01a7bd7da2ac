/*
 * nsdp_sampling.h -- farthest-point sampling of large clouds by a cluster of workgroups (libnsdp_hip.so, ABI version 12).
 *
 * nsdp_furthest_point_sampling (nsdp_hip.h) gives a cloud to ONE workgroup; up to 8192 points the cloud lives in that
 * workgroup's registers, above it the kernel re-reads the cloud and a running-distance scratch from memory at every one of
 * the `nsamples` dependent steps.  The entries here cut a cloud into `groups` slices of at most 8192 points, each
 * register-resident in a workgroup of its own, and exchange one 8-byte arg-max key per workgroup and step through the
 * workspace.  The key is the one the single-workgroup kernels maximise, {bits(min-dist) : tie priority}, a maximum over all
 * points whatever the partition: the indices are those of nsdp_furthest_point_sampling (of the reference), ties included,
 * for every `groups`.
 *
 * The conventions are those of nsdp_hip.h: device pointers + sizes, outputs and the workspace allocated by the caller and
 * possibly UNINITIALISED on entry, `stream` a hipStream_t passed as void*, 0 / negative NSDP_E* / positive hipError_t as the
 * return value, the message in nsdp_last_error().  A call touches exactly idx_out and the first
 * nsdp_fps_cluster_workspace_bytes(...) bytes of the workspace.  It initialises the workspace itself, stream-ordered (one
 * memset in front of the kernels): a workspace an earlier call used needs no cleaning, and a captured call is correct on
 * every replay.  A workspace must not be shared by calls that may run at the same time.
 *
 * Waiting.  The workgroups of a cloud wait for each other at every step, so they must all be resident: a launch holds at most
 * one workgroup per compute unit of the device, and a batch with more clouds than that is split by the host into consecutive
 * launches on `stream`.  Every wait is bounded (2 s on the constant-rate clock).  A workgroup whose wait runs out sets a
 * status word in the workspace, waits no more during that launch and carries on with the best key it has seen; the other
 * workgroups stop waiting as soon as they see the word.  The indices written are then wrong numbers inside the cloud (inside
 * the packed rows), never a fault, and nsdp_fps_cluster_status reports it.
 *
 * tests/test_fps_cluster_arena_gpu.py holds the two launching entries to this inside the poisoned arena.
 */
#ifndef NSDP_SAMPLING_H_
#define NSDP_SAMPLING_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NSDP_ETIMEOUT (-3)  /* a bounded wait between workgroups ran out (nsdp_fps_cluster_status) */

/* The workgroups per cloud the entries below take for groups = 0: ceil(n_max / 8192) for 8192 < n_max <= 262144, and 0
 * where the cluster does not serve by default (n_max <= 8192: one workgroup holds the cloud; n_max > 262144: too large). */
int nsdp_fps_cluster_groups(int n_max);

/* Bytes of workspace a call with these arguments uses (groups = 0: the default for n_max).  0 for arguments the entries
 * refuse.  Monotone in every argument over the arguments they accept. */
size_t nsdp_fps_cluster_workspace_bytes(int B, int n_max, int nsamples, int groups);

/* furthest_point_sampling(points(B,N,3), nsamples) -> idx_out(B,nsamples) i32, the result of nsdp_furthest_point_sampling.
 * groups: 0 = the default (NSDP_EINVAL where that is 0), or 1..32 with N <= groups * 8192 -- honoured for any such N; a
 * workgroup whose slice is empty takes part in the exchange with the key of a lane without a point.
 * B <= 0 or nsamples <= 0: nothing to do, 0. */
int nsdp_furthest_point_sampling_cluster(const float *xyz, int B, int N, int nsamples, int groups, void *workspace,
                                         int32_t *idx_out, void *stream);

/* The same over a packed set, the mirror of nsdp_furthest_point_sampling_ragged: xyz_packed(cap,3) + offsets(B+1) i32 on the
 * device (clamped as that entry clamps them; the host never reads them) -> idx_out(B,nsamples) of PACKED rows.  n_max bounds
 * any shape's row count (the kernel clamps to it) and, with groups = 0, chooses the cluster size; every shape of the set is
 * sampled by `groups` workgroups.  A shape without rows gets its clamped first row in every slot.  B <= 0: nothing to do. */
int nsdp_furthest_point_sampling_cluster_ragged(const float *xyz_packed, const int32_t *offsets, int B, int cap, int n_max,
                                                int nsamples, int groups, void *workspace, int32_t *idx_out, void *stream);

/* Synchronises `stream` and reads the status word of a workspace whose last use was one of the two calls above: 0, or
 * NSDP_ETIMEOUT if a wait gave up (the indices of that call are not to be trusted). */
int nsdp_fps_cluster_status(const void *workspace, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NSDP_SAMPLING_H_ */
