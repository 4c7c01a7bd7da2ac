/*
 * nsdp_search.h -- exact k-nearest-neighbour search of large clouds through a uniform cell grid (libnsdp_hip.so, ABI version 13).
 *
 * nsdp_knn / nsdp_knn_ragged_source (nsdp_hip.h) test every query against every source point of its shape.  The entries here
 * bin the source points of every shape into the cells of a grid over the shape's bounding box and search a query's own cell and
 * shells of growing Chebyshev radius around it, until the list holds k entries whose last distance is strictly below a
 * conservative lower bound of the distance to any point not yet visited.  The list is ordered by the pair (distance, index), a
 * strict total order, and the distance is the scan's expression (nsdp::sq_dist3, one rounding per operation): the k best are
 * unique, so the indices and the distance bits are those of the scan entries, exact ties and duplicates included, whatever
 * order the binning leaves the points in.  The bound is formed in the box's own frame (coordinates minus the box's corner), so
 * it does not depend on where the cloud sits.  A query opens shells while its rows read plus distance tests stay within 64 + m / 4
 * (none if it lies farther outside the box than the box's largest extent); one that gives up (a far outlier, a query far
 * outside) is finished by an exhaustive scan of its shape that the 64 lanes of its wave carry out together.
 *
 * The conventions are those of nsdp_sampling.h: device pointers + sizes, outputs and the workspace allocated by the caller and
 * possibly UNINITIALISED on entry, `stream` a hipStream_t passed as void*, 0 / negative NSDP_E* / positive hipError_t as the
 * return value, the message in nsdp_last_error().  A call touches exactly idx_out, dist_out and the first
 * nsdp_knn_grid_workspace_bytes(...) bytes of the workspace.  It initialises the workspace itself, stream-ordered (one memset
 * in front of the kernels): a workspace an earlier call used needs no cleaning, and a captured call is correct on every replay.
 * The phases (bounds, cells, binning, search) are separate launches on `stream`; no workgroup waits for another inside a
 * kernel.  The host never reads an offsets tensor.  A workspace must not be shared by calls that may run at the same time.
 *
 * Limits: k <= 32, at most 1 048 576 source points per shape (m, n_max), B <= 65535.  Any size inside them is honoured, down
 * to m = k = 1.  Non-finite coordinates are out of contract for the result, as in nsdp_knn; they cannot form an address
 * outside the workspace (a cell coordinate is clamped as a float, NaN to cell 0, before it becomes an integer).
 *
 * tests/test_knn_grid_arena_gpu.py holds the two launching entries to this inside the poisoned arena, and
 * tests/test_knn_grid_anywhere_arena_gpu.py on clouds far from the origin, volumes and queries that all take the finish.
 */
#ifndef NSDP_SEARCH_H_
#define NSDP_SEARCH_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace a call uses: B shapes, `queries` / `source_rows` the totals (B * n / B * m, or qcap / cap of packed
 * sets), m_max the bound of a shape's source points (m, or n_max).  0 for arguments the entries refuse and for empty work.
 * Monotone in every argument over the arguments they accept. */
size_t nsdp_knn_grid_workspace_bytes(int B, int queries, int source_rows, int m_max);

/* knn(query(B,n,3), source(B,m,3), k) -> idx_out(B,n,k) i32 ascending by (distance, index) and, unless NULL,
 * dist_out(B,n,k): the bits of nsdp_knn.  query == source with n == m (the self-search) takes the queries in cell order.
 * B <= 0, n <= 0 or k <= 0: nothing to do, 0. */
int nsdp_knn_grid(const float *query, const float *source, int B, int n, int m, int k, void *workspace, int32_t *idx_out,
                  float *dist_out, void *stream);

/* The same against a packed source set, the mirror of nsdp_knn_ragged_source in both its forms: source(cap,3) + offsets(B+1)
 * i32 on the device (clamped as that entry clamps them), n_max the bound of a shape's rows (the kernels clamp to it); queries
 * rectangular (query_offsets NULL: query(B,n,3) -> idx_out(B,n,k)) or packed (query(qcap,3) + query_offsets(B+1) ->
 * idx_out(qcap,k); rows at or beyond query_offsets[B] are not written).  Indices are PACKED rows of `source`; a shape with
 * fewer than k rows gets its clamped first row and FLT_MAX in the empty slots, as the scan gives them. */
int nsdp_knn_grid_ragged_source(const float *query, const int32_t *query_offsets, const float *source, const int32_t *offsets,
                                int B, int n, int qcap, int cap, int n_max, int k, void *workspace, int32_t *idx_out,
                                float *dist_out, void *stream);

/* Synchronises `stream` and reports on the call that last used the workspace: out = {queries, distance tests, queries
 * finished by the exhaustive scan, cells allocated}.  (Each workgroup of the search leaves one partial in the workspace; this call
 * sums them on the host.) */
int nsdp_knn_grid_stats(const void *workspace, void *stream, int64_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* NSDP_SEARCH_H_ */
