// Evaluation metrics for a whole batch of meshes (include/nsdp_eval.h): the nearest-neighbour DISTANCE search of the Chamfer
// metric and the per-shape means of l2 / normal consistency / Chamfer, over rectangular or packed (ragged.h) point sets.
//
// nn_dist2: knn.hip at k = 1 without what the top-k kernels carry -- no sorted list, no insertion branch and, for the metric,
// no index.  MI355X design:
//   * the source streams through LDS as the plane tile of plane_tile.h (three coordinate planes, sentinels no minimum admits):
//     four candidates are three 16-byte broadcast reads, no range checks in the scan;
//   * a lane holds kQ = 4 queries in registers, so one LDS read serves four distance tests; the distances are plane_tile.h's
//     dist4: the bits of nsdp::sq_dist3, hence of nsdp_knn;
//   * without an index the source range is split over workgroups (grid y) until the grid fills the chip, and the partial
//     minima meet in dist2_out by an INTEGER minimum on the distance bits -- d2 >= 0 makes unsigned order float order, so the
//     result is exact and independent of the order of arrival.  dist2_out is initialised by a kernel of the same call.
//     With an index one workgroup scans the whole source of its queries and writes both outputs itself -- or, where that grid
//     would leave most of the chip idle (the rectangular entry, four or more parts), the split search runs first and a second
//     split pass finds, by an integer minimum again, the smallest index whose distance has the bits of the minimum.  No
//     workspace either way.
// segment_mean: one workgroup per shape, thread t sums the shape's rows t, t + 256, ... in double, then a fixed tree over
// the 256 partial sums: a function of the shape's rows alone, the same bits wherever the shape sits and from run to run.
#include <cfloat>
#include <climits>

#include "../../include/nsdp_eval.h"
#include "common.h"
#include "list_reduce.h"
#include "plane_tile.h"
#include "prof.h"
#include "ragged.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
static_assert(kThreads == nsdp::lists::kThreads, "segment_mean_kernel sums its partial sums through the 256-wide tree");
constexpr int kQ = 4;                      // queries per lane
constexpr int kQueryTile = kThreads * kQ;  // queries per workgroup (1024)
constexpr int kTile = 1024;                // source rows per LDS tile (12 KiB in three planes)
constexpr int kPad = 4;                    // sentinel entries behind the last row: the scan takes four rows at a time

// One workgroup's search.  Queries: rows [row0, min(row0 + kQueryTile, end)) of `query` (row r at query + 3 r); lane t holds rows
// row0 + t + 256 q.  Source: rows [c0, c1) of the m rows at `source`, 0 <= c0, c1 <= m.  `combine`: the workgroup is one of
// several over the source range and dist2_out[row] (initialised to FLT_MAX by the call) takes the minimum of the distance
// bits; else the row is stored.  kMode: kDist the distance alone; kDistIdx the index as well, min(idx_base + index within
// `source`, idx_max), the smallest index among exact ties (candidates are met in increasing order, strict `<`; an empty
// range leaves (FLT_MAX, idx_base)); kMatch the second pass of a split search with an index: dist2_out[row] holds the
// minimum over the whole source, and idx_out[row] (initialised to a valid index by the call) takes the minimum of the
// indices of this workgroup's candidates at exactly that distance -- the same arithmetic gives the same bits.
// Every lane of the workgroup must call it (barriers).
enum { kDist = 0, kDistIdx = 1, kMatch = 2 };

template <int kMode>
__device__ __forceinline__ void nn_scan(const float *__restrict__ query, int row0, int end, const float *__restrict__ source,
                                        int c0, int c1, bool combine, float *__restrict__ dist2_out,
                                        int32_t *__restrict__ idx_out, int idx_base, int idx_max) {
  __shared__ nsdp::PlaneTile<kTile, kPad> tile;
  float qx[kQ], qy[kQ], qz[kQ], best[kQ];
  int bi[kQ];
#pragma unroll
  for (int q = 0; q < kQ; ++q) {
    const int r = row0 + static_cast<int>(threadIdx.x) + q * kThreads;
    qx[q] = qy[q] = qz[q] = 0.f;
    if (r < end) {
      const float *p = query + static_cast<size_t>(r) * 3;
      qx[q] = p[0]; qy[q] = p[1]; qz[q] = p[2];
    }
    best[q] = FLT_MAX;
    bi[q] = kMode == kMatch ? INT_MAX : 0;
    if constexpr (kMode == kMatch) {
      if (r < end) best[q] = dist2_out[r];
    }
  }
  for (int base = c0; base < c1; base += kTile) {
    const int cnt = min(kTile, c1 - base);
    __syncthreads();
    tile.load<kThreads>(source + static_cast<size_t>(base) * 3, cnt);
    __syncthreads();
    for (int t = 0; t < cnt; t += 4) {
      nsdp::f32x4 X, Y, Z;
      tile.read4(t, X, Y, Z);      // once for the lane's kQ queries
#pragma unroll
      for (int q = 0; q < kQ; ++q) {
        nsdp::f32x2 d01, d23;
        nsdp::dist4(X, Y, Z, qx[q], qy[q], qz[q], d01, d23);
        if constexpr (kMode == kDistIdx) {
          const float d[4] = {d01[0], d01[1], d23[0], d23[1]};
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const bool better = d[u] < best[q];
            best[q] = better ? d[u] : best[q];
            bi[q] = better ? base + t + u : bi[q];
          }
        } else if constexpr (kMode == kMatch) {
          // (rare: a lane matches once per exact tie; descending u leaves the smallest index of the four)
          if (fminf(fminf(d01[0], d01[1]), fminf(d23[0], d23[1])) == best[q]) {
            const float d[4] = {d01[0], d01[1], d23[0], d23[1]};
#pragma unroll
            for (int u = 3; u >= 0; --u) bi[q] = (d[u] == best[q] && base + t + u < bi[q]) ? base + t + u : bi[q];
          }
        } else {
          // (a minimum of non-negative, non-NaN values: the order of the operands does not matter)
          best[q] = fminf(best[q], fminf(fminf(d01[0], d01[1]), fminf(d23[0], d23[1])));
        }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < kQ; ++q) {
    const int r = row0 + static_cast<int>(threadIdx.x) + q * kThreads;
    if (r < end) {
      if constexpr (kMode == kMatch) {
        if (bi[q] != INT_MAX) atomicMin(idx_out + r, min(bi[q] + idx_base, idx_max));
      } else if (combine) {
        atomicMin(reinterpret_cast<unsigned int *>(dist2_out + r), __float_as_uint(best[q]));
      } else {
        dist2_out[r] = best[q];
        if constexpr (kMode == kDistIdx) idx_out[r] = min(bi[q] + idx_base, idx_max);
      }
    }
  }
}

// the source rows [c0, c1) of workgroup `part` of `parts` over m rows, in whole LDS tiles; false: nothing for this workgroup
// (an empty part of a split range -- the initialisation already holds FLT_MAX; a single part always runs and stores)
__device__ __forceinline__ bool nn_part(int m, int part, int parts, int &c0, int &c1) {
  const int tiles = (m + kTile - 1) / kTile;
  const int per = (tiles + parts - 1) / parts * kTile;
  c0 = static_cast<int>(min(static_cast<long long>(part) * per, static_cast<long long>(m)));
  c1 = c0 + min(per, m - c0);
  return parts == 1 || c0 < c1;
}

template <int kMode>
__global__ __launch_bounds__(kThreads) void nn_dist2_kernel(const float *__restrict__ query_all,
                                                            const float *__restrict__ source_all, int n, int m,
                                                            float *__restrict__ dist2_all, int32_t *__restrict__ idx_all) {
  const size_t b = blockIdx.z;
  int c0, c1;
  if (!nn_part(m, static_cast<int>(blockIdx.y), static_cast<int>(gridDim.y), c0, c1)) return;
  nn_scan<kMode>(query_all + b * n * 3, static_cast<int>(blockIdx.x) * kQueryTile, n, source_all + b * m * 3, c0, c1,
                 gridDim.y > 1, dist2_all + b * n, kMode != kDist ? idx_all + b * n : nullptr, 0, INT_MAX);
}

// Both sets packed (ragged.h): a workgroup's kQueryTile queries belong to one shape and search that shape's source rows;
// surplus workgroups return as a whole before any barrier; rows at or beyond query_offsets[B] are not written.
template <int kMode>
__global__ __launch_bounds__(kThreads) void nn_dist2_ragged_kernel(const float *__restrict__ query,
                                                                   const int32_t *__restrict__ query_offsets,
                                                                   const float *__restrict__ source,
                                                                   const int32_t *__restrict__ source_offsets, int B, int qcap,
                                                                   int scap, float *__restrict__ dist2_out,
                                                                   int32_t *__restrict__ idx_out) {
  int b, row0, end, lo, hi, c0, c1;
  if (!nsdp::ragged_tile<kQueryTile>(query_offsets, B, qcap, static_cast<int>(blockIdx.x), b, row0, end)) return;
  nsdp::ragged_range(source_offsets, b, scap, lo, hi);
  if (!nn_part(hi - lo, static_cast<int>(blockIdx.y), static_cast<int>(gridDim.y), c0, c1)) return;
  nn_scan<kMode>(query, row0, end, source + static_cast<size_t>(lo) * 3, c0, c1, gridDim.y > 1, dist2_out, idx_out, lo,
                 scap - 1);
}

// dist2_out of a split search: FLT_MAX in every row the call writes -- all `rows` of a rectangular set (offsets NULL), the
// rows of the B shapes of a packed one (clamped as ragged_range clamps them); idx_out (or NULL) of a two-pass search:
// `idx_init`, the last index of the source -- valid whatever the second pass finds
__global__ __launch_bounds__(kThreads) void nn_dist2_init_kernel(const int32_t *__restrict__ offsets, int B, long long rows,
                                                                 int cap, float *__restrict__ dist2_out,
                                                                 int32_t *__restrict__ idx_out, int idx_init) {
  long long first = 0, last = rows;
  if (offsets) {
    int lo, hi;
    nsdp::ragged_range(offsets, 0, cap, lo, hi);
    first = lo;
    nsdp::ragged_range(offsets, B - 1, cap, lo, hi);
    last = hi;
  }
  const long long r = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x;
  if (r >= first && r < last) {
    dist2_out[r] = FLT_MAX;
    if (idx_out) idx_out[r] = idx_init;
  }
}

__global__ __launch_bounds__(kThreads) void segment_mean_kernel(const float *__restrict__ values,
                                                                const int32_t *__restrict__ offsets, int cap, int transform,
                                                                float *__restrict__ out) {
  __shared__ double part[kThreads];
  int lo, hi;
  nsdp::ragged_range(offsets, static_cast<int>(blockIdx.x), cap, lo, hi);
  double acc = 0.0;
  for (int r = lo + static_cast<int>(threadIdx.x); r < hi; r += kThreads) {
    const float v = values[r];
    acc += static_cast<double>(transform ? sqrtf(fmaxf(v, 0.f)) : v);
  }
  part[threadIdx.x] = acc;
  nsdp::lists::tree_sum(part);
  // (an empty shape: 0 / 0 = NaN, the mean of nothing)
  if (threadIdx.x == 0) out[blockIdx.x] = static_cast<float>(part[0] / static_cast<double>(hi - lo));
}

// parts of the source range: until the grid holds four workgroups per compute unit, at least one LDS tile each
int source_parts(long long query_tiles, long long source_rows) {
  const long long tiles = (source_rows + kTile - 1) / kTile;
  const long long want = (4LL * nsdp::num_cus() + query_tiles - 1) / (query_tiles > 0 ? query_tiles : 1);
  long long parts = want < tiles ? want : tiles;
  if (parts < 1) parts = 1;
  if (parts > 65535) parts = 65535;
  return static_cast<int>(parts);
}

}  // namespace

extern "C" int nsdp_nn_dist2(const float *query, const float *source, int B, int n, int m, float *dist2_out, int32_t *idx_out,
                             void *stream) {
  if (B <= 0 || n <= 0) return 0;
  NSDP_REQUIRE(query && source && dist2_out, "nn_dist2: null pointer");
  NSDP_REQUIRE(m >= 1, "nn_dist2: no source points (m=%d)", m);
  NSDP_REQUIRE(B <= 65535, "nn_dist2: batch %d too large for one launch", B);
  NSDP_REQUIRE(static_cast<long long>(B) * n < (1LL << 31), "nn_dist2: %d x %d query rows too large", B, n);
  hipStream_t st = nsdp::as_stream(stream);
  nsdp::prof::Scope scope(nsdp::prof::kKnn, st, 0.0, static_cast<double>(B) * (12.0 * (n + m) + 4.0 * n * (idx_out ? 2 : 1)));
  const int qt = nsdp::ceil_div(n, kQueryTile);
  const int parts = source_parts(static_cast<long long>(qt) * B, m);
  // an index: one pass unsplit, unless that grid is a quarter of the chip or less -- then two split passes (the second costs
  // about as much as the first)
  if (idx_out && parts < 4) {
    NSDP_TRACE("nn_dist2<idx>");
    hipLaunchKernelGGL((nn_dist2_kernel<kDistIdx>), dim3(qt, 1, B), dim3(kThreads), 0, st, query, source, n, m, dist2_out,
                       idx_out);
    return nsdp::launch_status("nn_dist2_kernel");
  }
  NSDP_TRACE("nn_dist2<parts=%d%s>", parts, idx_out ? ",idx" : "");
  if (parts > 1) {
    const long long rows = static_cast<long long>(B) * n;
    hipLaunchKernelGGL(nn_dist2_init_kernel, dim3(nsdp::ceil_div(rows, kThreads)), dim3(kThreads), 0, st, nullptr, B, rows, 0,
                       dist2_out, idx_out, m - 1);
  }
  hipLaunchKernelGGL((nn_dist2_kernel<kDist>), dim3(qt, parts, B), dim3(kThreads), 0, st, query, source, n, m, dist2_out,
                     nullptr);
  if (idx_out)
    hipLaunchKernelGGL((nn_dist2_kernel<kMatch>), dim3(qt, parts, B), dim3(kThreads), 0, st, query, source, n, m, dist2_out,
                       idx_out);
  return nsdp::launch_status("nn_dist2_kernel");
}

extern "C" int nsdp_nn_dist2_ragged(const float *query, const int32_t *query_offsets, const float *source,
                                    const int32_t *source_offsets, int B, int qcap, int scap, float *dist2_out, int32_t *idx_out,
                                    void *stream) {
  if (B <= 0 || qcap <= 0) return 0;
  NSDP_REQUIRE(query && query_offsets && source && source_offsets && dist2_out, "nn_dist2_ragged: null pointer");
  NSDP_REQUIRE(scap > 0, "nn_dist2_ragged: the packed source needs a positive capacity (scap=%d)", scap);
  NSDP_REQUIRE(B <= 65535, "nn_dist2_ragged: batch %d too large for one launch", B);
  hipStream_t st = nsdp::as_stream(stream);
  nsdp::prof::Scope scope(nsdp::prof::kKnn, st, 0.0,
                          12.0 * (static_cast<double>(qcap) + scap) + 4.0 * qcap * (idx_out ? 2 : 1));
  // the host knows the capacities alone: the grid is sized for them, workgroups without rows return
  const long long qt = nsdp::ragged_max_tiles(qcap, B, kQueryTile);
  if (idx_out) {
    NSDP_TRACE("nn_dist2_ragged<idx>");
    hipLaunchKernelGGL((nn_dist2_ragged_kernel<kDistIdx>), dim3(static_cast<unsigned>(qt)), dim3(kThreads), 0, st, query,
                       query_offsets, source, source_offsets, B, qcap, scap, dist2_out, idx_out);
    return nsdp::launch_status("nn_dist2_ragged_kernel");
  }
  // (a shape may own every source row: the parts are cut for that bound, a part beyond a shape's rows returns at once)
  const int parts = source_parts(qt, scap);
  NSDP_TRACE("nn_dist2_ragged<parts=%d>", parts);
  if (parts > 1)
    hipLaunchKernelGGL(nn_dist2_init_kernel, dim3(nsdp::ceil_div(qcap, kThreads)), dim3(kThreads), 0, st, query_offsets, B,
                       static_cast<long long>(qcap), qcap, dist2_out, nullptr, 0);
  hipLaunchKernelGGL((nn_dist2_ragged_kernel<kDist>), dim3(static_cast<unsigned>(qt), parts), dim3(kThreads), 0, st, query,
                     query_offsets, source, source_offsets, B, qcap, scap, dist2_out, nullptr);
  return nsdp::launch_status("nn_dist2_ragged_kernel");
}

extern "C" int nsdp_segment_mean_f32(const float *values, const int32_t *offsets, int B, int cap, int transform, float *out,
                                     void *stream) {
  if (B <= 0) return 0;
  NSDP_REQUIRE(cap >= 0, "segment_mean: negative capacity %d", cap);
  NSDP_REQUIRE(offsets && out && (values || cap == 0), "segment_mean: null pointer");      // (no rows: nothing is read)
  NSDP_REQUIRE(transform == 0 || transform == 1, "segment_mean: transform %d is neither 0 (identity) nor 1 (sqrt)", transform);
  hipStream_t st = nsdp::as_stream(stream);
  hipLaunchKernelGGL(segment_mean_kernel, dim3(B), dim3(kThreads), 0, st, values, offsets, cap, transform, out);
  return nsdp::launch_status("segment_mean_kernel");
}
