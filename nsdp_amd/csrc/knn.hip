// k-nearest-neighbour index search for gfx950 -- replaces the ATen sequence
// `square_distance(a, b).argsort()[:, :, :k]` of the reference
// (/root/reference/model/utils.py:39-55; call sites model/encoder/blocks.py:101-102, :287-288 and
// model/decoder/blocks.py:50-52), which materialises a [B,n,m,3] difference tensor, a [B,n,m] distance
// matrix and a full m-wide sort per row.
//
// MI355X design: one lane per query point; the source cloud streams through LDS in float4 tiles
// (coalesced global loads, broadcast ds_read_b128 per candidate); each lane keeps its k best
// (distance, index) pairs sorted in VGPRs (fully unrolled insertion, no scratch).  HBM traffic is the
// algorithmic minimum: (n+m)*12 bytes in, n*k*4 out.  Nothing of size n x m ever exists.
// Exactness: distance = ((dx*dx + dy*dy) + dz*dz), dx = query - source, one rounding per op
// (contraction off), bit-identical to the reference's torch.sum of squares; order = ascending
// (distance, index) (torch.argsort is unstable on CPU, so exact ties have no reference order).
#include <cfloat>
#include <climits>
#include <type_traits>

#include "common.h"
#include "plane_tile.h"
#include "prof.h"
#include "ragged.h"

#pragma clang fp contract(off)

namespace {

constexpr int kTile = 1024;  // source points per LDS tile (16 KiB)

// One lane's search: `tile` is the workgroup's LDS tile, `qp` the lane's query point (read when `active`), `source` the m
// points of the lane's shape; the k best go to io[0..k) / dout[0..k) (dout may be NULL).  Every lane of the workgroup must
// call it (barriers), with the same `source` and `m`.  The indices written are min(idx_base + index within `source`, idx_max):
// (0, INT_MAX) for a rectangular source, (the shape's first row, cap - 1) for a packed one.
template <int K>
__device__ __forceinline__ void knn_scan(float4 *tile, const float *__restrict__ qp, const float *__restrict__ source, int m,
                                         int k, bool active, int32_t *__restrict__ io, float *__restrict__ dout,
                                         int idx_base = 0, int idx_max = INT_MAX) {
  float qx = 0.f, qy = 0.f, qz = 0.f;
  if (active) {
    qx = qp[0]; qy = qp[1]; qz = qp[2];
  }
  float bd[K];
  int bi[K];
#pragma unroll
  for (int t = 0; t < K; ++t) {
    bd[t] = FLT_MAX;
    bi[t] = 0;
  }
  // FLT_MAX sentinel: a real distance equal to FLT_MAX cannot displace it, inf/NaN inputs are out of
  // contract (the reference's argsort order for NaN is unspecified as well).
  for (int base = 0; base < m; base += kTile) {
    const int cnt = min(kTile, m - base);
    __syncthreads();
    for (int t = threadIdx.x; t < cnt; t += 256) {
      const float *p = source + static_cast<size_t>(base + t) * 3;
      tile[t] = make_float4(p[0], p[1], p[2], 0.f);
    }
    __syncthreads();
    for (int t = 0; t < cnt; ++t) {
      const float4 s = tile[t];
      const float d = nsdp::sq_dist3(qx, qy, qz, s.x, s.y, s.z);
      if (d < bd[K - 1]) {  // wave-level branch: skipped when no lane improves
        const int j = base + t;
#pragma unroll
        for (int u = K - 1; u > 0; --u) {
          const bool shift = d < bd[u - 1];
          const bool here = !shift && d < bd[u];
          const float nd = shift ? bd[u - 1] : (here ? d : bd[u]);
          const int ni = shift ? bi[u - 1] : (here ? j : bi[u]);
          bd[u] = nd;
          bi[u] = ni;
        }
        if (d < bd[0]) {
          bd[0] = d;
          bi[0] = j;
        }
      }
    }
  }
  if (active) {
#pragma unroll
    for (int t = 0; t < K; ++t)
      if (t < k) io[t] = min(bi[t] + idx_base, idx_max);
    if (dout) {
#pragma unroll
      for (int t = 0; t < K; ++t)
        if (t < k) dout[t] = bd[t];
    }
  }
}

template <int K>
__global__ __launch_bounds__(256) void knn_kernel(const float *__restrict__ query_all,
                                                  const float *__restrict__ source_all, int n, int m,
                                                  int k, int32_t *__restrict__ idx_all,
                                                  float *__restrict__ dist_all) {
  __shared__ float4 tile[kTile];
  const int b = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const size_t row = static_cast<size_t>(b) * n + i;
  knn_scan<K>(tile, query_all + row * 3, source_all + static_cast<size_t>(b) * m * 3, m, k, i < n, idx_all + row * k,
              dist_all ? dist_all + row * k : nullptr);
}

// The same search over a packed query set (ragged.h): query [cap,3], offsets [B+1] on the device, source [B,m,3].  A
// workgroup's 256 queries belong to one shape -- its LDS tile holds that shape's source points -- and a shape's last
// workgroup is partial.  Surplus workgroups return as a whole (before any barrier); rows at or beyond offsets[B] are not
// written.
template <int K>
__global__ __launch_bounds__(256) void knn_ragged_kernel(const float *__restrict__ query, const int32_t *__restrict__ offsets,
                                                         const float *__restrict__ source_all, int B, int cap, int m, int k,
                                                         int32_t *__restrict__ idx_all, float *__restrict__ dist_all) {
  __shared__ float4 tile[kTile];
  int b, row0, end;
  if (!nsdp::ragged_tile<256>(offsets, B, cap, static_cast<int>(blockIdx.x), b, row0, end)) return;
  const int i = row0 + threadIdx.x;
  const bool active = i < end;
  const size_t row = static_cast<size_t>(active ? i : end - 1);         // (inactive lanes form no pointer past the buffers)
  knn_scan<K>(tile, query + row * 3, source_all + static_cast<size_t>(b) * m * 3, m, k, active, idx_all + row * k,
              dist_all ? dist_all + row * k : nullptr);
}

// Several lanes per query, the insertion DEFERRED.  With one lane per query the kernel is one wave per SIMD at the encoder's
// sizes (2048 queries x 32 shapes = 1024 waves) and the wave-level insertion branch fires in most iterations (any of 64 lanes
// improving runs the unrolled shift for all): 313 us per launch whatever the batch.  Here S lanes share a query, lane s scans
// one S-th of each LDS tile with its own sorted top-K, and the S lists are merged through LDS by (distance, index) -- the same
// total order, S times the waves, 1/S of the iterations per wave.  Inserting at once would still take that branch (~5 K VALU
// operations) whenever ANY of the 64 lanes improves its list -- for 16 neighbours out of 512 candidates per lane ~95 % of all
// iterations, although a single lane inserts only ~70 times.  So a lane that sees a candidate below its (possibly stale, hence
// never too small) threshold only appends (distance, index) to a private FIFO of kQueue entries in LDS; the lists are updated
// when some lane's FIFO is nearly full and once at the end, by insertion rounds in which most lanes take part.  A lane still
// meets its candidates in increasing index order and the insertion is knn_scan's strict `<` chain, so the result -- ties
// included -- is the one of inserting at once, bit for bit; per candidate the loop is a distance, a compare and a predicated
// LDS append.  Measured (k = 16, four lanes per query; inserting at once -> deferred): 500 x 2048 x 32 shapes 200 -> 111 us,
// 2048 x 8192 x 32 1227 -> 691 us, 4096 x 16384 x 16 1979 -> 1251 us; a 16-entry FIFO with the candidates taken four at a time
// (independent LDS reads and distances) against 8 entries one at a time: 111 against 125 us; eight lanes per query instead of
// four: slower (124 / 1096 / 2029 us, more list work).  With the tile as three planes + sentinels and the distances on packed
// fp32 operations (plane_tile.h): 92 / 458 / 767 us.
// One workgroup's search as a function of what the two kernels below differ in: `qp` the query point of this lane's query
// (read when `active`; the S lanes of a query pass the same), `source` the m points every lane of the workgroup searches, `io` /
// `dout` (or NULL) the query's k output slots, and the index written = min(idx_base + index within `source`, idx_max).
template <int K, int S, int kQueue>
__device__ __forceinline__ void knn_split_queue_scan(const float *__restrict__ qp, bool active,
                                                     const float *__restrict__ source, int m, int k,
                                                     int32_t *__restrict__ io, float *__restrict__ dout, int idx_base,
                                                     int idx_max) {
  __shared__ nsdp::PlaneTile<kTile, 16> tile;      // 16 sentinel entries: no range checks in the scan
  __shared__ float md[256 * K];      // the FIFOs during the scan ([slot][thread]: conflict-free), the S lists afterwards
  __shared__ int mi[256 * K];
  static_assert(K >= kQueue, "the FIFOs live in the merge buffers");
  const int sub = threadIdx.x % S;
  float qx = 0.f, qy = 0.f, qz = 0.f;
  if (active) {
    qx = qp[0]; qy = qp[1]; qz = qp[2];
  }
  float bd[K];
  int bi[K];
#pragma unroll
  for (int t = 0; t < K; ++t) {
    bd[t] = FLT_MAX;
    bi[t] = 0x7fffffff;
  }
  int fill = 0;                      // entries in this lane's FIFO
  auto drain = [&]() __attribute__((always_inline)) {
    for (int sl = 0; sl < kQueue; ++sl) {
      const bool has = sl < fill;
      if (__builtin_amdgcn_ballot_w64(has) == 0) break;
      const float d = has ? md[sl * 256 + threadIdx.x] : FLT_MAX;
      const int j = mi[sl * 256 + threadIdx.x];
      if (d < bd[K - 1]) {
#pragma unroll
        for (int u = K - 1; u > 0; --u) {
          const bool shift = d < bd[u - 1];
          const bool here = !shift && d < bd[u];
          const float nd = shift ? bd[u - 1] : (here ? d : bd[u]);
          const int ni = shift ? bi[u - 1] : (here ? j : bi[u]);
          bd[u] = nd;
          bi[u] = ni;
        }
        if (d < bd[0]) {
          bd[0] = d;
          bi[0] = j;
        }
      }
    }
    fill = 0;
  };
  for (int base = 0; base < m; base += kTile) {
    const int cnt = min(kTile, m - base);
    __syncthreads();
    tile.load<256>(source + static_cast<size_t>(base) * 3, cnt);
    __syncthreads();
    // lane `sub` scans tile entries [sub * per, (sub + 1) * per), per a multiple of four (the same trip count in every
    // lane: the ballots see whole waves); S * per <= cnt + 4 S - 1: the sentinels cover what lies behind the tile.
    const int per = (((cnt + S - 1) / S) + 3) & ~3;
    const int t0 = sub * per;
    static_assert(S <= 4, "16 sentinel entries");
    for (int tt = 0; tt < per; tt += 4) {
      const int t = t0 + tt;
      nsdp::f32x4 X, Y, Z;
      nsdp::f32x2 d01, d23;
      tile.read4(t, X, Y, Z);
      nsdp::dist4(X, Y, Z, qx, qy, qz, d01, d23);
      const float d[4] = {d01[0], d01[1], d23[0], d23[1]};
      const float thr = bd[K - 1];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (d[u] < thr) {
          md[fill * 256 + threadIdx.x] = d[u];
          mi[fill * 256 + threadIdx.x] = base + t + u;
          ++fill;
        }
      }
      if (__builtin_amdgcn_ballot_w64(fill > kQueue - 4) != 0) drain();
    }
  }
  drain();
  __syncthreads();                   // every wave is done with its FIFOs: the buffers become the merge lists
#pragma unroll
  for (int t = 0; t < K; ++t) {
    md[threadIdx.x * K + t] = bd[t];
    mi[threadIdx.x * K + t] = bi[t];
  }
  __syncthreads();
  if (active && sub == 0) {
    int head[S];
#pragma unroll
    for (int u = 0; u < S; ++u) head[u] = 0;
    for (int t = 0; t < k; ++t) {
      float best_d = FLT_MAX;
      int best_i = 0x7fffffff, best_u = 0;
#pragma unroll
      for (int u = 0; u < S; ++u) {
        const int h = head[u];
        const float dd = h < K ? md[(threadIdx.x + u) * K + h] : FLT_MAX;
        const int ii = h < K ? mi[(threadIdx.x + u) * K + h] : 0x7fffffff;
        if (dd < best_d || (dd == best_d && ii < best_i)) {
          best_d = dd; best_i = ii; best_u = u;
        }
      }
#pragma unroll
      for (int u = 0; u < S; ++u) head[u] += (u == best_u) ? 1 : 0;
      // (an empty slot -- fewer than k source points, which only a packed source with corrupt offsets can have -- names the
      // source's first point)
      io[t] = min((best_i == 0x7fffffff ? 0 : best_i) + idx_base, idx_max);
      if (dout) dout[t] = best_d;
    }
  }
}

template <int K, int S, int kQueue>
__global__ __launch_bounds__(256) void knn_split_queue_kernel(const float *__restrict__ query_all,
                                                              const float *__restrict__ source_all, int n, int m, int k,
                                                              int32_t *__restrict__ idx_all, float *__restrict__ dist_all) {
  constexpr int kQ = 256 / S;
  const int b = blockIdx.y;
  const int i = blockIdx.x * kQ + threadIdx.x / S;
  const size_t row = static_cast<size_t>(b) * n + i;
  knn_split_queue_scan<K, S, kQueue>(query_all + row * 3, i < n, source_all + static_cast<size_t>(b) * m * 3, m, k,
                                     idx_all + row * k, dist_all ? dist_all + row * k : nullptr, 0, INT_MAX);
}

// Both searches against a PACKED source set (ragged.h): source [cap,3] + offsets [B+1] on the device, shape b's queries search
// rows offsets[b] .. offsets[b+1] (clamped as ragged.h clamps them, and to n_max rows) and get packed-row indices.  The queries
// are rectangular [B,n,3] (query_offsets NULL: the shape is the grid's y index) or packed themselves ([qcap,3] +
// query_offsets: kQ queries of a workgroup belong to one shape, surplus workgroups return as a whole before any barrier, rows
// at or beyond query_offsets[B] are not written).  `row` never leaves the query buffer: inactive lanes take the last row of
// their shape.
template <int kQ>
__device__ __forceinline__ bool knn_rs_tile(const int32_t *__restrict__ query_offsets, const int32_t *__restrict__ offsets, int B,
                                            int n, int qcap, int cap, int n_max, int ql, size_t &row, bool &active, int &lo,
                                            int &m) {
  int b, row0, end;
  if (query_offsets) {
    if (!nsdp::ragged_tile<kQ>(query_offsets, B, qcap, static_cast<int>(blockIdx.x), b, row0, end)) return false;
    active = row0 + ql < end;
    row = static_cast<size_t>(active ? row0 + ql : end - 1);
  } else {
    b = blockIdx.y;
    const int i = blockIdx.x * kQ + ql;
    active = i < n;
    row = static_cast<size_t>(b) * n + (active ? i : n - 1);
  }
  int hi;
  nsdp::ragged_range(offsets, b, cap, lo, hi);
  m = min(hi - lo, n_max);
  return true;
}

template <int K, int S, int kQueue>
__global__ __launch_bounds__(256) void knn_rs_split_queue_kernel(const float *__restrict__ query,
                                                                 const int32_t *__restrict__ query_offsets,
                                                                 const float *__restrict__ source,
                                                                 const int32_t *__restrict__ offsets, int B, int n, int qcap,
                                                                 int cap, int n_max, int k, int32_t *__restrict__ idx_all,
                                                                 float *__restrict__ dist_all) {
  size_t row;
  bool active;
  int lo, m;
  if (!knn_rs_tile<256 / S>(query_offsets, offsets, B, n, qcap, cap, n_max, threadIdx.x / S, row, active, lo, m)) return;
  knn_split_queue_scan<K, S, kQueue>(query + row * 3, active, source + static_cast<size_t>(lo) * 3, m, k, idx_all + row * k,
                                     dist_all ? dist_all + row * k : nullptr, lo, cap - 1);
}

template <int K>
__global__ __launch_bounds__(256) void knn_rs_kernel(const float *__restrict__ query, const int32_t *__restrict__ query_offsets,
                                                     const float *__restrict__ source, const int32_t *__restrict__ offsets,
                                                     int B, int n, int qcap, int cap, int n_max, int k,
                                                     int32_t *__restrict__ idx_all, float *__restrict__ dist_all) {
  __shared__ float4 tile[kTile];
  size_t row;
  bool active;
  int lo, m;
  if (!knn_rs_tile<256>(query_offsets, offsets, B, n, qcap, cap, n_max, threadIdx.x, row, active, lo, m)) return;
  knn_scan<K>(tile, query + row * 3, source + static_cast<size_t>(lo) * 3, m, k, active, idx_all + row * k,
              dist_all ? dist_all + row * k : nullptr, lo, cap - 1);
}

template <int K>
int launch(const float *q, const float *s, int B, int n, int m, int k, int32_t *idx, float *d2,
           hipStream_t st) {
  // enough queries to fill the chip with one lane each (the decoder: 8192 queries per shape), or a cloud too small to
  // split: the one-lane-per-query form
  const long long waves = (static_cast<long long>(n) + 255) / 256 * 4 * B;
  if constexpr (K <= 16) {
    if (m >= 256 && waves < 8LL * nsdp::num_cus()) {
      dim3 grid(nsdp::ceil_div(n, 64), B);
      constexpr int kQueue = K >= 16 ? 16 : 8;
      NSDP_TRACE("knn_split_queue<%d,4,%d>", K, kQueue);
      hipLaunchKernelGGL((knn_split_queue_kernel<K, 4, kQueue>), grid, dim3(256), 0, st, q, s, n, m, k, idx, d2);
      return nsdp::launch_status("knn_split_queue_kernel");
    }
  }
  dim3 grid(nsdp::ceil_div(n, 256), B);
  NSDP_TRACE("knn<%d>", K);
  hipLaunchKernelGGL((knn_kernel<K>), grid, dim3(256), 0, st, q, s, n, m, k, idx, d2);
  return nsdp::launch_status("knn_kernel");
}

template <int K>
int launch_ragged(const float *q, const int32_t *offsets, const float *s, int B, int cap, int m, int k, int32_t *idx,
                  float *d2, hipStream_t st) {
  NSDP_TRACE("knn_ragged<%d>", K);
  const int tiles = static_cast<int>(nsdp::ragged_max_tiles(cap, B, 256));
  hipLaunchKernelGGL((knn_ragged_kernel<K>), dim3(tiles), dim3(256), 0, st, q, offsets, s, B, cap, m, k, idx, d2);
  return nsdp::launch_status("knn_ragged_kernel");
}

// the form is chosen as `launch` chooses it, from what the host knows: the number of query rows (B * n, or the capacity of a
// packed query set) and the bound of a shape's source rows
template <int K>
int launch_rs(const float *q, const int32_t *qoff, const float *s, const int32_t *offsets, int B, int n, int qcap, int cap,
              int n_max, int k, int32_t *idx, float *d2, hipStream_t st) {
  const long long rows = qoff ? qcap : static_cast<long long>(B) * n;
  if constexpr (K <= 16) {
    if (n_max >= 256 && (rows + 255) / 256 * 4 < 8LL * nsdp::num_cus()) {
      constexpr int kQueue = K >= 16 ? 16 : 8;
      NSDP_TRACE("knn_rs_split_queue<%d,4,%d>", K, kQueue);
      const dim3 grid = qoff ? dim3(static_cast<unsigned>(nsdp::ragged_max_tiles(qcap, B, 64))) : dim3(nsdp::ceil_div(n, 64), B);
      hipLaunchKernelGGL((knn_rs_split_queue_kernel<K, 4, kQueue>), grid, dim3(256), 0, st, q, qoff, s, offsets, B, n, qcap, cap,
                         n_max, k, idx, d2);
      return nsdp::launch_status("knn_rs_split_queue_kernel");
    }
  }
  NSDP_TRACE("knn_rs<%d>", K);
  const dim3 grid = qoff ? dim3(static_cast<unsigned>(nsdp::ragged_max_tiles(qcap, B, 256))) : dim3(nsdp::ceil_div(n, 256), B);
  hipLaunchKernelGGL((knn_rs_kernel<K>), grid, dim3(256), 0, st, q, qoff, s, offsets, B, n, qcap, cap, n_max, k, idx, d2);
  return nsdp::launch_status("knn_rs_kernel");
}

// the kernels keep K list entries in registers: f(std::integral_constant<int, K>) for the smallest instantiated K >= k (the
// entries have checked k <= 64)
template <class F>
int with_list_size(int k, F &&f) {
  if (k <= 8) return f(std::integral_constant<int, 8>{});
  if (k <= 16) return f(std::integral_constant<int, 16>{});
  if (k <= 32) return f(std::integral_constant<int, 32>{});
  return f(std::integral_constant<int, 64>{});
}

}  // namespace

extern "C" int nsdp_knn(const float *query, const float *source, int B, int n, int m, int k,
                        int32_t *idx_out, float *dist2_out, void *stream) {
  if (B <= 0 || n <= 0 || k <= 0) return 0;
  NSDP_REQUIRE(query && source && idx_out, "knn: null pointer");
  NSDP_REQUIRE(k <= m, "knn: k=%d exceeds the number of source points m=%d", k, m);
  NSDP_REQUIRE(k <= 64, "knn: k=%d > 64 is not supported", k);
  NSDP_REQUIRE(B <= 65535, "knn: batch %d too large for one launch", B);
  hipStream_t st = nsdp::as_stream(stream);
  nsdp::prof::Scope scope(nsdp::prof::kKnn, st, 0.0,
                          static_cast<double>(B) * (12.0 * (n + m) + 4.0 * n * k * (dist2_out ? 2 : 1)));
  return with_list_size(k, [&](auto K) { return launch<K>(query, source, B, n, m, k, idx_out, dist2_out, st); });
}

extern "C" int nsdp_knn_ragged(const float *query, const int32_t *offsets, const float *source, int B, int cap, int m,
                               int k, int32_t *idx_out, float *dist2_out, void *stream) {
  if (static_cast<long long>(B) * cap <= 0 || k <= 0) return 0;
  NSDP_REQUIRE(query && offsets && source && idx_out, "knn_ragged: null pointer");
  NSDP_REQUIRE(k <= m, "knn_ragged: k=%d exceeds the number of source points m=%d", k, m);
  NSDP_REQUIRE(k <= 64, "knn_ragged: k=%d > 64 is not supported", k);
  NSDP_REQUIRE(B <= 65535, "knn_ragged: batch %d too large for one launch", B);
  hipStream_t st = nsdp::as_stream(stream);
  // the number of real rows is known to the device alone: bytes accounted with cap, an upper bound
  nsdp::prof::Scope scope(nsdp::prof::kKnn, st, 0.0,
                          12.0 * (static_cast<double>(cap) + static_cast<double>(B) * m) +
                              4.0 * cap * k * (dist2_out ? 2 : 1));
  return with_list_size(k, [&](auto K) { return launch_ragged<K>(query, offsets, source, B, cap, m, k, idx_out, dist2_out, st); });
}

extern "C" int nsdp_knn_ragged_source(const float *query, const int32_t *query_offsets, const float *source,
                                      const int32_t *offsets, int B, int n, int qcap, int cap, int n_max, int k, int32_t *idx_out,
                                      float *dist2_out, void *stream) {
  const long long rows = query_offsets ? static_cast<long long>(qcap) : static_cast<long long>(B) * n;
  if (B <= 0 || rows <= 0 || k <= 0) return 0;
  NSDP_REQUIRE(query && source && offsets && idx_out, "knn_ragged_source: null pointer");
  NSDP_REQUIRE(cap > 0 && n_max > 0, "knn_ragged_source: cap and n_max must be positive (got %d, %d)", cap, n_max);
  NSDP_REQUIRE(k <= n_max, "knn_ragged_source: k=%d exceeds the bound of a shape's source points n_max=%d", k, n_max);
  NSDP_REQUIRE(k <= 64, "knn_ragged_source: k=%d > 64 is not supported", k);
  NSDP_REQUIRE(B <= 65535, "knn_ragged_source: batch %d too large for one launch", B);
  NSDP_REQUIRE(rows * k < (1LL << 31), "knn_ragged_source: %lld query rows x k=%d too large", rows, k);
  hipStream_t st = nsdp::as_stream(stream);
  nsdp::prof::Scope scope(nsdp::prof::kKnn, st, 0.0,
                          12.0 * (static_cast<double>(rows) + cap) + 4.0 * rows * k * (dist2_out ? 2 : 1));
  return with_list_size(k, [&](auto K) {
    return launch_rs<K>(query, query_offsets, source, offsets, B, n, qcap, cap, n_max, k, idx_out, dist2_out, st);
  });
}
