// Inverse neighbour lists of large index sets, built by the whole chip (include/nsdp_scatter.h).
//
// nsdp_knn_invert (segment.hip) builds the lists of a shape with ONE workgroup and keeps its counters in LDS: it refuses more
// than 32 768 sources, orders its lists from LDS only up to ~2200 points at k = 16, and leaves one compute unit with the whole
// build at B = 1.  Here the same lists -- entries[b][offsets[b][s] .. offsets[b][s+1]) = the ascending e with idx[b][e] == s --
// are a counting sort in global memory: integer work only, every phase a launch of its own on the caller's stream, no workgroup
// ever waits for another.
//
//   zero     the counters cnt[B][N] and the long-list counters nlong[B] -- a kernel, not a memset: a captured call then
//            consists of kernel nodes alone, ordered like any other chain of launches on the stream;
//   count    one lane per four entries (one 16-byte load where the index tensor allows it): cnt[b][s] += 1, an integer atomic
//            without a return value.  Integer sums do not depend on the order of arrival;
//   sums     one workgroup per tile of kScanTile sources: the tile's total of counts -> tsum[b][t];
//   offsets  one workgroup per tile again: the tiles in front of it are summed from tsum (at most 1024 values: N <= 2^20), the
//            tile itself is scanned in the workgroup.  offsets[b][s] is written, cnt[b][s] becomes the fill cursor (the same
//            value), and a source whose list is longer than kSortMax draws a slot of the shape's worklist;
//   fill     one lane per four entries: tmp[b][cursor[b][s]++] = e for the entries of lists up to kSortMax -- the order inside a
//            list is whatever order the atomics retire in;
//   order    one lane per slot i of tmp: the slot's entry v names its list (s = idx[v]); v's place is the number of smaller
//            entries of that list, read through the caches (adjacent lanes sit in the same list and read the same lines), and
//            v goes straight to entries[lo + place];
//   long     one workgroup per list longer than kSortMax.  It does not sort: it walks the shape's idx from e = 0 to E and writes
//            every e with idx[e] == s, in that order, behind a running count (a stream compaction, one block scan per 4096
//            entries).  tmp holds nothing for these lists.
//
// Uniqueness.  The entries of a list are distinct integers, so "ascending" fixes every list completely, and offsets are the
// exclusive scan of integer counts: the result is the stable sort of e by idx[b][e], whatever the atomics did.  `order` ranks
// by counting (the entries are distinct: the ranks are a permutation of the list's slots); `long` emits in ascending e by
// construction.  Every slot of entries is written exactly once by exactly one of the two.
//
// Cost.  count / fill: E atomics, at most kSortMax of the fill's on one address (count: a list's length -- the all-duplicate
// cloud puts n atomics on each of k addresses, which serialise in one L2 channel).  order: sum of L^2 over the lists up to
// kSortMax, <= kSortMax * E reads that hit the caches.  long: E index reads per long list, at most E / (kSortMax + 1) lists per
// shape, each an independent workgroup: <= E^2 / 1025 reads per shape, spread over the chip.  Finite for every input; fast for
// what a k-NN index set looks like (lists of E / N entries on average).
//
// Invalid indices.  Every index read from idx is clamped into [0, N) before it is used, the same way in every phase, so the
// counts, the cursors and the lists agree with each other whatever idx holds; values read back from the workspace (a slot's
// entry in uninitialised parts of tmp, a worklist slot) are clamped before they form an address, and every store into entries
// or tmp is bounded by its list, whose bounds are themselves cut to [0, E] after they are read: whatever the workspace and
// offsets hold when a kernel reads them, it forms no address outside offsets, entries and the workspace.
#include "common.h"
#include "prof.h"

#include "../../include/nsdp_scatter.h"

namespace {

constexpr int kMaxSources = 1 << 20;
constexpr int kMaxEntries = 1 << 25;
constexpr int kSortMax = 1024;          // longest list ordered by rank counting (segment.hip's bound); longer ones by compaction
constexpr int kScanTile = 1024;         // sources per workgroup of the scan (hip_attention.INVERT_WIDE_TILE mirrors it)
constexpr int kThreads = 256;
constexpr int kLongThreads = 1024;
constexpr int kLongTile = kLongThreads * 4;
static_assert(kScanTile == kThreads * 4, "the scan kernels hold four sources per lane");
static_assert(kMaxSources / kScanTile <= kThreads * 4, "offsets kernel: the tile sums of a shape are four per lane at most");

struct Layout {
  size_t cnt, nlong, tsum, work, tmp, total, zero_bytes;
  int tiles, max_long;
};

inline size_t align16(size_t v) { return (v + 15) & ~static_cast<size_t>(15); }

Layout layout(int B, int E, int N) {
  Layout L;
  L.tiles = (N + kScanTile - 1) / kScanTile;
  L.max_long = E / (kSortMax + 1);
  const size_t b = static_cast<size_t>(B);
  L.cnt = 0;
  L.nlong = L.cnt + b * N * sizeof(int32_t);                  // (directly behind the counters: zeroed together)
  L.zero_bytes = align16(L.nlong + b * sizeof(int32_t));
  L.tsum = L.zero_bytes;
  L.work = align16(L.tsum + b * L.tiles * sizeof(int32_t));
  L.tmp = align16(L.work + b * L.max_long * sizeof(int32_t));
  L.total = align16(L.tmp + b * E * sizeof(int32_t));
  return L;
}

__device__ __forceinline__ int clamp_source(int s, int N) { return min(max(s, 0), N - 1); }

// the bounds of a list as read back from offsets, cut to 0 <= lo <= hi <= E
__device__ __forceinline__ void list_bounds(const int32_t *__restrict__ offsets, int s, int E, int &lo, int &hi) {
  lo = min(max(offsets[s], 0), E);
  hi = min(max(offsets[s + 1], lo), E);
}

__global__ __launch_bounds__(kThreads) void invert_zero_kernel(int32_t *__restrict__ p, long long n) {
  const long long i0 = (static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x) * 4;
#pragma unroll
  for (int u = 0; u < 4; ++u)
    if (i0 + u < n) p[i0 + u] = 0;
}

// four consecutive entries e0 .. e0 + 3 of one shape (e0 a multiple of 4, e0 < E); `valid` = how many of them lie below E (1 .. 4)
template <bool VEC>
__device__ __forceinline__ int4 load_entries(const int32_t *__restrict__ idx, int e0, int E, int &valid) {
  valid = min(4, E - e0);
  if (VEC) return *reinterpret_cast<const int4 *>(idx + e0);       // (E % 4 == 0 and a 16-byte aligned tensor: all four exist)
  int4 r = make_int4(0, 0, 0, 0);
  r.x = idx[e0];
  if (valid > 1) r.y = idx[e0 + 1];
  if (valid > 2) r.z = idx[e0 + 2];
  if (valid > 3) r.w = idx[e0 + 3];
  return r;
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void invert_count_kernel(const int32_t *__restrict__ idx_all, int E, int N,
                                                                int32_t *__restrict__ cnt_all) {
  const int b = blockIdx.y;
  const long long e0l = (static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x) * 4;
  if (e0l >= E) return;
  const int e0 = static_cast<int>(e0l);
  int valid;
  const int4 v = load_entries<VEC>(idx_all + static_cast<long long>(b) * E, e0, E, valid);
  int32_t *cnt = cnt_all + static_cast<long long>(b) * N;
  atomicAdd(&cnt[clamp_source(v.x, N)], 1);
  if (valid > 1) atomicAdd(&cnt[clamp_source(v.y, N)], 1);
  if (valid > 2) atomicAdd(&cnt[clamp_source(v.z, N)], 1);
  if (valid > 3) atomicAdd(&cnt[clamp_source(v.w, N)], 1);
}

// sum over the workgroup of one int per lane; every lane gets the total.  `red` holds one int per wave.
template <int THREADS>
__device__ __forceinline__ int block_sum(int v, int *red) {
#pragma unroll
  for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) red[wave] = v;
  __syncthreads();
  int total = 0;
#pragma unroll
  for (int w = 0; w < THREADS / 64; ++w) total += red[w];
  return total;
}

// exclusive prefix over the workgroup of one int per lane (in lane order); `total` gets the workgroup's sum
template <int THREADS>
__device__ __forceinline__ int block_exclusive(int v, int *red, int &total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int up = __shfl_up(inc, off);
    if (lane >= off) inc += up;
  }
  if (lane == 63) red[wave] = inc;
  __syncthreads();
  int before = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < THREADS / 64; ++w) {
    const int t = red[w];
    before += w < wave ? t : 0;
    total += t;
  }
  return before + inc - v;
}

__global__ __launch_bounds__(kThreads) void invert_tile_sums_kernel(const int32_t *__restrict__ cnt_all, int N, int tiles,
                                                                    int32_t *__restrict__ tsum_all) {
  __shared__ int red[kThreads / 64];
  const int b = blockIdx.y, t = blockIdx.x;
  const int32_t *cnt = cnt_all + static_cast<long long>(b) * N;
  const int s0 = t * kScanTile + threadIdx.x * 4;
  int local = 0;
#pragma unroll
  for (int u = 0; u < 4; ++u) local += s0 + u < N ? cnt[s0 + u] : 0;
  const int total = block_sum<kThreads>(local, red);
  if (threadIdx.x == 0) tsum_all[static_cast<long long>(b) * tiles + t] = total;
}

__global__ __launch_bounds__(kThreads) void invert_offsets_kernel(int32_t *__restrict__ cnt_all, const int32_t *__restrict__ tsum_all,
                                                                  int E, int N, int tiles, int max_long,
                                                                  int32_t *__restrict__ offsets_all, int32_t *__restrict__ nlong_all,
                                                                  int32_t *__restrict__ work_all) {
  __shared__ int red[kThreads / 64];
  __shared__ int red2[kThreads / 64];
  const int b = blockIdx.y, t = blockIdx.x;
  int32_t *cnt = cnt_all + static_cast<long long>(b) * N;
  int32_t *offsets = offsets_all + static_cast<long long>(b) * (N + 1);
  const int32_t *tsum = tsum_all + static_cast<long long>(b) * tiles;
  // the tiles in front of this one
  int ahead = 0;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int j = threadIdx.x * 4 + u;
    ahead += j < t ? tsum[j] : 0;
  }
  const int base = block_sum<kThreads>(ahead, red);
  const int s0 = t * kScanTile + threadIdx.x * 4;
  int c[4], local = 0;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    c[u] = s0 + u < N ? cnt[s0 + u] : 0;
    local += c[u];
  }
  int total;
  int run = base + block_exclusive<kThreads>(local, red2, total);
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int s = s0 + u;
    if (s < N) {
      offsets[s] = min(run, E);      // (= run: the counts of a shape sum to E)
      cnt[s] = min(run, E);          // the fill cursor
      if (c[u] > kSortMax) {
        const int slot = atomicAdd(&nlong_all[b], 1);      // (at most E / (kSortMax + 1) such lists: the worklist's size)
        if (slot < max_long) work_all[static_cast<long long>(b) * max_long + slot] = s;
      }
      run += c[u];
    }
  }
  if (t == 0 && threadIdx.x == 0) offsets[N] = E;
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void invert_fill_kernel(const int32_t *__restrict__ idx_all, int E, int N,
                                                               const int32_t *__restrict__ offsets_all,
                                                               int32_t *__restrict__ cursor_all, int32_t *__restrict__ tmp_all) {
  const int b = blockIdx.y;
  const long long e0l = (static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x) * 4;
  if (e0l >= E) return;
  const int e0 = static_cast<int>(e0l);
  int valid;
  const int4 v = load_entries<VEC>(idx_all + static_cast<long long>(b) * E, e0, E, valid);
  const int32_t *offsets = offsets_all + static_cast<long long>(b) * (N + 1);
  int32_t *cursor = cursor_all + static_cast<long long>(b) * N;
  int32_t *tmp = tmp_all + static_cast<long long>(b) * E;
  const int raw[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    if (u < valid) {
      const int s = clamp_source(raw[u], N);
      int lo, hi;
      list_bounds(offsets, s, E, lo, hi);
      if (hi - lo <= kSortMax) {      // (a longer list is written from idx itself, by invert_long_kernel)
        const int pos = atomicAdd(&cursor[s], 1);
        if (pos >= lo && pos < hi) tmp[pos] = e0 + u;
      }
    }
  }
}

__global__ __launch_bounds__(kThreads) void invert_order_kernel(const int32_t *__restrict__ idx_all, int E, int N,
                                                                const int32_t *__restrict__ offsets_all,
                                                                const int32_t *__restrict__ tmp_all,
                                                                int32_t *__restrict__ entries_all) {
  const int b = blockIdx.y;
  const long long il = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x;
  if (il >= E) return;
  const int i = static_cast<int>(il);
  const int32_t *idx = idx_all + static_cast<long long>(b) * E;
  const int32_t *offsets = offsets_all + static_cast<long long>(b) * (N + 1);
  const int32_t *tmp = tmp_all + static_cast<long long>(b) * E;
  // (a slot of a long list was never written: whatever it holds is clamped, and the range test below drops it -- slot i lies in
  // exactly one list, a long one, so no short list's range can contain it)
  const int v = tmp[i];
  const int s = clamp_source(idx[min(max(v, 0), E - 1)], N);
  int lo, hi;
  list_bounds(offsets, s, E, lo, hi);
  if (i < lo || i >= hi || hi - lo > kSortMax) return;
  int rank = 0;
  for (int j = lo; j < hi; ++j) rank += tmp[j] < v ? 1 : 0;
  entries_all[static_cast<long long>(b) * E + lo + rank] = v;
}

template <bool VEC>
__global__ __launch_bounds__(kLongThreads) void invert_long_kernel(const int32_t *__restrict__ idx_all, int E, int N, int max_long,
                                                                   const int32_t *__restrict__ offsets_all,
                                                                   const int32_t *__restrict__ nlong_all,
                                                                   const int32_t *__restrict__ work_all,
                                                                   int32_t *__restrict__ entries_all) {
  __shared__ int red[2][kLongThreads / 64];
  const int b = blockIdx.y;
  if (static_cast<int>(blockIdx.x) >= min(nlong_all[b], max_long)) return;      // (uniform over the workgroup)
  const int s = clamp_source(work_all[static_cast<long long>(b) * max_long + blockIdx.x], N);
  const int32_t *idx = idx_all + static_cast<long long>(b) * E;
  const int32_t *offsets = offsets_all + static_cast<long long>(b) * (N + 1);
  int32_t *entries = entries_all + static_cast<long long>(b) * E;
  int lo, hi;
  list_bounds(offsets, s, E, lo, hi);
  int run = lo;
  int buf = 0;
  for (long long base = 0; base < E; base += kLongTile, buf ^= 1) {      // (the bound is uniform: every lane meets every barrier)
    const long long e0l = base + threadIdx.x * 4;
    int valid = 0;
    int4 v = make_int4(0, 0, 0, 0);
    if (e0l < E) v = load_entries<VEC>(idx, static_cast<int>(e0l), E, valid);
    const int raw[4] = {v.x, v.y, v.z, v.w};
    bool hit[4];
    int mine = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      hit[u] = u < valid && clamp_source(raw[u], N) == s;
      mine += hit[u] ? 1 : 0;
    }
    // (one barrier per tile: the two halves of `red` alternate, and a wave can only be one barrier ahead of another)
    int total;
    int pos = run + block_exclusive<kLongThreads>(mine, red[buf], total);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (hit[u]) {
        if (pos >= lo && pos < hi) entries[pos] = static_cast<int>(e0l) + u;
        ++pos;
      }
    }
    run += total;
  }
}

bool refused(int B, int E, int N) {
  return B < 1 || B > 65535 || N < 1 || N > kMaxSources || E < 1 || E > kMaxEntries;
}

}  // namespace

extern "C" size_t nsdp_knn_invert_wide_workspace_bytes(int B, int E, int N) {
  if (refused(B, E, N)) return 0;
  return layout(B, E, N).total;
}

extern "C" int nsdp_knn_invert_wide(const int32_t *idx, int B, int E, int N, void *workspace, int32_t *offsets, int32_t *entries,
                                    void *stream) {
  NSDP_REQUIRE(B >= 1 && B <= 65535, "knn_invert_wide: batch %d must be in [1, 65535]", B);
  NSDP_REQUIRE(N >= 1 && N <= kMaxSources, "knn_invert_wide: N=%d sources per shape must be in [1, %d]", N, kMaxSources);
  NSDP_REQUIRE(E >= 1 && E <= kMaxEntries, "knn_invert_wide: E=%d entries per shape must be in [1, %d]", E, kMaxEntries);
  NSDP_REQUIRE(idx && offsets && entries, "knn_invert_wide: null pointer");
  NSDP_REQUIRE(workspace, "knn_invert_wide: null workspace pointer");
  NSDP_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 3) == 0, "knn_invert_wide: the workspace must be 4-byte aligned");
  hipStream_t st = nsdp::as_stream(stream);
  const Layout L = layout(B, E, N);
  char *ws = static_cast<char *>(workspace);
  int32_t *cnt = reinterpret_cast<int32_t *>(ws + L.cnt), *nlong = reinterpret_cast<int32_t *>(ws + L.nlong);
  int32_t *tsum = reinterpret_cast<int32_t *>(ws + L.tsum), *work = reinterpret_cast<int32_t *>(ws + L.work);
  int32_t *tmp = reinterpret_cast<int32_t *>(ws + L.tmp);
  nsdp::prof::Scope scope(nsdp::prof::kKnn, st, 0.0, static_cast<double>(B) * (20.0 * E + 16.0 * N));
  const bool vec = E % 4 == 0 && (reinterpret_cast<uintptr_t>(idx) & 15) == 0;
  const dim3 by_entries(nsdp::ceil_div(nsdp::ceil_div(E, 4), kThreads), B), by_tiles(L.tiles, B);
  int rc;
  const long long zero_ints = static_cast<long long>(L.zero_bytes / sizeof(int32_t));
  hipLaunchKernelGGL(invert_zero_kernel, dim3(nsdp::ceil_div(zero_ints, 4 * kThreads)), dim3(kThreads), 0, st,
                     reinterpret_cast<int32_t *>(ws), zero_ints);
  if ((rc = nsdp::launch_status("invert_zero_kernel"))) return rc;
  if (vec) hipLaunchKernelGGL(invert_count_kernel<true>, by_entries, dim3(kThreads), 0, st, idx, E, N, cnt);
  else hipLaunchKernelGGL(invert_count_kernel<false>, by_entries, dim3(kThreads), 0, st, idx, E, N, cnt);
  if ((rc = nsdp::launch_status("invert_count_kernel"))) return rc;
  hipLaunchKernelGGL(invert_tile_sums_kernel, by_tiles, dim3(kThreads), 0, st, cnt, N, L.tiles, tsum);
  if ((rc = nsdp::launch_status("invert_tile_sums_kernel"))) return rc;
  hipLaunchKernelGGL(invert_offsets_kernel, by_tiles, dim3(kThreads), 0, st, cnt, tsum, E, N, L.tiles, L.max_long, offsets, nlong,
                     work);
  if ((rc = nsdp::launch_status("invert_offsets_kernel"))) return rc;
  if (vec) hipLaunchKernelGGL(invert_fill_kernel<true>, by_entries, dim3(kThreads), 0, st, idx, E, N, offsets, cnt, tmp);
  else hipLaunchKernelGGL(invert_fill_kernel<false>, by_entries, dim3(kThreads), 0, st, idx, E, N, offsets, cnt, tmp);
  if ((rc = nsdp::launch_status("invert_fill_kernel"))) return rc;
  hipLaunchKernelGGL(invert_order_kernel, dim3(nsdp::ceil_div(E, kThreads), B), dim3(kThreads), 0, st, idx, E, N, offsets, tmp,
                     entries);
  if ((rc = nsdp::launch_status("invert_order_kernel"))) return rc;
  if (L.max_long > 0) {      // (E <= kSortMax: no list can be long)
    const dim3 by_lists(L.max_long, B);
    if (vec) hipLaunchKernelGGL(invert_long_kernel<true>, by_lists, dim3(kLongThreads), 0, st, idx, E, N, L.max_long, offsets, nlong,
                                work, entries);
    else hipLaunchKernelGGL(invert_long_kernel<false>, by_lists, dim3(kLongThreads), 0, st, idx, E, N, L.max_long, offsets, nlong,
                            work, entries);
    if ((rc = nsdp::launch_status("invert_long_kernel"))) return rc;
  }
  return 0;
}
