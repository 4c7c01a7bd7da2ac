// Exact k-nearest-neighbour search of large clouds through a uniform cell grid (include/nsdp_search.h).
//
// knn.hip tests every query against every source point of its shape: n x m distance tests.  Here the source points of every
// shape are binned into the cells of a grid over the shape's bounding box, and a query visits its own cell and shells of
// growing Chebyshev radius around it until it can prove that no unvisited point can enter its list.
//
// Phases, separate launches on the caller's stream (no workgroup ever waits for another inside a kernel):
//   memset     the zeroed part of the workspace: the search's partial counters, the per-shape cursors, the raw bounds, the cell
//              counts;
//   bounds     per shape the bounding box of its own rows, fp32, by integer atomic maxima over order-preserving encodings;
//   params     per shape: cell side h = largest extent / Gs, 1/h, the cell counts per axis g = cell(hi) + 1 <= Gs, the extent
//              and the slack of the stop rule; G = min(128, ceil(sqrt(m_max / 4))) is a host number (m_max = m or n_max), so
//              the cell arrays have a host-known size, G^3 cells per shape, and Gs = min(G, ceil(sqrt(m_s / 4))) follows the
//              shape's own row count;
//   count      one lane per source point: its cell, one integer atomic;
//   ranges     every cell gets a range [start, end) of the shape's m slots: a block scan of 1024 counts and one atomic per
//              workgroup on the shape's cursor -- the blocks lie in whatever order the workgroups arrive, the ranges inside
//              a block follow each other;
//   scatter    every point is written as (x, y, z, bits(index within the shape)) into its cell's range, in whatever order the
//              lanes arrive;
//   search     one lane per query, 64 queries per workgroup.  In the self-search (query == source) lane t takes the t-th point
//              of the SORTED array as its query and writes to that point's original row: the lanes of a wave are neighbours in
//              space and walk the same cells, whose points come from the caches.  Other queries are taken as they come.
//
// A cell coordinate is clamp(floor((p - lo) * (1/h)), 0, g - 1) per axis, clamped as a float in a form that sends NaN to 0
// before the conversion: whatever the coordinates hold, a cell index lies inside the shape's G^3 cells.  Every slot index read
// back from the workspace is clamped to the shape's rows.
//
// Exactness.  The list is ordered by the pair (distance, index) -- insert when d < bd[u] || (d == bd[u] && j < bi[u]) -- a
// strict total order, and d is nsdp::sq_dist3 with contraction off, the scan's bits.  The k smallest pairs of a set are unique,
// so the result does not depend on the order in which candidates arrive: it equals the scan's as soon as every point that can
// enter the list has been seen.
//
// The stop rule lives in the box's own frame u = fl(p - lo), the first operation of the cell function, so nothing in it scales
// with where the cloud sits.  Roundings are written (1 + e), |e| <= 2^-24; ext is the largest extent, h = fl(ext / Gs).
//   cell    c(p) = clamp(floor(fl(u_p * inv_h))), inv_h = fl(1 / h) = (1 + e2) / h.  After shell R the visited block is
//           [c - R, c + R] per axis (cut to the grid).  An unvisited point has, on some axis, a cell >= e = c + R + 1 or
//           <= c - R - 1.  Rounding is monotone and e is a float, so fl(u_p * inv_h) >= e gives u_p * inv_h >= e (1 - 2^-24),
//           and fl(u_p * inv_h) < e (e = c - R) gives u_p * inv_h < e.  The clamp keeps both (a clamped cell lies between 0 and
//           floor of the product).  With the edge E = fl(e * h) = e h (1 + e3):  u_p >= E (1 - 2^-22), resp. u_p < E (1 + 2^-22).
//           Every e used is <= g - 1 <= Gs - 1, so 0 <= E <= ext.
//   frame   u_p = (p - lo)(1 + ep), uq = fl(q - lo) = (q - lo)(1 + eq): relative to |u|, not to |p|.  The true difference is
//           p - q = u_p / (1 + ep) - uq / (1 + eq), increasing in u_p >= 0, hence
//           p - q >= E - uq - 2^-21 ext - 2^-23 |uq|   (and q - p >= uq - E - the same) for every unvisited point.
//   gap     the kernel forms fl(fl(E - uq) - s) with s = 2^-20 ext + 2^-22 |uq|: the inner subtraction errs by at most
//           2^-24 (E + |uq|), so s covers the frame's terms and this one with a factor 1.8 to spare (which also swallows the
//           rounding of s itself); the outer subtraction errs by 2^-24 of the gap.  So gap <= |p - q| (1 + 2^-24) on the offending
//           axis, taken as the smallest over the faces that still have cells beyond them.
//   bound   fl(fl(gap * gap) * (1 - 2^-19)) <= |p - q|^2 (1 - 2^-19.3), for gaps in [1e-15, 1e18] whose squares are normal
//           numbers; any other gap proves nothing (bound 0).  The computed distance is at least fl(dx * dx) with dx = fl(q - p)
//           (adding non-negative terms and rounding cannot go below a float already reached), >= |p - q|^2 (1 - 2^-24)^3.
// So bound is STRICTLY below the computed sq_dist3 of every unvisited point, wherever the cloud sits: the slack follows the
// extent, plus a term in |uq| that matters only for queries outside the box.  A box whose extent is a few ulps of its offset
// changes nothing: u is then exact, and the argument never used the size of lo.  The query stops when its k-th distance is
// strictly below the bound -- an unvisited point can then not even tie -- or when the block covers the whole grid.
//
// Budget.  Shells are opened while that is cheaper than the exhaustive finish.  A query counts its work, one per row of cells
// read and one per distance test, and gives up when the count passes kBudgetFloor + m / kBudgetShare: a wave whose lanes all
// need the finish pays m steps for it, a wave with one such lane m / 64, and the shells of a query run in one divergent lane;
// m / 4 lies between the two and is 1.7 times the most a clustered surface was seen to need.  A query farther
// outside the box than the box's largest extent, on any axis, gets no budget: its neighbours are spread over the side of the
// cloud that faces it, the faces on the other axes stay closer than its k-th distance until the block has all but covered
// them, and the rule ends, if at all, after most of the grid's rows and most of the m tests.  (An argument, NOT measured: no
// build gave such queries a budget.  What they cost without one is measured: 500 queries 1.2 to 2.5 extents outside take
// the finish in 18.1 ms, as the 50-sigma ones do.)
//
// Finish.  The lanes that gave up empty their lists, and the WAVE scans the shape's rows for them, 64 consecutive rows per load,
// coalesced, in one of two forms chosen per wave by the number of its needy lanes:
//   queries broadcast (up to kCrowd needy lanes, K <= 16)   for each needy lane in turn its query and its k-th pair are
//           broadcast, every lane tests its own row, a ballot marks the candidates that beat the k-th pair under the same
//           (distance, index) order, and the owner lane inserts them with the same `consider` into the same registers: m / 64
//           steps per needy lane.
//   rows broadcast (more needy lanes; always at K = 32)      each row in turn is broadcast, every needy lane tests it against
//           its own query and inserts into its own list, all of them side by side: m steps, whatever the number of needy lanes.
// Exact by construction; the order of arrival is irrelevant as above.  Every lane of the wave takes part, also lanes without a
// query, and all loop bounds are wave-uniform.  No LDS, no barrier.  Measured, 500 far queries against 100 000 points, k = 16
// (profiles/knn_grid_anywhere.txt): rows broadcast 18.2 ms, queries broadcast 25.4 ms, one plain scan per lane (the parent) 20.1 ms.
// The first costs a wave the same whatever its needy lanes, the second grows with their number, so they meet at 64 * 18.2 /
// 25.4 = 45.7 needy lanes: kCrowd = 45.  K = 32 has the second form alone: see the kernel.
//
// Limits.  G follows sqrt(m / 4), the density of a SURFACE, and is one number per shape.  A volume-filling cloud has 8 / sqrt(m)
// points per cell and walks several hundred mostly empty rows per query; a cluster that falls into a handful of cells costs
// every query near it all the points of those cells.  Both are exact and pruned, neither is what the grid was sized for; a
// density-adaptive grid is not built.  Queries other than the self-search are not binned.  A call whose queries ALL take the
// finish (500 far queries against 100 000 points: 18.2 ms, the parent 20.1, the scan kernel 1.6) is the scan's work done by 8
// waves: the scan wins it, and the dispatch cannot know.
#include <cfloat>
#include <climits>
#include <vector>

#include "common.h"
#include "prof.h"
#include "ragged.h"

#include "../../include/nsdp_search.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMaxGrid = 128;                 // cells per axis at most
constexpr int kBudgetShare = 4;               // a query opens shells until its rows read + tests pass kBudgetFloor + m / kBudgetShare
constexpr int kBudgetFloor = 64;
constexpr int kBothFormsMaxK = 16;            // longer lists: the row-broadcast finish alone
constexpr int kCrowd = 45;                    // more needy lanes in a wave than this: the finish broadcasts rows, not queries
constexpr int kMaxK = 32;
constexpr int kMaxPoints = 1 << 20;           // source points per shape
constexpr int kSearchLanes = 64;              // queries per workgroup of the search
constexpr int kRangeBlock = 1024;             // consecutive cells whose ranges one workgroup lays out back to back
constexpr unsigned kMagic = 0x6b6e6e67u;      // "knng": the header of a workspace a call has used
constexpr size_t kHeadBytes = 64;

struct Head {                                 // first bytes of the workspace, written by the params kernel
  unsigned magic;
  unsigned partials;
  long long cells;
};

int grid_dim(int m_max) {                     // ceil(sqrt(m_max / 4)) in [1, 128]
  int g = 1;
  while (g < kMaxGrid && 4LL * g * g < m_max) ++g;
  return g;
}

inline size_t up16(size_t v) { return (v + 15) / 16 * 16; }

struct Layout {
  int G, P;
  long long C;
  size_t partials, cursor, raw, count, zero_end, params, ranges, sorted, total;
};

Layout layout(long long B, long long queries, long long source_rows, int m_max) {
  Layout L;
  L.G = grid_dim(m_max);
  L.C = static_cast<long long>(L.G) * L.G * L.G;
  L.P = static_cast<int>((queries + kSearchLanes - 1) / kSearchLanes + B);
  size_t at = kHeadBytes;
  L.partials = at; at += up16(static_cast<size_t>(L.P) * 16);
  L.cursor = at;   at += up16(static_cast<size_t>(B) * 4);
  L.raw = at;      at += static_cast<size_t>(B) * 32;
  L.count = at;    at += up16(static_cast<size_t>(B) * L.C * 4);
  L.zero_end = at;
  L.params = at;   at += static_cast<size_t>(B) * 64;
  L.ranges = at;   at += up16(static_cast<size_t>(B) * L.C * 8);
  L.sorted = at;   at += static_cast<size_t>(source_rows) * 16;
  L.total = at;
  return L;
}

struct Workspace {                            // device pointers into the caller's workspace
  Head *head;
  uint4 *partials;
  int *cursor;
  unsigned *raw;                              // [B][8]: ~enc(lo) x y z, enc(hi) x y z
  int *count;                                 // [B][C]
  float *params;                              // [B][16]
  int2 *ranges;                               // [B][C]
  float4 *sorted;                             // [source rows]
};

Workspace carve(void *workspace, const Layout &L) {
  char *p = static_cast<char *>(workspace);
  Workspace w;
  w.head = reinterpret_cast<Head *>(p);
  w.partials = reinterpret_cast<uint4 *>(p + L.partials);
  w.cursor = reinterpret_cast<int *>(p + L.cursor);
  w.raw = reinterpret_cast<unsigned *>(p + L.raw);
  w.count = reinterpret_cast<int *>(p + L.count);
  w.params = reinterpret_cast<float *>(p + L.params);
  w.ranges = reinterpret_cast<int2 *>(p + L.ranges);
  w.sorted = reinterpret_cast<float4 *>(p + L.sorted);
  return w;
}

// order-preserving map of the non-NaN floats onto unsigned (a NaN lands at one of the ends: the box is then not finite)
__device__ __forceinline__ unsigned enc(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float dec(unsigned e) { return __uint_as_float((e & 0x80000000u) ? (e & 0x7fffffffu) : ~e); }

// The source rows of this workgroup's tile of kT rows: shape b owns rows [lo, lo + m) of `source` (a packed set: offsets
// clamped as ragged.h clamps them, m clamped to n_max; a rectangular one: offsets NULL, n_max = m, the shape is the grid's y
// index), and the tile starts at row0.  false: nothing to do (before any barrier).
template <int kT>
__device__ __forceinline__ bool source_tile(const int32_t *__restrict__ offsets, int B, int cap, int n_max, int &b, int &lo,
                                            int &m, int &row0) {
  if (offsets) {
    int end, hi;
    if (!nsdp::ragged_tile<kT>(offsets, B, cap, static_cast<int>(blockIdx.x), b, row0, end)) return false;
    nsdp::ragged_range(offsets, b, cap, lo, hi);
    m = min(hi - lo, n_max);
    return row0 < lo + m;
  }
  b = blockIdx.y;
  lo = b * n_max;
  m = n_max;
  row0 = lo + static_cast<int>(blockIdx.x) * kT;
  return static_cast<int>(blockIdx.x) * kT < m;
}

struct Grid {
  float lox, loy, loz, inv_h, h, slack, ext;
  int gx, gy, gz;
};

__device__ __forceinline__ Grid load_grid(const float *__restrict__ params, int b, int G) {
  const float4 a = *reinterpret_cast<const float4 *>(params + static_cast<size_t>(b) * 16);
  const float4 c = *reinterpret_cast<const float4 *>(params + static_cast<size_t>(b) * 16 + 4);
  const int4 g = *reinterpret_cast<const int4 *>(params + static_cast<size_t>(b) * 16 + 8);
  Grid r;
  r.lox = a.x; r.loy = a.y; r.loz = a.z; r.inv_h = a.w;
  r.h = c.x; r.slack = c.y; r.ext = c.z;
  // (read back from memory: clamped, so that nothing downstream depends on what the workspace holds)
  r.gx = min(max(g.x, 1), G); r.gy = min(max(g.y, 1), G); r.gz = min(max(g.z, 1), G);
  return r;
}

// clamp(floor((p - lo) * inv_h), 0, g - 1), clamped in the float domain: NaN fails `v > 0` and becomes cell 0, +inf becomes
// g - 1; only then an integer.  Monotone in p.
__device__ __forceinline__ int axis_cell(float p, float lo, float inv_h, int g) {
  const float v = floorf(__fmul_rn(__fsub_rn(p, lo), inv_h));
  const float c = v > 0.f ? fminf(v, static_cast<float>(g - 1)) : 0.f;
  return static_cast<int>(c);
}

__device__ __forceinline__ int cell_of(const Grid &g, float x, float y, float z) {
  const int cx = axis_cell(x, g.lox, g.inv_h, g.gx), cy = axis_cell(y, g.loy, g.inv_h, g.gy), cz = axis_cell(z, g.loz, g.inv_h, g.gz);
  return (cz * g.gy + cy) * g.gx + cx;      // < gx * gy * gz <= G^3
}

// ---------------------------------------------------------------------------------------------------------------- bounds
__global__ __launch_bounds__(256) void knn_grid_bounds_kernel(const float *__restrict__ source, const int32_t *__restrict__ offsets,
                                                              int B, int cap, int n_max, unsigned *__restrict__ raw) {
  __shared__ unsigned part[4][6];
  int b, lo, m, row0;
  if (!source_tile<1024>(offsets, B, cap, n_max, b, lo, m, row0)) return;
  unsigned v[6] = {0u, 0u, 0u, 0u, 0u, 0u};      // 0: the identity of the maxima
  for (int s = 0; s < 4; ++s) {
    const int row = row0 + s * 256 + static_cast<int>(threadIdx.x);
    if (row < lo + m) {
      const float *p = source + static_cast<size_t>(row) * 3;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const unsigned e = enc(p[a]);
        v[a] = max(v[a], ~e);
        v[3 + a] = max(v[3 + a], e);
      }
    }
  }
#pragma unroll
  for (int a = 0; a < 6; ++a)
    for (int off = 32; off > 0; off >>= 1) v[a] = max(v[a], static_cast<unsigned>(__shfl_xor(static_cast<int>(v[a]), off)));
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int a = 0; a < 6; ++a) part[threadIdx.x >> 6][a] = v[a];
  __syncthreads();
  if (threadIdx.x < 6) {
    const unsigned best = max(max(part[0][threadIdx.x], part[1][threadIdx.x]), max(part[2][threadIdx.x], part[3][threadIdx.x]));
    atomicMax(raw + static_cast<size_t>(b) * 8 + threadIdx.x, best);
  }
}

// ---------------------------------------------------------------------------------------------------------------- params
__global__ __launch_bounds__(256) void knn_grid_params_kernel(const unsigned *__restrict__ raw, const int32_t *__restrict__ offsets,
                                                              int B, int cap, int n_max, int G, unsigned partials, long long cells,
                                                              float *__restrict__ params, Head *head) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b == 0) {
    head->magic = kMagic;
    head->partials = partials;
    head->cells = cells;
  }
  if (b >= B) return;
  // The shape's own grid: Gs = min(G, ceil(sqrt(m / 4))) from its own row count (clamped as ragged.h clamps the offsets; one
  // lane per shape, so not through the wave-uniform helpers), inside the G^3 cells the host has set aside for it.  A short
  // shape of a packed set whose bound is large gets cells of its own density.
  // (every lane walks the offsets in front of its shape: B^2 / 2 loads in all, as the O(B) walks of every workgroup of the other
  // kernels add up to -- nothing at the few shapes of a batch, about a second at the 65535 the entries accept)
  int m = n_max;
  if (offsets) {
    int l = min(max(offsets[0], 0), cap);
    for (int s = 0; s < b; ++s) l = min(max(offsets[s + 1], l), cap);
    m = min(min(max(offsets[b + 1], l), cap) - l, n_max);
  }
  int Gs = 1;
  while (Gs < G && 4LL * Gs * Gs < m) ++Gs;
  const unsigned *r = raw + static_cast<size_t>(b) * 8;
  const float lox = dec(~r[0]), loy = dec(~r[1]), loz = dec(~r[2]);
  const float hix = dec(r[3]), hiy = dec(r[4]), hiz = dec(r[5]);
  const float ext = fmaxf(fmaxf(hix - lox, hiy - loy), hiz - loz);
  const float big = fmaxf(fmaxf(fmaxf(fabsf(lox), fabsf(hix)), fmaxf(fabsf(loy), fabsf(hiy))), fmaxf(fabsf(loz), fabsf(hiz)));
  const float h = ext / static_cast<float>(Gs);
  const float inv_h = 1.0f / h;
  // a box without extent (one point, identical points, no point), a non-finite one or one of denormal size: a single cell
  const bool ok = ext > 0.f && ext < FLT_MAX && big < FLT_MAX && h >= 1e-30f && inv_h > 0.f && inv_h < FLT_MAX && lox == lox &&
                  loy == loy && loz == loz;
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f), c = make_float4(0.f, 0.f, 0.f, 0.f);
  int4 g = make_int4(1, 1, 1, 0);
  if (ok) {
    a = make_float4(lox, loy, loz, inv_h);
    c = make_float4(h, ext * 0x1p-20f, ext, 0.f);      // (the stop rule's slack follows the extent: see Exactness)
    g = make_int4(axis_cell(hix, lox, inv_h, Gs) + 1, axis_cell(hiy, loy, inv_h, Gs) + 1, axis_cell(hiz, loz, inv_h, Gs) + 1, 0);
  }
  float *p = params + static_cast<size_t>(b) * 16;
  *reinterpret_cast<float4 *>(p) = a;
  *reinterpret_cast<float4 *>(p + 4) = c;
  *reinterpret_cast<int4 *>(p + 8) = g;
  *reinterpret_cast<int4 *>(p + 12) = make_int4(0, 0, 0, 0);
}

// ---------------------------------------------------------------------------------------------------------------- binning
__global__ __launch_bounds__(256) void knn_grid_count_kernel(const float *__restrict__ source, const int32_t *__restrict__ offsets,
                                                             int B, int cap, int n_max, const float *__restrict__ params,
                                                             int G, int *__restrict__ count) {
  const long long C = static_cast<long long>(G) * G * G;
  int b, lo, m, row0;
  if (!source_tile<256>(offsets, B, cap, n_max, b, lo, m, row0)) return;
  const int row = row0 + static_cast<int>(threadIdx.x);
  if (row >= lo + m) return;
  const Grid g = load_grid(params, b, G);
  const float *p = source + static_cast<size_t>(row) * 3;
  atomicAdd(count + static_cast<size_t>(b) * C + cell_of(g, p[0], p[1], p[2]), 1);
}

// grid (ceil(C / kRangeBlock), B): four consecutive cells per lane, 256 lanes = kRangeBlock cells whose ranges follow each other
__global__ __launch_bounds__(256) void knn_grid_ranges_kernel(const int *__restrict__ count, long long C, int *__restrict__ cursor,
                                                              int2 *__restrict__ ranges) {
  __shared__ int wave_sum[4];
  __shared__ int base;
  const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long c0 = (static_cast<long long>(blockIdx.x) * 256 + threadIdx.x) * 4;
  const int *cnt_b = count + static_cast<size_t>(b) * C;
  int cnt[4], mine = 0;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    cnt[u] = c0 + u < C ? max(cnt_b[c0 + u], 0) : 0;
    mine += cnt[u];
  }
  int incl = mine;
  for (int off = 1; off < 64; off <<= 1) {
    const int v = __shfl_up(incl, off);
    if (lane >= off) incl += v;
  }
  if (lane == 63) wave_sum[wave] = incl;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int total = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
    base = total ? atomicAdd(cursor + b, total) : 0;
  }
  __syncthreads();
  int start = base + incl - mine;
  for (int w = 0; w < wave; ++w) start += wave_sum[w];
  int2 *out = ranges + static_cast<size_t>(b) * C;
#pragma unroll
  for (int u = 0; u < 4; ++u)
    if (c0 + u < C) {
      out[c0 + u] = make_int2(start, start + cnt[u]);
      start += cnt[u];
    }
}

__global__ __launch_bounds__(256) void knn_grid_scatter_kernel(const float *__restrict__ source, const int32_t *__restrict__ offsets,
                                                               int B, int cap, int n_max, const float *__restrict__ params,
                                                               int G, int *__restrict__ count,
                                                               const int2 *__restrict__ ranges, float4 *__restrict__ sorted) {
  const long long C = static_cast<long long>(G) * G * G;
  int b, lo, m, row0;
  if (!source_tile<256>(offsets, B, cap, n_max, b, lo, m, row0)) return;
  const int row = row0 + static_cast<int>(threadIdx.x);
  if (row >= lo + m) return;
  const Grid g = load_grid(params, b, G);
  const float *p = source + static_cast<size_t>(row) * 3;
  const float x = p[0], y = p[1], z = p[2];
  const size_t cell = static_cast<size_t>(b) * C + cell_of(g, x, y, z);
  const int r = atomicSub(count + cell, 1) - 1;                  // the cell's counts run back to zero
  const int slot = min(max(ranges[cell].x + r, 0), m - 1);       // (inside the shape's rows whatever was read back)
  sorted[static_cast<size_t>(lo) + slot] = make_float4(x, y, z, __int_as_float(row - lo));
}

// ---------------------------------------------------------------------------------------------------------------- search
template <int K>
__global__ __launch_bounds__(kSearchLanes) void knn_grid_search_kernel(
    const float *__restrict__ query, const int32_t *__restrict__ query_offsets, const float *__restrict__ source,
    const int32_t *__restrict__ offsets, int B, int n, int qcap, int cap, int n_max, int k, int self,
    const float *__restrict__ params, int G, const int2 *__restrict__ ranges, const float4 *__restrict__ sorted,
    uint4 *__restrict__ partials, int32_t *__restrict__ idx_all, float *__restrict__ dist_all) {
  const long long C = static_cast<long long>(G) * G * G;
  int b, row0, qlo, qend;
  if (query_offsets) {
    int qhi;
    if (!nsdp::ragged_tile<kSearchLanes>(query_offsets, B, qcap, static_cast<int>(blockIdx.x), b, row0, qend)) return;
    nsdp::ragged_range(query_offsets, b, qcap, qlo, qhi);
  } else {
    b = blockIdx.y;
    qlo = b * n;
    qend = qlo + n;
    row0 = qlo + static_cast<int>(blockIdx.x) * kSearchLanes;
  }
  int lo, m, idx_base, idx_max;
  if (offsets) {
    int hi;
    nsdp::ragged_range(offsets, b, cap, lo, hi);
    m = min(hi - lo, n_max);
    idx_base = lo;
    idx_max = cap - 1;
  } else {
    lo = b * n_max;
    m = n_max;
    idx_base = 0;
    idx_max = INT_MAX;
  }
  const int row = row0 + static_cast<int>(threadIdx.x), lane = static_cast<int>(threadIdx.x);
  const bool live = row < qend;      // (a lane without a query still takes part in the finish of the others)
  unsigned tests = 0, scanned = 0, queries = 0;
  float qx = 0.f, qy = 0.f, qz = 0.f;
  size_t out_row = 0;
  float bd[K];
  int bi[K];
#pragma unroll
  for (int t = 0; t < K; ++t) {
    bd[t] = FLT_MAX;      // an empty slot: (FLT_MAX, -1) lets no candidate at FLT_MAX in, as the scan's `d < FLT_MAX` does not
    bi[t] = -1;
  }
  auto consider = [&](float d, int j) __attribute__((always_inline)) {
    if (d < bd[K - 1] || (d == bd[K - 1] && j < bi[K - 1])) {
#pragma unroll
      for (int u = K - 1; u > 0; --u) {
        const bool shift = d < bd[u - 1] || (d == bd[u - 1] && j < bi[u - 1]);
        const bool here = !shift && (d < bd[u] || (d == bd[u] && j < bi[u]));
        const float nd = shift ? bd[u - 1] : (here ? d : bd[u]);
        const int ni = shift ? bi[u - 1] : (here ? j : bi[u]);
        bd[u] = nd;
        bi[u] = ni;
      }
      if (d < bd[0] || (d == bd[0] && j < bi[0])) {
        bd[0] = d;
        bi[0] = j;
      }
    }
  };
  bool done = true;
  if (live) {
    queries = 1;
    out_row = static_cast<size_t>(row);
    if (self && row - qlo < m) {      // the self-search in cell order: this lane's query is a sorted point, its row that point's
      const float4 P = sorted[static_cast<size_t>(lo) + (row - qlo)];
      qx = P.x; qy = P.y; qz = P.z;
      out_row = static_cast<size_t>(qlo) + min(max(__float_as_int(P.w), 0), m - 1);
    } else {
      const float *qp = query + static_cast<size_t>(row) * 3;
      qx = qp[0]; qy = qp[1]; qz = qp[2];
    }
    const Grid g = load_grid(params, b, G);
    const int cx = axis_cell(qx, g.lox, g.inv_h, g.gx), cy = axis_cell(qy, g.loy, g.inv_h, g.gy), cz = axis_cell(qz, g.loz, g.inv_h, g.gz);
    // the query in the box's frame, the first operation of axis_cell: the stop rule's arithmetic stays there (see Exactness)
    const float ux = __fsub_rn(qx, g.lox), uy = __fsub_rn(qy, g.loy), uz = __fsub_rn(qz, g.loz);
    const float sx = g.slack + 0x1p-22f * fabsf(ux), sy = g.slack + 0x1p-22f * fabsf(uy), sz = g.slack + 0x1p-22f * fabsf(uz);
    // rows read + tests this query may spend on shells; none for a query farther outside the box than the box is wide
    const bool far = ux < -g.ext || ux > 2.f * g.ext || uy < -g.ext || uy > 2.f * g.ext || uz < -g.ext || uz > 2.f * g.ext;
    const unsigned budget = far ? 0u : static_cast<unsigned>(kBudgetFloor + m / kBudgetShare);
    unsigned reads = 0;
    const int2 *cells = ranges + static_cast<size_t>(b) * C;
    const float4 *pts = sorted + static_cast<size_t>(lo);
    done = false;
    for (int R = 0; R < kMaxGrid; ++R) {      // (shell kMaxGrid - 1 covers any grid)
      const int z0 = max(cz - R, 0), z1 = min(cz + R, g.gz - 1), y0 = max(cy - R, 0), y1 = min(cy + R, g.gy - 1);
      for (int z = z0; z <= z1; ++z)
        for (int y = y0; y <= y1; ++y) {
          // shell R: whole rows on the z and y faces, the two ends of the row elsewhere
          const bool face = z - cz == R || cz - z == R || y - cy == R || cy - y == R;
          const int step = face ? 1 : 2 * R;
          const int xa = face ? max(cx - R, 0) : cx - R, xb = face ? min(cx + R, g.gx - 1) : cx + R;
          const int row_base = (z * g.gy + y) * g.gx;
          for (int x = xa; x <= xb;) {
            if (x < 0 || x >= g.gx) {      // (an end of a row outside the grid)
              x += step;
              continue;
            }
            // the ranges of the 1024 consecutive cells one workgroup has laid out follow each other: the cells of a row up to
            // the end of that block are one run of slots
            const int c = row_base + x;
            const int xe = face ? min(xb, x + (kRangeBlock - 1 - (c & (kRangeBlock - 1)))) : x;
            const int first = cells[c].x, last = cells[row_base + xe].y;
            const int j0 = min(max(first, 0), m), j1 = min(max(last, j0), m);
            ++reads;
            if (j0 < j1) {
              float4 P = pts[j0];
              for (int j = j0; j < j1; ++j) {
                const float4 next = pts[min(j + 1, j1 - 1)];      // (in flight during the insertion)
                ++tests;
                consider(nsdp::sq_dist3(qx, qy, qz, P.x, P.y, P.z), __float_as_int(P.w));
                P = next;
              }
            }
            x = face ? xe + 1 : x + step;
          }
        }
      // the faces of the visited block that still have cells beyond them
      const bool more_x0 = cx - R > 0, more_x1 = cx + R < g.gx - 1, more_y0 = cy - R > 0, more_y1 = cy + R < g.gy - 1,
                 more_z0 = cz - R > 0, more_z1 = cz + R < g.gz - 1;
      if (!(more_x0 || more_x1 || more_y0 || more_y1 || more_z0 || more_z1)) {
        done = true;      // the block covers the grid: every point of the shape has been seen
        break;
      }
      float kth = bd[0];
#pragma unroll
      for (int t = 1; t < K; ++t) kth = (t == k - 1) ? bd[t] : kth;
      float gap = FLT_MAX;
      if (more_x0) gap = fminf(gap, (ux - static_cast<float>(cx - R) * g.h) - sx);
      if (more_x1) gap = fminf(gap, (static_cast<float>(cx + R + 1) * g.h - ux) - sx);
      if (more_y0) gap = fminf(gap, (uy - static_cast<float>(cy - R) * g.h) - sy);
      if (more_y1) gap = fminf(gap, (static_cast<float>(cy + R + 1) * g.h - uy) - sy);
      if (more_z0) gap = fminf(gap, (uz - static_cast<float>(cz - R) * g.h) - sz);
      if (more_z1) gap = fminf(gap, (static_cast<float>(cz + R + 1) * g.h - uz) - sz);
      // (a gap too small to square without underflow, or so large that its square overflows, proves nothing)
      const float bound = (gap > 1e-15f && gap < 1e18f) ? (gap * gap) * (1.0f - 0x1p-19f) : 0.f;
      if (kth < FLT_MAX && kth < bound) {
        done = true;
        break;
      }
      if (reads + tests > budget) break;      // the finish is cheaper from here
    }
  }
  // The exhaustive finish, by the whole wave for all its lanes that gave up.  Every lane of the wave arrives here, and `needy`,
  // the choice between the two forms, `owner` and the row loops are wave-uniform (m and lo belong to the workgroup's shape).
  //   few needy lanes   the QUERIES are broadcast.  The rows are the outer loop and the needy lanes the inner one: 4 x 64 rows
  //                     are loaded once, coalesced, and serve every needy lane before the next load; m / 64 steps per needy
  //                     lane, the insertions in the owner lane alone.
  //   a crowded wave    the ROWS are broadcast: m steps, in each of them every needy lane tests the row against its own query
  //                     and inserts into its own list -- as many tests per step, without the five broadcasts and the ballot
  //                     per needy lane and with the insertions of a step side by side.
  const unsigned long long needy = __ballot(!done);
  if (needy && m > 0) {
    float kd = FLT_MAX;      // this lane's k-th pair, what a candidate has to beat: kept beside the list for the broadcast
    int ki = -1;
    if (!done) {      // start over: a list that holds only rows of this scan cannot name a row twice
      scanned = 1;
      tests += static_cast<unsigned>(m);
#pragma unroll
      for (int t = 0; t < K; ++t) {
        bd[t] = FLT_MAX;
        bi[t] = -1;
      }
    }
    const float *src = source + static_cast<size_t>(lo) * 3;
    // (K = 32 has this form alone, which costs any wave what one plain scan per lane did: with both forms that kernel needs
    // 160 registers, not 121, a wave per SIMD less for every search, and with the other form alone a crowded wave takes twice
    // the time of the plain scans)
    if (K > kBothFormsMaxK || __popcll(needy) > kCrowd) {
      // 64 rows one per lane, the next 64 in flight meanwhile (the last row of the shape again past its end; m >= 1 here: a
      // shape without rows is a single cell, which shell 0 covers)
      int j = min(lane, m - 1);
      float px = src[j * 3 + 0], py = src[j * 3 + 1], pz = src[j * 3 + 2];
      for (int jb = 0; jb < m; jb += kSearchLanes) {
        j = min(jb + kSearchLanes + lane, m - 1);
        const float nx = src[j * 3 + 0], ny = src[j * 3 + 1], nz = src[j * 3 + 2];
        const int rows = min(kSearchLanes, m - jb);
#pragma unroll 1
        for (int r = 0; r < rows; ++r) {
          const float rx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(px), r));
          const float ry = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(py), r));
          const float rz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pz), r));
          // (a lane that is not needy offers FLT_MAX, which enters no list: an empty slot is (FLT_MAX, -1))
          consider(done ? FLT_MAX : nsdp::sq_dist3(qx, qy, qz, rx, ry, rz), jb + r);
        }
        px = nx; py = ny; pz = nz;
      }
    } else
    for (int j0 = 0; j0 < m; j0 += 4 * kSearchLanes) {
      float px[4], py[4], pz[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {      // 4 x 64 consecutive rows in flight (the last row of the shape again past its end)
        const int j = min(j0 + u * kSearchLanes + lane, m - 1);
        px[u] = src[j * 3 + 0]; py[u] = src[j * 3 + 1]; pz[u] = src[j * 3 + 2];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int jb = j0 + u * kSearchLanes, j = jb + lane;
        if (jb >= m) break;
        for (unsigned long long left = needy; left; left &= left - 1) {
          const int owner = __builtin_amdgcn_readfirstlane(__ffsll(left) - 1);
          const float ox = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(qx), owner));
          const float oy = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(qy), owner));
          const float oz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(qz), owner));
          const float od = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(kd), owner));
          const int oi = __builtin_amdgcn_readlane(ki, owner);
          const float d = nsdp::sq_dist3(ox, oy, oz, px[u], py[u], pz[u]);
          unsigned long long cand = __ballot(j < m && (d < od || (d == od && j < oi)));
          if (cand) {
            do {
              const int from = __builtin_amdgcn_readfirstlane(__ffsll(cand) - 1);
              cand &= cand - 1;
              const float dc = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(d), from));
              if (lane == owner) consider(dc, jb + from);
            } while (cand);
            if (lane == owner) {
              kd = bd[0];
              ki = bi[0];
#pragma unroll
              for (int t = 1; t < K; ++t) {
                kd = (t == k - 1) ? bd[t] : kd;
                ki = (t == k - 1) ? bi[t] : ki;
              }
            }
          }
        }
      }
    }
  }
  if (live) {
    int32_t *io = idx_all + out_row * k;
#pragma unroll
    for (int t = 0; t < K; ++t)
      if (t < k) io[t] = min(max(bi[t], 0) + idx_base, idx_max);      // (an empty slot names the shape's first row)
    if (dist_all) {
      float *dout = dist_all + out_row * k;
#pragma unroll
      for (int t = 0; t < K; ++t)
        if (t < k) dout[t] = bd[t];
    }
  }
  // one partial per workgroup (= wave), a plain vector store: nsdp_knn_grid_stats sums them on the host
  unsigned long long t64 = tests;
  for (int off = 32; off > 0; off >>= 1) {
    t64 += static_cast<unsigned long long>(__shfl_xor(static_cast<long long>(t64), off));
    scanned += static_cast<unsigned>(__shfl_xor(static_cast<int>(scanned), off));
    queries += static_cast<unsigned>(__shfl_xor(static_cast<int>(queries), off));
  }
  if (threadIdx.x == 0)
    partials[static_cast<size_t>(blockIdx.y) * gridDim.x + blockIdx.x] =
        make_uint4(queries, scanned, static_cast<unsigned>(t64), static_cast<unsigned>(t64 >> 32));
}

// One call: rectangular source (offsets NULL, cap = B * m, n_max = m) or packed; rectangular queries (query_offsets NULL) or
// packed.  Everything the grids need is a host number.
int run(const float *query, const int32_t *qoff, const float *source, const int32_t *offsets, int B, int n, int qcap, int cap,
        int n_max, int k, void *workspace, int32_t *idx, float *d2, hipStream_t st) {
  const long long rows = qoff ? qcap : static_cast<long long>(B) * n;
  const Layout L = layout(B, rows, cap, n_max);
  const Workspace w = carve(workspace, L);
  // the self-search: the queries are the source rows themselves, shape for shape
  const int self = query == source && (qoff ? (qoff == offsets && qcap == cap) : (!offsets && n == n_max));
  nsdp::prof::Scope scope(nsdp::prof::kKnn, st, 0.0,
                          12.0 * (static_cast<double>(rows) + cap) + 4.0 * rows * k * (d2 ? 2 : 1) + 28.0 * cap +
                              16.0 * static_cast<double>(B) * L.C);
  NSDP_TRACE("knn_grid<%d>", k <= 8 ? 8 : k <= 16 ? 16 : 32);
  NSDP_HIP_TRY(hipMemsetAsync(static_cast<char *>(workspace) + kHeadBytes, 0, L.zero_end - kHeadBytes, st));
  const auto tiles = [&](int t) {
    return offsets ? dim3(static_cast<unsigned>(nsdp::ragged_max_tiles(cap, B, t))) : dim3(nsdp::ceil_div(n_max, t), B);
  };
  int rc;
  hipLaunchKernelGGL(knn_grid_bounds_kernel, tiles(1024), dim3(256), 0, st, source, offsets, B, cap, n_max, w.raw);
  if ((rc = nsdp::launch_status("knn_grid_bounds_kernel"))) return rc;
  hipLaunchKernelGGL(knn_grid_params_kernel, dim3(nsdp::ceil_div(B, 256)), dim3(256), 0, st, w.raw, offsets, B, cap, n_max,
                     L.G, static_cast<unsigned>(L.P), static_cast<long long>(B) * L.C, w.params, w.head);
  if ((rc = nsdp::launch_status("knn_grid_params_kernel"))) return rc;
  hipLaunchKernelGGL(knn_grid_count_kernel, tiles(256), dim3(256), 0, st, source, offsets, B, cap, n_max, w.params, L.G, w.count);
  if ((rc = nsdp::launch_status("knn_grid_count_kernel"))) return rc;
  hipLaunchKernelGGL(knn_grid_ranges_kernel, dim3(nsdp::ceil_div(L.C, kRangeBlock), B), dim3(256), 0, st, w.count, L.C, w.cursor,
                     w.ranges);
  static_assert(kRangeBlock == 256 * 4, "knn_grid_ranges_kernel: four cells per lane");
  if ((rc = nsdp::launch_status("knn_grid_ranges_kernel"))) return rc;
  hipLaunchKernelGGL(knn_grid_scatter_kernel, tiles(256), dim3(256), 0, st, source, offsets, B, cap, n_max, w.params, L.G, w.count,
                     w.ranges, w.sorted);
  if ((rc = nsdp::launch_status("knn_grid_scatter_kernel"))) return rc;
  const dim3 grid = qoff ? dim3(static_cast<unsigned>(nsdp::ragged_max_tiles(qcap, B, kSearchLanes)))
                         : dim3(nsdp::ceil_div(n, kSearchLanes), B);
#define NSDP_GRID_SEARCH(KK)                                                                                                  \
  hipLaunchKernelGGL((knn_grid_search_kernel<KK>), grid, dim3(kSearchLanes), 0, st, query, qoff, source, offsets, B, n, qcap, \
                     cap, n_max, k, self, w.params, L.G, w.ranges, w.sorted, w.partials, idx, d2)
  if (k <= 8) NSDP_GRID_SEARCH(8);
  else if (k <= 16) NSDP_GRID_SEARCH(16);
  else NSDP_GRID_SEARCH(32);
#undef NSDP_GRID_SEARCH
  return nsdp::launch_status("knn_grid_search_kernel");
}

}  // namespace

extern "C" size_t nsdp_knn_grid_workspace_bytes(int B, int queries, int source_rows, int m_max) {
  if (B <= 0 || B > 65535 || queries <= 0 || source_rows <= 0 || m_max <= 0 || m_max > kMaxPoints) return 0;
  return layout(B, queries, source_rows, m_max).total;
}

extern "C" int nsdp_knn_grid(const float *query, const float *source, int B, int n, int m, int k, void *workspace,
                             int32_t *idx_out, float *dist_out, void *stream) {
  if (B <= 0 || n <= 0 || k <= 0) return 0;
  NSDP_REQUIRE(query && source && idx_out, "knn_grid: null pointer");
  NSDP_REQUIRE(k <= m, "knn_grid: k=%d exceeds the number of source points m=%d", k, m);
  NSDP_REQUIRE(k <= kMaxK, "knn_grid: k=%d > %d is not supported", k, kMaxK);
  NSDP_REQUIRE(m <= kMaxPoints, "knn_grid: m=%d source points per shape exceed the limit %d", m, kMaxPoints);
  NSDP_REQUIRE(B <= 65535, "knn_grid: batch %d too large for one launch", B);
  NSDP_REQUIRE(static_cast<long long>(B) * m < (1LL << 31) && static_cast<long long>(B) * n * k < (1LL << 31),
               "knn_grid: %d shapes of %d x %d points with k=%d are too large", B, n, m, k);
  NSDP_REQUIRE(workspace, "knn_grid: null workspace pointer");
  return run(query, nullptr, source, nullptr, B, n, 0, B * m, m, k, workspace, idx_out, dist_out, nsdp::as_stream(stream));
}

extern "C" int nsdp_knn_grid_ragged_source(const float *query, const int32_t *query_offsets, const float *source,
                                           const int32_t *offsets, int B, int n, int qcap, int cap, int n_max, int k,
                                           void *workspace, int32_t *idx_out, float *dist_out, void *stream) {
  const long long rows = query_offsets ? static_cast<long long>(qcap) : static_cast<long long>(B) * n;
  if (B <= 0 || rows <= 0 || k <= 0) return 0;
  NSDP_REQUIRE(query && source && offsets && idx_out, "knn_grid_ragged_source: null pointer");
  NSDP_REQUIRE(cap > 0 && n_max > 0, "knn_grid_ragged_source: cap and n_max must be positive (got %d, %d)", cap, n_max);
  n_max = n_max < cap ? n_max : cap;
  NSDP_REQUIRE(k <= n_max, "knn_grid_ragged_source: k=%d exceeds the bound of a shape's source points n_max=%d", k, n_max);
  NSDP_REQUIRE(k <= kMaxK, "knn_grid_ragged_source: k=%d > %d is not supported", k, kMaxK);
  NSDP_REQUIRE(n_max <= kMaxPoints, "knn_grid_ragged_source: n_max=%d source points per shape exceed the limit %d", n_max, kMaxPoints);
  NSDP_REQUIRE(B <= 65535, "knn_grid_ragged_source: batch %d too large for one launch", B);
  NSDP_REQUIRE(rows * k < (1LL << 31), "knn_grid_ragged_source: %lld query rows x k=%d too large", rows, k);
  NSDP_REQUIRE(workspace, "knn_grid_ragged_source: null workspace pointer");
  return run(query, query_offsets, source, offsets, B, n, qcap, cap, n_max, k, workspace, idx_out, dist_out,
             nsdp::as_stream(stream));
}

extern "C" int nsdp_knn_grid_stats(const void *workspace, void *stream, int64_t out[4]) {
  NSDP_REQUIRE(workspace && out, "knn_grid_stats: null pointer");
  hipStream_t st = nsdp::as_stream(stream);
  Head head;
  NSDP_HIP_TRY(hipMemcpyAsync(&head, workspace, sizeof(head), hipMemcpyDeviceToHost, st));
  NSDP_HIP_TRY(hipStreamSynchronize(st));
  NSDP_REQUIRE(head.magic == kMagic && head.partials <= (1u << 31) / kSearchLanes + 65536u,
               "knn_grid_stats: no search has used this workspace");
  std::vector<uint4> parts(head.partials);
  if (!parts.empty()) {
    NSDP_HIP_TRY(hipMemcpyAsync(parts.data(), static_cast<const char *>(workspace) + kHeadBytes, parts.size() * sizeof(uint4),
                                hipMemcpyDeviceToHost, st));
    NSDP_HIP_TRY(hipStreamSynchronize(st));
  }
  out[0] = out[1] = out[2] = 0;
  out[3] = head.cells;
  for (const uint4 &p : parts) {
    out[0] += p.x;
    out[2] += p.y;
    out[1] += static_cast<int64_t>(p.z) | (static_cast<int64_t>(p.w) << 32);
  }
  return 0;
}
