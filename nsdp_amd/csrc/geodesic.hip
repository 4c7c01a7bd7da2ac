// Geodesic distances over the edge graph of packed triangle meshes (include/nsdp_geodesic.h): the edge table of a pose in one
// launch, and the relaxation to the fixed point a number of rounds per call.
//
// nsdp_mesh_edge_lengths
//   edges    one lane per position e of the corner lists and pose: the corner's face, its three rows (mesh_corners.h, a search
//            per lane: neighbouring positions name unrelated faces), two 12-byte gathers beside the row's own point, two
//            lengths; one 8-byte store into len, and into nbr for pose 0.
// nsdp_mesh_geodesic_relax
//   zero     changed_out = 0 (a kernel, so that a captured call is kernel nodes alone);
//   relax    once per round.  A workgroup of 256 threads owns kBlock = 256 consecutive vertex rows of one pose, a thread one of
//            them (kBlock / 256 in general: row0 + i * 256 + tid, coalesced).  It sanitises their distances into LDS, relaxes every row ONCE against
//            its out-of-block neighbours -- relaxed atomic loads of what other workgroups hold, a stale value is a valid upper
//            bound -- and then repeats passes over the in-block neighbours out of LDS until a workgroup vote sees no change
//            (or kBlock passes, the cap).  A row with up to kLaneMax list positions is walked by its lane, a longer one by its
//            wave (a minimum needs no order).  The in-block pairs (slot, length) of a row with up to kCached = 8 list positions
//            stay in the lane's registers, so a pass is LDS reads and additions; longer lists are streamed from L2 on every
//            pass.  LDS holds the block's distances alone.  A block whose rows and out-of-block neighbours are
//            all +inf changes nothing in its first pass and leaves.  Rows whose bits differ from what came in are stored;
//            the last round adds the rows it lowered to changed_out (one integer atomic per workgroup).
// Distances are handled as their bits (uint32): non-negative floats order as their bits do, and whatever exceeds the limit's
// bits -- negatives, NaN -- is +inf.  Built with -ffp-contract=off: one rounding per operation, sqrtf is the correctly rounded one.
#include "../../include/nsdp_geodesic.h"

#include <cstring>

#include "common.h"
#include "mesh_corners.h"
#include "prof.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kBlock = NSDP_GEODESIC_BLOCK;      // vertex rows of a workgroup
constexpr int kRows = kBlock / kThreads;         // ... of a thread
constexpr int kLaneMax = 32;                     // the longest list (in corner positions) one lane walks alone
constexpr int kCached = 8;                       // ... whose in-block entries a lane keeps in registers (a mesh vertex has ~6)
constexpr int kMaxRows = 1 << 20;                // nsdp_mesh_corner_lists's limits
constexpr int kMaxCorners = 1 << 25;
constexpr int kMaxPoses = 65535;
constexpr uint32_t kInf = 0x7f800000u;
static_assert(kBlock % kThreads == 0 && kRows >= 1, "a thread owns whole rows");

inline bool aligned_to(const void *p, size_t to) { return reinterpret_cast<uintptr_t>(p) % to == 0; }

__global__ __launch_bounds__(kThreads) void mesh_edge_lengths_kernel(const Mesh m, const float *__restrict__ verts_all,
                                                                     const int32_t *__restrict__ list_offsets,
                                                                     const int32_t *__restrict__ list_entries,
                                                                     int32_t *__restrict__ nbr, float *__restrict__ len_all) {
  const int E = 3 * m.fcap;
  const long long e = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x;
  if (e >= E) return;
  const size_t p = blockIdx.y;
  const float *verts = verts_all + p * m.vcap * 3;
  int n1 = 0, n2 = 0;
  float l1 = 0.f, l2 = 0.f;
  int rows[3];
  const int c = clamped(list_entries[e], 0, E - 1), q = c / 3, j = c - 3 * q;
  if (e < clamped(list_offsets[m.vcap], 0, E) && corner_rows_any(m, q, rows)) {
    n1 = rows[j == 2 ? 0 : j + 1];
    n2 = rows[j == 0 ? 2 : j - 1];
    const float *a = verts + static_cast<size_t>(rows[j]) * 3, *b = verts + static_cast<size_t>(n1) * 3,
                *d = verts + static_cast<size_t>(n2) * 3;
    l1 = __builtin_sqrtf(nsdp::sq_dist3(a[0], a[1], a[2], b[0], b[1], b[2]));
    l2 = __builtin_sqrtf(nsdp::sq_dist3(a[0], a[1], a[2], d[0], d[1], d[2]));
  }
  if (nbr && p == 0) *reinterpret_cast<int2 *>(nbr + 2 * e) = make_int2(n1, n2);
  *reinterpret_cast<float2 *>(len_all + p * (2 * static_cast<size_t>(E)) + 2 * e) = make_float2(l1, l2);
}

__global__ void geodesic_zero_kernel(int32_t *__restrict__ changed_out) { *changed_out = 0; }

struct Relax {
  const int32_t *list_offsets, *nbr;
  const float *len;      // of this pose
  uint32_t *dist;        // of this pose
  int vcap, E;           // E = 3 fcap corner positions, 2 E table entries
  uint32_t limit;
};

__device__ __forceinline__ uint32_t sanitised(uint32_t bits, uint32_t limit) { return bits <= limit ? bits : kInf; }

// the smallest S(fl(D[u] + w)) over list positions lo + first, lo + first + stride, ... below hi; kOutside: over the entries
// whose row lies outside the block [row0, row0 + kBlock), read from memory -- otherwise over those inside it, read from LDS
template <bool kOutside>
__device__ __forceinline__ uint32_t best_of(const Relax &g, const uint32_t *block, int row0, int lo, int hi, int first, int stride) {
  uint32_t best = kInf;
  for (int e = lo + first; e < hi; e += stride) {
    const int2 u2 = *reinterpret_cast<const int2 *>(g.nbr + 2 * static_cast<size_t>(e));
    const float2 w2 = *reinterpret_cast<const float2 *>(g.len + 2 * static_cast<size_t>(e));
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int u = clamped(k ? u2.y : u2.x, 0, g.vcap - 1);
      const float w = k ? w2.y : w2.x;
      const bool inside = static_cast<unsigned>(u - row0) < static_cast<unsigned>(kBlock);
      if (inside == kOutside) continue;
      uint32_t du;
      if (kOutside)
        du = sanitised(__hip_atomic_load(g.dist + u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), g.limit);
      else
        du = __hip_atomic_load(block + (u - row0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (du == kInf) continue;
      const uint32_t cand = __float_as_uint(__fadd_rn(__uint_as_float(du), w));
      if (cand <= g.limit && cand < best) best = cand;
    }
  }
  return best;
}

// the in-block entries of a row with up to kCached list positions, kept in registers for the passes over LDS: the slot of the
// neighbour in the block, -1 for an entry outside it or beyond the list
struct Cached {
  int u[2 * kCached];
  float w[2 * kCached];
};

__device__ __forceinline__ void load_cached(const Relax &g, int row0, int lo, int hi, Cached &c) {
#pragma unroll
  for (int j = 0; j < kCached; ++j) {
    int2 u2 = make_int2(-1, -1);
    float2 w2 = make_float2(0.f, 0.f);
    if (lo + j < hi && hi - lo <= kCached) {
      u2 = *reinterpret_cast<const int2 *>(g.nbr + 2 * static_cast<size_t>(lo + j));
      w2 = *reinterpret_cast<const float2 *>(g.len + 2 * static_cast<size_t>(lo + j));
      u2.x = clamped(u2.x, 0, g.vcap - 1) - row0;
      u2.y = clamped(u2.y, 0, g.vcap - 1) - row0;
      if (static_cast<unsigned>(u2.x) >= static_cast<unsigned>(kBlock)) u2.x = -1;
      if (static_cast<unsigned>(u2.y) >= static_cast<unsigned>(kBlock)) u2.y = -1;
    }
    c.u[2 * j] = u2.x, c.u[2 * j + 1] = u2.y;
    c.w[2 * j] = w2.x, c.w[2 * j + 1] = w2.y;
  }
}

__device__ __forceinline__ uint32_t best_cached(const Cached &c, const uint32_t *block, uint32_t limit) {
  uint32_t best = kInf;
#pragma unroll
  for (int t = 0; t < 2 * kCached; ++t) {
    if (c.u[t] < 0) continue;
    const uint32_t du = __hip_atomic_load(block + c.u[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (du == kInf) continue;
    const uint32_t cand = __float_as_uint(__fadd_rn(__uint_as_float(du), c.w[t]));
    if (cand <= limit && cand < best) best = cand;
  }
  return best;
}

__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) v = min(v, static_cast<uint32_t>(__shfl_xor(static_cast<int>(v), s)));
  return v;
}

// one pass over the workgroup's rows: every row's candidate minimum (a lane up to kLaneMax positions, the wave beyond) -> best[]
template <bool kOutside>
__device__ __forceinline__ void pass(const Relax &g, const uint32_t *block, int row0, const int (&lo)[kRows], const int (&hi)[kRows],
                                     const Cached (&cache)[kRows], uint32_t (&best)[kRows]) {
  const int lane = static_cast<int>(threadIdx.x) & 63;
#pragma unroll
  for (int i = 0; i < kRows; ++i) {
    const int n = hi[i] - lo[i];
    if (!kOutside && n <= kCached)
      best[i] = best_cached(cache[i], block, g.limit);
    else
      best[i] = n <= kLaneMax ? best_of<kOutside>(g, block, row0, lo[i], hi[i], 0, 1) : kInf;
    unsigned long long todo = __ballot(n > kLaneMax);      // (all 64 lanes are here: a lane without a row has n == 0)
    while (todo) {
      const int src = __ffsll(static_cast<long long>(todo)) - 1;
      todo &= todo - 1;
      const uint32_t got = wave_min(best_of<kOutside>(g, block, row0, __shfl(lo[i], src), __shfl(hi[i], src), lane, 64));
      if (lane == src) best[i] = got;
    }
  }
}

__global__ __launch_bounds__(kThreads) void geodesic_relax_kernel(const int32_t *__restrict__ list_offsets,
                                                                  const int32_t *__restrict__ nbr, const float *__restrict__ len_all,
                                                                  const int32_t *__restrict__ vert_offsets, int B, int vcap, int fcap,
                                                                  uint32_t limit, int passes, uint32_t *dist_all,
                                                                  int32_t *__restrict__ changed_out) {
  __shared__ uint32_t block[kBlock];
  __shared__ int lowered_rows;
  const int tid = static_cast<int>(threadIdx.x);
  const size_t p = blockIdx.y;
  const int row0 = static_cast<int>(blockIdx.x) * kBlock;
  const int E = 3 * fcap;
  const int live = clamped(vert_offsets[B], 0, vcap);
  const Relax g{list_offsets, nbr, len_all + p * (2 * static_cast<size_t>(E)), dist_all + p * vcap, vcap, E, limit};

  uint32_t raw[kRows], start[kRows], mine[kRows], best[kRows];
  int lo[kRows], hi[kRows];
  Cached cache[kRows];
  if (tid == 0) lowered_rows = 0;
#pragma unroll
  for (int i = 0; i < kRows; ++i) {
    const int r = row0 + i * kThreads + tid;
    raw[i] = start[i] = kInf;
    lo[i] = hi[i] = 0;
    if (r < vcap) {
      raw[i] = g.dist[r];
      if (r < live) {
        start[i] = sanitised(raw[i], limit);
        lo[i] = clamped(list_offsets[r], 0, E);
        hi[i] = clamped(list_offsets[r + 1], lo[i], E);
      }
    }
    mine[i] = start[i];
    load_cached(g, row0, lo[i], hi[i], cache[i]);
  }
  // the out-of-block neighbours, once: what other workgroups held when this one looked
  pass<true>(g, block, row0, lo, hi, cache, best);
#pragma unroll
  for (int i = 0; i < kRows; ++i) {
    mine[i] = min(mine[i], best[i]);
    block[i * kThreads + tid] = mine[i];
  }
  __syncthreads();
  // the in-block neighbours out of LDS, until nothing falls (reads race with the stores of the same pass: either value is an
  // upper bound of the fixed point, and a pass that stores nothing has read the final values)
  for (int it = 0; it < passes; ++it) {
    pass<false>(g, block, row0, lo, hi, cache, best);
    int fell = 0;
#pragma unroll
    for (int i = 0; i < kRows; ++i) {
      if (best[i] < mine[i]) {
        mine[i] = best[i];
        __hip_atomic_store(block + i * kThreads + tid, mine[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        fell = 1;
      }
    }
    if (!__syncthreads_or(fell)) break;
  }
  int lowered = 0;
#pragma unroll
  for (int i = 0; i < kRows; ++i) {
    const int r = row0 + i * kThreads + tid;
    if (r < vcap && mine[i] != raw[i]) __hip_atomic_store(g.dist + r, mine[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    lowered += mine[i] < start[i];
  }
  if (changed_out) {      // (uniform: a kernel argument)
    if (lowered) atomicAdd(&lowered_rows, lowered);
    __syncthreads();
    if (tid == 0 && lowered_rows) atomicAdd(changed_out, lowered_rows);
  }
}

bool sizes_refused(int B, int vcap, int fcap) {
  return B < 1 || B > 65535 || vcap < 1 || vcap > kMaxRows || fcap < 1 || fcap > kMaxCorners / 3;
}

}  // namespace

#define GEODESIC_SIZES(who)                                                                                                        \
  NSDP_REQUIRE(P >= 1 && P <= kMaxPoses, who ": P=%d poses outside [1, %d]", P, kMaxPoses);                                        \
  NSDP_REQUIRE(B >= 1 && B <= 65535, who ": batch B=%d outside [1, 65535]", B);                                                    \
  NSDP_REQUIRE(vcap >= 1 && vcap <= kMaxRows, who ": vcap=%d vertex rows outside [1, %d]", vcap, kMaxRows);                        \
  NSDP_REQUIRE(fcap >= 1 && fcap <= kMaxCorners / 3, who ": fcap=%d face rows outside [1, %d] (3 fcap corners <= %d)", fcap,       \
               kMaxCorners / 3, kMaxCorners)

extern "C" size_t nsdp_mesh_edge_table_entries(int B, int vcap, int fcap) {
  return sizes_refused(B, vcap, fcap) ? 0 : static_cast<size_t>(6) * fcap;
}

extern "C" int nsdp_mesh_geodesic_block(void) { return kBlock; }

extern "C" int nsdp_mesh_edge_lengths(const float *verts, int P, const int32_t *faces, const int32_t *face_offsets,
                                      const int32_t *vert_offsets, int B, int vcap, int fcap, const int32_t *list_offsets,
                                      const int32_t *list_entries, int32_t *nbr, float *len, void *stream) {
  GEODESIC_SIZES("mesh_edge_lengths");
  NSDP_REQUIRE(verts && faces && face_offsets && vert_offsets, "mesh_edge_lengths: null pointer (verts / faces / offsets)");
  NSDP_REQUIRE(list_offsets && list_entries, "mesh_edge_lengths: null pointer (lists)");
  NSDP_REQUIRE(len, "mesh_edge_lengths: null pointer (len)");
  NSDP_REQUIRE(aligned_to(verts, 4) && aligned_to(faces, 4) && aligned_to(face_offsets, 4) && aligned_to(vert_offsets, 4) &&
                   aligned_to(list_offsets, 4) && aligned_to(list_entries, 4),
               "mesh_edge_lengths: an index or fp32 operand is not 4-byte aligned");
  NSDP_REQUIRE(aligned_to(nbr, 8) && aligned_to(len, 8), "mesh_edge_lengths: nbr / len are not 8-byte aligned (pairs)");
  const Mesh m{faces, face_offsets, vert_offsets, B, vcap, fcap};
  NSDP_TRACE("mesh_edge_lengths<P=%d,B=%d,vcap=%d,fcap=%d>", P, B, vcap, fcap);
  hipLaunchKernelGGL(mesh_edge_lengths_kernel, dim3(nsdp::ceil_div(3LL * fcap, kThreads), P), dim3(kThreads), 0,
                     nsdp::as_stream(stream), m, verts, list_offsets, list_entries, nbr, len);
  return nsdp::launch_status("mesh_edge_lengths_kernel");
}

extern "C" int nsdp_mesh_geodesic_relax(const int32_t *list_offsets, const int32_t *nbr, const float *len, const int32_t *vert_offsets,
                                        int B, int vcap, int fcap, int P, float limit, int rounds, int flags, float *dist,
                                        int32_t *changed_out, void *stream) {
  GEODESIC_SIZES("mesh_geodesic_relax");
  NSDP_REQUIRE(limit == limit && !std::signbit(limit), "mesh_geodesic_relax: limit=%g is NaN or negative (limit >= +0, +inf allowed)",
               static_cast<double>(limit));
  NSDP_REQUIRE(rounds >= 1 && rounds <= NSDP_GEODESIC_MAX_ROUNDS, "mesh_geodesic_relax: rounds=%d outside [1, %d]", rounds,
               NSDP_GEODESIC_MAX_ROUNDS);
  NSDP_REQUIRE((flags & ~NSDP_GEODESIC_NO_LOCAL) == 0, "mesh_geodesic_relax: flags=%d has unknown bits (NSDP_GEODESIC_NO_LOCAL = 1)",
               flags);
  NSDP_REQUIRE(list_offsets && nbr && len && vert_offsets, "mesh_geodesic_relax: null pointer (lists / table / offsets)");
  NSDP_REQUIRE(dist && changed_out, "mesh_geodesic_relax: null pointer (dist / changed_out)");
  NSDP_REQUIRE(aligned_to(list_offsets, 4) && aligned_to(vert_offsets, 4) && aligned_to(dist, 4) && aligned_to(changed_out, 4),
               "mesh_geodesic_relax: an index or fp32 operand is not 4-byte aligned");
  NSDP_REQUIRE(aligned_to(nbr, 8) && aligned_to(len, 8), "mesh_geodesic_relax: nbr / len are not 8-byte aligned (pairs)");
  hipStream_t st = nsdp::as_stream(stream);
  uint32_t limit_bits;
  memcpy(&limit_bits, &limit, sizeof limit_bits);
  const int passes = (flags & NSDP_GEODESIC_NO_LOCAL) ? 1 : kBlock;
  NSDP_TRACE("mesh_geodesic_relax<P=%d,B=%d,vcap=%d,fcap=%d,rounds=%d,flags=%d>", P, B, vcap, fcap, rounds, flags);
  hipLaunchKernelGGL(geodesic_zero_kernel, dim3(1), dim3(1), 0, st, changed_out);
  if (const int rc = nsdp::launch_status("geodesic_zero_kernel")) return rc;
  const dim3 grid(nsdp::ceil_div(vcap, kBlock), P);
  for (int r = 0; r < rounds; ++r) {
    hipLaunchKernelGGL(geodesic_relax_kernel, grid, dim3(kThreads), 0, st, list_offsets, nbr, len, vert_offsets, B, vcap, fcap,
                       limit_bits, passes, reinterpret_cast<uint32_t *>(dist), r == rounds - 1 ? changed_out : nullptr);
    if (const int rc = nsdp::launch_status("geodesic_relax_kernel")) return rc;
  }
  return 0;
}
