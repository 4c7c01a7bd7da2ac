// Exact point-to-mesh distance (include/nsdp_surface.h): for every query the closest point of a triangle mesh.
//
//   boxes_kernel    (mesh_blocks.h, shared with ray_cast.hip) one wave per block of 64 consecutive faces of a mesh: the bounding
//                   box of the block's corners -> workspace
//   init_kernel     one lane per query: its start key -- (FLT_MAX, no face), or with the bound pass the smallest over its mesh's blocks
//                   of the largest squared distance to a box, raised by the margin and one ulp (some whole face lies in each box)
//   scan_kernel     one wave per 64 queries of a mesh and per part of the mesh's blocks: a wave-wide vote on box distance
//                   against the lanes' best, the block's corners staged once in LDS, every lane tests all of the block's faces;
//                   one 64-bit integer atomic minimum per lane at the end
//   finish_kernel   one lane per query: key -> dist2, face; the barycentric coordinates recomputed for the winning face
//
// Built with -ffp-contract=off: every operation below rounds once, in the order the header documents.
#include <cfloat>
#include <climits>

#include "../../include/nsdp_surface.h"
#include "common.h"
#include "mesh_blocks.h"
#include "prof.h"
#include "ragged.h"

namespace {

constexpr int kRec = 9;                         // a staged face: 9 dwords (a, b, c) -- an odd stride, see scan_kernel
constexpr float kMargin = 1.9073486328125e-06f; // 2^-19 = 32 * 2^-24: 17 (the envelope) + 5 (a box distance) + 2 (the margin's own
                                                // product and subtraction), the rest slack for second order -- DESIGN.md 4k
constexpr unsigned long long kNoFace = 0xFFFFFFFFull;
constexpr unsigned long long kStartKey = (0x7F7FFFFFull << 32) | kNoFace;      // (FLT_MAX bits, no face)

__device__ __forceinline__ V3 sub(const V3 &a, const V3 &b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ float dot(const V3 &a, const V3 &b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ V3 axpy(const V3 &p, float t, const V3 &e) { return {p.x + t * e.x, p.y + t * e.y, p.z + t * e.z}; }

// the closest point of segment P + t e (0 <= t <= 1) to the origin: its parameter and squared distance
__device__ __forceinline__ float edge(const V3 &P, const V3 &e, float &t) {
  const float ee = dot(e, e), tn = -dot(P, e);
  t = (ee == 0.f || tn <= 0.f) ? 0.f : (tn >= ee ? 1.f : tn / ee);
  const V3 X = axpy(P, t, e);
  return dot(X, X);
}

// The squared distance from the origin to triangle (A, B, C) -- corners already in the query's frame; kBary: the barycentric
// coordinates of the closest point too.  The one definition both the scan and the finishing pass use: the same bits.
template <bool kBary>
__device__ __forceinline__ float closest(const V3 &A, const V3 &B, const V3 &C, float *bary) {
  const V3 ab = sub(B, A), ac = sub(C, A), bc = sub(C, B);
  float t, s;
  float best = edge(A, ab, t);
  int which = 0;
  float d = edge(A, ac, s);
  if (d < best) best = d, which = 1, t = s;
  d = edge(B, bc, s);
  if (d < best) best = d, which = 2, t = s;
  const float g11 = dot(ab, ab), g12 = dot(ab, ac), g22 = dot(ac, ac), r1 = -dot(A, ab), r2 = -dot(A, ac);
  const float det = g11 * g22 - g12 * g12, v = g22 * r1 - g12 * r2, w = g11 * r2 - g12 * r1;
  float b1 = 0.f, b2 = 0.f;
  // (a degenerate face fails the first test: det is at most rounding noise of g11 g22, and 0 > 0 is false where both vanish)
  if (det > 9.5367431640625e-07f * (g11 * g22) && v > 0.f && w > 0.f && v + w < det) {
    b1 = v / det, b2 = w / det;
    const V3 X = axpy(axpy(A, b1, ab), b2, ac);
    d = dot(X, X);
    if (d < best) best = d, which = 3;
  }
  if (kBary) {
    const float u = 1.f - t;
    if (which == 0) bary[0] = u, bary[1] = t, bary[2] = 0.f;
    else if (which == 1) bary[0] = u, bary[1] = 0.f, bary[2] = t;
    else if (which == 2) bary[0] = 0.f, bary[1] = u, bary[2] = t;
    else bary[0] = fmaxf(0.f, (1.f - b1) - b2), bary[1] = b1, bary[2] = b2;
  }
  return best;
}

// the smallest (lo2) and largest (hi2) squared distance from p to the box [lo, hi], as computed: each within 5 * 2^-24 of itself
__device__ __forceinline__ void box_dist(const V3 &p, const float *__restrict__ box, float &lo2, float &hi2) {
  const float ax = box[0] - p.x, bx = p.x - box[3], ay = box[1] - p.y, by = p.y - box[4], az = box[2] - p.z, bz = p.z - box[5];
  const V3 n = {fmaxf(fmaxf(ax, bx), 0.f), fmaxf(fmaxf(ay, by), 0.f), fmaxf(fmaxf(az, bz), 0.f)};
  const V3 f = {fmaxf(-ax, -bx), fmaxf(-ay, -by), fmaxf(-az, -bz)};
  lo2 = dot(n, n);
  hi2 = dot(f, f);
}

__global__ __launch_bounds__(kWave) void init_kernel(const float *__restrict__ query, const int32_t *__restrict__ query_offsets,
                                                     const int32_t *__restrict__ vert_offsets,
                                                     const int32_t *__restrict__ face_offsets, int B, int qcap, int vcap, int fcap,
                                                     int bound_pass, const float *__restrict__ boxes,
                                                     unsigned long long *__restrict__ keys) {
  int b, row0, end;
  if (!nsdp::ragged_tile<kWave>(query_offsets, B, qcap, static_cast<int>(blockIdx.x), b, row0, end)) return;
  const int row = row0 + static_cast<int>(threadIdx.x);
  if (row >= end) return;
  unsigned long long key = kStartKey;
  if (bound_pass) {
    const Mesh m = mesh_of(vert_offsets, face_offsets, b, vcap, fcap);
    const int nb = (m.fhi - m.flo + kBlock - 1) / kBlock;
    const V3 p = {query[static_cast<size_t>(row) * 3], query[static_cast<size_t>(row) * 3 + 1], query[static_cast<size_t>(row) * 3 + 2]};
    float bound = FLT_MAX;
    for (int j = 0; j < nb; ++j) {
      float lo2, hi2;
      box_dist(p, boxes + static_cast<size_t>(m.slot0 + j) * 6, lo2, hi2);
      bound = fminf(bound, hi2);
    }
    // raised by the margin, then one ulp up (the sum's own rounding); never beyond FLT_MAX
    const float raised = fminf(bound + kMargin * bound, FLT_MAX);
    const unsigned bits = min(__float_as_uint(raised) + 1u, 0x7F7FFFFFu);
    key = (static_cast<unsigned long long>(bits) << 32) | kNoFace;
  }
  keys[row] = key;
}

__global__ __launch_bounds__(kWave) void scan_kernel(const float *__restrict__ query, const int32_t *__restrict__ query_offsets,
                                                     const float *__restrict__ verts, const int32_t *__restrict__ vert_offsets,
                                                     const int32_t *__restrict__ faces, const int32_t *__restrict__ face_offsets,
                                                     int B, int qcap, int vcap, int fcap, int cull, const float *__restrict__ boxes,
                                                     unsigned long long *__restrict__ keys) {
  // a face is a record of 9 dwords: lane i writes dwords 9 i .. 9 i + 8 one ds_write_b32 at a time -- the stride is odd, so the 32
  // lanes of a write group fall on 32 different banks; every read is wave-uniform (one address, a broadcast)
  __shared__ float rec[kBlock * kRec];
  int b, row0, end;
  if (!nsdp::ragged_tile<kWave>(query_offsets, B, qcap, static_cast<int>(blockIdx.x), b, row0, end)) return;
  const Mesh m = mesh_of(vert_offsets, face_offsets, b, vcap, fcap);
  const long long nb = (m.fhi - m.flo + kBlock - 1) / kBlock;
  const int j0 = static_cast<int>(nb * blockIdx.y / gridDim.y), j1 = static_cast<int>(nb * (blockIdx.y + 1) / gridDim.y);
  if (j0 >= j1) return;
  const int lane = static_cast<int>(threadIdx.x);
  const bool live = row0 + lane < end;
  const int row = min(row0 + lane, end - 1);
  const V3 p = {query[static_cast<size_t>(row) * 3], query[static_cast<size_t>(row) * 3 + 1], query[static_cast<size_t>(row) * 3 + 2]};
  const unsigned long long start = keys[row];
  unsigned long long best = start;
  for (int j = j0; j < j1; ++j) {
    if (cull) {
      float lo2, hi2;
      box_dist(p, boxes + static_cast<size_t>(m.slot0 + j) * 6, lo2, hi2);
      // skipped only where lo2 - margin * hi2 exceeds every live lane's best: no face of the block can reach it
      const bool want = live && !(lo2 - kMargin * hi2 > __uint_as_float(static_cast<unsigned>(best >> 32)));
      if (!__any(want)) continue;
    }
    const int f0 = m.flo + j * kBlock, cnt = min(kBlock, m.fhi - f0);
    __syncthreads();                                           // (the previous block's records have been read)
    if (lane < cnt) {
      const size_t fr = static_cast<size_t>(f0 + lane) * 3;
      const V3 a = corner(verts, m, faces[fr]), c1 = corner(verts, m, faces[fr + 1]), c2 = corner(verts, m, faces[fr + 2]);
      float *r = rec + lane * kRec;
      r[0] = a.x, r[1] = a.y, r[2] = a.z, r[3] = c1.x, r[4] = c1.y, r[5] = c1.z, r[6] = c2.x, r[7] = c2.y, r[8] = c2.z;
    }
    __syncthreads();
    for (int f = 0; f < cnt; ++f) {
      const float *r = rec + f * kRec;
      const V3 A = {r[0] - p.x, r[1] - p.y, r[2] - p.z}, Bc = {r[3] - p.x, r[4] - p.y, r[5] - p.z},
               C = {r[6] - p.x, r[7] - p.y, r[8] - p.z};
      const float d = closest<false>(A, Bc, C, nullptr);
      const unsigned long long key = (static_cast<unsigned long long>(__float_as_uint(d)) << 32) | static_cast<unsigned>(f0 + f);
      best = key < best ? key : best;
    }
  }
  if (live && best < start) atomicMin(keys + row, best);
}

__global__ __launch_bounds__(kWave) void finish_kernel(const float *__restrict__ query, const int32_t *__restrict__ query_offsets,
                                                       const float *__restrict__ verts, const int32_t *__restrict__ vert_offsets,
                                                       const int32_t *__restrict__ faces, const int32_t *__restrict__ face_offsets,
                                                       int B, int qcap, int vcap, int fcap,
                                                       const unsigned long long *__restrict__ keys, float *__restrict__ dist2_out,
                                                       int32_t *__restrict__ face_out, float *__restrict__ bary_out) {
  int b, row0, end;
  if (!nsdp::ragged_tile<kWave>(query_offsets, B, qcap, static_cast<int>(blockIdx.x), b, row0, end)) return;
  const int row = row0 + static_cast<int>(threadIdx.x);
  if (row >= end) return;
  const unsigned long long key = keys[row];
  const unsigned low = static_cast<unsigned>(key & kNoFace);
  const Mesh m = mesh_of(vert_offsets, face_offsets, b, vcap, fcap);
  float bary[3] = {0.f, 0.f, 0.f};
  // (a key no face improved -- a mesh without faces -- or a row outside the mesh: FLT_MAX, -1, 0)
  const bool found = low != kNoFace && static_cast<int>(low) >= m.flo && static_cast<int>(low) < m.fhi;
  if (found && bary_out) {
    const size_t fr = static_cast<size_t>(low) * 3, q = static_cast<size_t>(row) * 3;
    const V3 p = {query[q], query[q + 1], query[q + 2]};
    const V3 a = corner(verts, m, faces[fr]), c1 = corner(verts, m, faces[fr + 1]), c2 = corner(verts, m, faces[fr + 2]);
    closest<true>(sub(a, p), sub(c1, p), sub(c2, p), bary);
  }
  dist2_out[row] = found ? __uint_as_float(static_cast<unsigned>(key >> 32)) : FLT_MAX;
  face_out[row] = found ? static_cast<int32_t>(low) : -1;
  if (bary_out) {
    float *o = bary_out + static_cast<size_t>(row) * 3;
    o[0] = bary[0], o[1] = bary[1], o[2] = bary[2];
  }
}

bool sizes_ok(int B, int qcap, int fcap) {
  return B >= 1 && B <= 65535 && qcap >= 1 && fcap >= 1 && qcap <= static_cast<long long>(kMaxRows) * B &&
         fcap <= static_cast<long long>(kMaxRows) * B;
}

}  // namespace

extern "C" size_t nsdp_mesh_closest_workspace_bytes(int B, int qcap, int fcap) {
  if (!sizes_ok(B, qcap, fcap)) return 0;
  return static_cast<size_t>(8) * qcap + static_cast<size_t>(24) * box_slots(B, fcap);
}

extern "C" int nsdp_mesh_closest(const float *query, const int32_t *query_offsets, const float *verts, const int32_t *vert_offsets,
                                 const int32_t *faces, const int32_t *face_offsets, int B, int qcap, int vcap, int fcap, int flags,
                                 void *workspace, float *dist2_out, int32_t *face_out, float *bary_out, void *stream) {
  NSDP_REQUIRE(B >= 1 && B <= 65535, "mesh_closest: batch B=%d outside 1 .. 65535", B);
  const long long most = static_cast<long long>(kMaxRows) * B;
  NSDP_REQUIRE(qcap >= 1 && qcap <= most, "mesh_closest: qcap=%d outside 1 .. 2^20 rows per shape (B=%d)", qcap, B);
  NSDP_REQUIRE(vcap >= 1 && vcap <= most, "mesh_closest: vcap=%d outside 1 .. 2^20 rows per shape (B=%d)", vcap, B);
  NSDP_REQUIRE(fcap >= 1 && fcap <= most, "mesh_closest: fcap=%d outside 1 .. 2^20 rows per shape (B=%d)", fcap, B);
  NSDP_REQUIRE((flags & ~(NSDP_SURFACE_NO_CULL | NSDP_SURFACE_NO_BOUND)) == 0,
               "mesh_closest: unknown flags=%d (bit 0: no culling, bit 1: no bound pass)", flags);
  NSDP_REQUIRE(query && query_offsets && verts && vert_offsets && faces && face_offsets && workspace && dist2_out && face_out,
               "mesh_closest: null pointer");
  NSDP_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 8 == 0, "mesh_closest: the workspace must be 8-byte aligned");
  hipStream_t st = nsdp::as_stream(stream);
  nsdp::prof::Scope scope(nsdp::prof::kKnn, st, 0.0, 12.0 * (static_cast<double>(qcap) + vcap + fcap) + 20.0 * qcap);
  const int cull = (flags & NSDP_SURFACE_NO_CULL) ? 0 : 1;
  unsigned long long *keys = static_cast<unsigned long long *>(workspace);
  float *boxes = reinterpret_cast<float *>(keys + qcap);
  // the host knows the capacities alone: the grids are sized for them, workgroups without rows return
  const unsigned qt = static_cast<unsigned>(nsdp::ragged_max_tiles(qcap, B, kWave));
  const unsigned ft = static_cast<unsigned>(nsdp::ragged_max_tiles(fcap, B, kBlock));
  // parts of a mesh's blocks: until the grid holds sixteen waves per compute unit (a shape may own every face: cut for that)
  long long parts = (16LL * nsdp::num_cus() + qt - 1) / qt;
  if (parts > ft) parts = ft;
  if (parts > 1024) parts = 1024;
  if (parts < 1) parts = 1;
  NSDP_TRACE("mesh_closest<cull=%d,parts=%d>", cull, static_cast<int>(parts));
  if (cull)
    hipLaunchKernelGGL(boxes_kernel, dim3(ft), dim3(kWave), 0, st, verts, vert_offsets, faces, face_offsets, B, vcap, fcap, boxes);
  hipLaunchKernelGGL(init_kernel, dim3(qt), dim3(kWave), 0, st, query, query_offsets, vert_offsets, face_offsets, B, qcap, vcap,
                     fcap, (cull && !(flags & NSDP_SURFACE_NO_BOUND)) ? 1 : 0, boxes, keys);
  hipLaunchKernelGGL(scan_kernel, dim3(qt, static_cast<unsigned>(parts)), dim3(kWave), 0, st, query, query_offsets, verts,
                     vert_offsets, faces, face_offsets, B, qcap, vcap, fcap, cull, boxes, keys);
  hipLaunchKernelGGL(finish_kernel, dim3(qt), dim3(kWave), 0, st, query, query_offsets, verts, vert_offsets, faces, face_offsets, B,
                     qcap, vcap, fcap, keys, dist2_out, face_out, bary_out);
  return nsdp::launch_status("mesh_closest");
}
