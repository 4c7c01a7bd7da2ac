// Per-vertex normals of packed triangle meshes (include/nsdp_meshnormals.h): the corner lists of a topology, once, and the
// area-weighted normals of P poses of it in two launches, no floating-point atomic anywhere.
//
// nsdp_mesh_corner_lists
//   corners  one lane per face row: the packed vertex row each of its three corners names -> a table of 3 fcap global rows in the
//            workspace.  A dead face's corners name row vcap - 1: dead faces are the rows behind face_offsets[B], so their
//            corners are the LARGEST corner numbers and land, ascending, behind the live corners of the last list -- the tail of
//            list_entries;
//   invert   nsdp_knn_invert_wide (invert_wide.hip: zero, count, scan, fill, order, long) over that table as ONE shape of 3 fcap
//            entries and vcap sources -- the code base's one counting sort, its result unique by construction.  It writes
//            list_offsets and list_entries in place;
//   finish   list_offsets[vcap] = 3 face_offsets[B], the number of live corners, and the tail behind it = 0: the dead corners
//            leave the last list.
// nsdp_mesh_vertex_normals
//   faces    one lane per face row and pose: three 12-byte position gathers, 9 subtractions / products per component group, one
//            12-byte store at a 12-byte stride (whole lines per wave).  One owner search per wave (packed_rows.h);
//   vertices one lane per vertex row and pose, 256 rows per workgroup: lists::reduce over the row's corner list with the face's
//            normal as the term (list_reduce.h: a lane up to 32 corners, the wave up to 1024, the workgroup beyond -- a mesh
//            vertex has ~6), then the unit normal.  12 bytes gathered per corner out of face_normals, which the launch in front
//            has just written: L2 hits at session sizes.
// Built with -ffp-contract=off: one rounding per operation, sqrtf and / of a HIP translation unit are the correctly rounded ones.
#include "../../include/nsdp_meshnormals.h"
#include "../../include/nsdp_scatter.h"
#include "common.h"
#include "list_reduce.h"
#include "mesh_corners.h"     // struct Mesh, a corner's row
#include "prof.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = nsdp::lists::kThreads;
constexpr int kMaxRows = 1 << 20;         // nsdp_knn_invert_wide's sources
constexpr int kMaxCorners = 1 << 25;      // ... and entries
constexpr int kMaxPoses = 65535;          // (a grid's y extent)

inline size_t align16(size_t v) { return (v + 15) & ~static_cast<size_t>(15); }
inline bool aligned_to(const void *p, size_t to) { return reinterpret_cast<uintptr_t>(p) % to == 0; }

__global__ __launch_bounds__(kThreads) void mesh_corner_rows_kernel(const Mesh m, int32_t *__restrict__ table) {
  const long long q = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x;
  if (q >= m.fcap) return;
  int rows[3] = {m.vcap - 1, m.vcap - 1, m.vcap - 1};
  corner_rows(m, q, rows);
  int32_t *o = table + static_cast<size_t>(q) * 3;
#pragma unroll
  for (int j = 0; j < 3; ++j) o[j] = rows[j];
}

__global__ __launch_bounds__(kThreads) void mesh_corner_finish_kernel(const Mesh m, int32_t *__restrict__ list_offsets,
                                                                      int32_t *__restrict__ list_entries) {
  const int E = 3 * m.fcap;
  const int live = 3 * clamped(m.face_offsets[m.B], 0, m.fcap);
  const long long i = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x;
  if (i == 0) list_offsets[m.vcap] = live;
  if (i >= live && i < E) list_entries[i] = 0;
}

__global__ __launch_bounds__(kThreads) void mesh_face_normals_kernel(const Mesh m, const float *__restrict__ verts_all,
                                                                     float *__restrict__ face_normals_all) {
  const long long q = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x;
  if (q >= m.fcap) return;
  const size_t p = blockIdx.y;
  const float *verts = verts_all + p * m.vcap * 3;
  float n[3] = {0.f, 0.f, 0.f};
  int rows[3];
  if (corner_rows(m, q, rows)) {
    const float *a = verts + static_cast<size_t>(rows[0]) * 3, *b = verts + static_cast<size_t>(rows[1]) * 3,
                *c = verts + static_cast<size_t>(rows[2]) * 3;
    float e1[3], e2[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      e1[k] = __fsub_rn(b[k], a[k]);
      e2[k] = __fsub_rn(c[k], a[k]);
    }
    n[0] = __fsub_rn(__fmul_rn(e1[1], e2[2]), __fmul_rn(e1[2], e2[1]));
    n[1] = __fsub_rn(__fmul_rn(e1[2], e2[0]), __fmul_rn(e1[0], e2[2]));
    n[2] = __fsub_rn(__fmul_rn(e1[0], e2[1]), __fmul_rn(e1[1], e2[0]));
  }
  float *o = face_normals_all + (p * m.fcap + static_cast<size_t>(q)) * 3;
#pragma unroll
  for (int k = 0; k < 3; ++k) o[k] = n[k];
}

// the term of list_reduce.h: the normal of the face that corner `entries[slot]` belongs to (the row's own point is not used)
struct FaceTerm {
  const int32_t *entries;
  const float *face_normals;
  int corners;
  __device__ __forceinline__ void add(int slot, float, float, float, float &sx, float &sy, float &sz) const {
    const float *n = face_normals + static_cast<size_t>(nsdp::lists::clampi(entries[slot], 0, corners - 1) / 3) * 3;
    sx = __fadd_rn(sx, n[0]);
    sy = __fadd_rn(sy, n[1]);
    sz = __fadd_rn(sz, n[2]);
  }
};

__global__ __launch_bounds__(kThreads) void mesh_vertex_normals_kernel(int vcap, int fcap, const float *__restrict__ verts_all,
                                                                       const int32_t *__restrict__ list_offsets,
                                                                       const int32_t *__restrict__ list_entries,
                                                                       const float *__restrict__ face_normals_all,
                                                                       float *__restrict__ sums_all, float *__restrict__ normals_all) {
  __shared__ nsdp::lists::Shared shared;
  const int E = 3 * fcap;
  const size_t p = blockIdx.y;
  const int row0 = static_cast<int>(blockIdx.x) * kThreads, r = row0 + static_cast<int>(threadIdx.x);
  int lo = 0, hi = 0;
  if (r < vcap) {
    lo = nsdp::lists::clampi(list_offsets[r], 0, E);
    hi = nsdp::lists::clampi(list_offsets[r + 1], lo, E);
  }
  const FaceTerm term{list_entries, face_normals_all + p * fcap * 3, E};
  float sx, sy, sz;
  // (x: what the workgroup form reads a shared row's point from -- any (vcap, 3) table will do, the term ignores the point)
  nsdp::lists::reduce(term, verts_all + p * vcap * 3, list_offsets, E, row0, lo, hi, 0.f, 0.f, 0.f, shared, sx, sy, sz);
  if (r >= vcap) return;
  const float ax = fabsf(sx), ay = fabsf(sy), az = fabsf(sz);
  const bool finite = ax <= FLT_MAX && ay <= FLT_MAX && az <= FLT_MAX;      // (false for a NaN too)
  const float m = fmaxf(fmaxf(ax, ay), az);
  float nx = 0.f, ny = 0.f, nz = 0.f;
  if (finite && m > 0.f) {
    const float tx = sx / m, ty = sy / m, tz = sz / m;
    const float d = __builtin_sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(tx, tx), __fmul_rn(ty, ty)), __fmul_rn(tz, tz)));
    nx = tx / d, ny = ty / d, nz = tz / d;
  }
  const size_t at = (p * vcap + static_cast<size_t>(r)) * 3;
  if (sums_all) sums_all[at] = sx, sums_all[at + 1] = sy, sums_all[at + 2] = sz;
  normals_all[at] = nx, normals_all[at + 1] = ny, normals_all[at + 2] = nz;
}

bool sizes_refused(int B, int vcap, int fcap) {
  return B < 1 || B > 65535 || vcap < 1 || vcap > kMaxRows || fcap < 1 || fcap > kMaxCorners / 3;
}

}  // namespace

#define MESH_SIZES(who)                                                                                                            \
  NSDP_REQUIRE(B >= 1 && B <= 65535, who ": batch B=%d outside [1, 65535]", B);                                                    \
  NSDP_REQUIRE(vcap >= 1 && vcap <= kMaxRows, who ": vcap=%d vertex rows outside [1, %d]", vcap, kMaxRows);                        \
  NSDP_REQUIRE(fcap >= 1 && fcap <= kMaxCorners / 3, who ": fcap=%d face rows outside [1, %d] (3 fcap corners <= %d)", fcap,       \
               kMaxCorners / 3, kMaxCorners)

extern "C" size_t nsdp_mesh_corner_lists_workspace_bytes(int B, int vcap, int fcap) {
  if (sizes_refused(B, vcap, fcap)) return 0;
  return align16(static_cast<size_t>(3) * fcap * sizeof(int32_t)) + nsdp_knn_invert_wide_workspace_bytes(1, 3 * fcap, vcap);
}

extern "C" int nsdp_mesh_corner_lists(const int32_t *faces, const int32_t *face_offsets, const int32_t *vert_offsets, int B, int vcap,
                                      int fcap, void *workspace, int32_t *list_offsets, int32_t *list_entries, void *stream) {
  MESH_SIZES("mesh_corner_lists");
  NSDP_REQUIRE(faces && face_offsets && vert_offsets, "mesh_corner_lists: null pointer (faces / offsets)");
  NSDP_REQUIRE(workspace, "mesh_corner_lists: null pointer (workspace)");
  NSDP_REQUIRE(list_offsets && list_entries, "mesh_corner_lists: null pointer (lists)");
  NSDP_REQUIRE(aligned_to(workspace, 16), "mesh_corner_lists: the workspace is not 16-byte aligned");
  NSDP_REQUIRE(aligned_to(faces, 4) && aligned_to(face_offsets, 4) && aligned_to(vert_offsets, 4) && aligned_to(list_offsets, 4) &&
                   aligned_to(list_entries, 4),
               "mesh_corner_lists: an index operand is not 4-byte aligned");
  const Mesh m{faces, face_offsets, vert_offsets, B, vcap, fcap};
  const int E = 3 * fcap;
  int32_t *table = static_cast<int32_t *>(workspace);
  void *sort_ws = static_cast<char *>(workspace) + align16(static_cast<size_t>(E) * sizeof(int32_t));
  hipStream_t st = nsdp::as_stream(stream);
  NSDP_TRACE("mesh_corner_lists<B=%d,vcap=%d,fcap=%d>", B, vcap, fcap);
  hipLaunchKernelGGL(mesh_corner_rows_kernel, dim3(nsdp::ceil_div(fcap, kThreads)), dim3(kThreads), 0, st, m, table);
  if (const int rc = nsdp::launch_status("mesh_corner_rows_kernel")) return rc;
  if (const int rc = nsdp_knn_invert_wide(table, 1, E, vcap, sort_ws, list_offsets, list_entries, stream)) return rc;
  hipLaunchKernelGGL(mesh_corner_finish_kernel, dim3(nsdp::ceil_div(E, kThreads)), dim3(kThreads), 0, st, m, list_offsets,
                     list_entries);
  return nsdp::launch_status("mesh_corner_finish_kernel");
}

extern "C" int nsdp_mesh_vertex_normals(const float *verts, int P, const int32_t *faces, const int32_t *face_offsets,
                                        const int32_t *vert_offsets, int B, int vcap, int fcap, const int32_t *list_offsets,
                                        const int32_t *list_entries, float *face_normals, float *sums, float *normals, void *stream) {
  NSDP_REQUIRE(P >= 1 && P <= kMaxPoses, "mesh_vertex_normals: P=%d poses outside [1, %d]", P, kMaxPoses);
  MESH_SIZES("mesh_vertex_normals");
  NSDP_REQUIRE(verts && faces && face_offsets && vert_offsets, "mesh_vertex_normals: null pointer (verts / faces / offsets)");
  NSDP_REQUIRE(list_offsets && list_entries, "mesh_vertex_normals: null pointer (lists)");
  NSDP_REQUIRE(face_normals && normals, "mesh_vertex_normals: null pointer (outputs)");
  NSDP_REQUIRE(aligned_to(verts, 4) && aligned_to(faces, 4) && aligned_to(face_offsets, 4) && aligned_to(vert_offsets, 4) &&
                   aligned_to(list_offsets, 4) && aligned_to(list_entries, 4) && aligned_to(face_normals, 4) && aligned_to(sums, 4) &&
                   aligned_to(normals, 4),
               "mesh_vertex_normals: an index or fp32 operand is not 4-byte aligned");
  const Mesh m{faces, face_offsets, vert_offsets, B, vcap, fcap};
  hipStream_t st = nsdp::as_stream(stream);
  NSDP_TRACE("mesh_vertex_normals<P=%d,B=%d,vcap=%d,fcap=%d>", P, B, vcap, fcap);
  hipLaunchKernelGGL(mesh_face_normals_kernel, dim3(nsdp::ceil_div(fcap, kThreads), P), dim3(kThreads), 0, st, m, verts, face_normals);
  if (const int rc = nsdp::launch_status("mesh_face_normals_kernel")) return rc;
  hipLaunchKernelGGL(mesh_vertex_normals_kernel, dim3(nsdp::ceil_div(vcap, kThreads), P), dim3(kThreads), 0, st, vcap, fcap, verts,
                     list_offsets, list_entries, face_normals, sums, normals);
  return nsdp::launch_status("mesh_vertex_normals_kernel");
}
