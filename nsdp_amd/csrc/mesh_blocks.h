// Packed triangle meshes cut into blocks of 64 consecutive faces: what the scans over block boxes share -- the exact
// point-to-mesh distance (surface_distance.hip, include/nsdp_surface.h) and the ray cast (ray_cast.hip, include/nsdp_raycast.h).
//
//   Mesh / mesh_of   a shape's rows of the packed vertices and faces, clamped as ragged.h clamps them, and the workspace slot of
//                    its first block
//   corner           a vertex of a mesh by its LOCAL index, clamped into the mesh before it forms an address
//   wave_min / max   butterfly reductions over the 64 lanes
//   boxes_kernel     one wave per block of 64 consecutive faces of a mesh: the bounding box of the block's corners -> workspace
//
// One definition, so both files clamp, number their blocks and box them alike.  Everything sits in an unnamed namespace: each
// translation unit that includes this header gets its own boxes_kernel (a __global__ with external linkage would be defined
// twice in the library).  Include it from files built with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ragged.h"

#pragma clang fp contract(off)

namespace {

constexpr int kWave = 64;                       // a workgroup is one wave: 64 queries (or rays), and a block is 64 faces
constexpr int kBlock = 64;
constexpr int kMaxRows = 1 << 20;               // rows of one kind a shape may hold

struct V3 {
  float x, y, z;
};

// A shape's rows of the three packed sets, clamped as ragged.h clamps them; a mesh without vertices has no faces.
struct Mesh {
  int vlo, vn, flo, fhi, slot0;      // slot0: the workspace slot of the mesh's first block -- flo / 64 + b: the blocks of shape s end
                                     // at or before (its last face row) / 64 + s + 1, where those of shape s + 1 begin at the earliest
};

__device__ __forceinline__ Mesh mesh_of(const int32_t *__restrict__ vert_offsets, const int32_t *__restrict__ face_offsets, int b,
                                        int vcap, int fcap) {
  Mesh m;
  int vhi;
  nsdp::ragged_range(vert_offsets, b, vcap, m.vlo, vhi);
  nsdp::ragged_range(face_offsets, b, fcap, m.flo, m.fhi);
  m.vn = vhi - m.vlo;
  if (m.vn <= 0) m.fhi = m.flo;
  m.slot0 = m.flo / kBlock + b;
  return m;
}

__device__ __forceinline__ V3 corner(const float *__restrict__ verts, const Mesh &m, int local) {
  const size_t r = static_cast<size_t>(m.vlo + min(max(local, 0), m.vn - 1)) * 3;
  return {verts[r], verts[r + 1], verts[r + 2]};
}

__device__ __forceinline__ float wave_min(float v) {
  for (int s = 32; s > 0; s >>= 1) v = fminf(v, __shfl_xor(v, s, kWave));
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
  for (int s = 32; s > 0; s >>= 1) v = fmaxf(v, __shfl_xor(v, s, kWave));
  return v;
}

// box slots of a workspace: fcap / 64 + B + 1 (a mesh's blocks start at its first face)
inline long long box_slots(int B, int fcap) { return static_cast<long long>(fcap) / kBlock + B + 1; }

__global__ __launch_bounds__(kWave) void boxes_kernel(const float *__restrict__ verts, const int32_t *__restrict__ vert_offsets,
                                                      const int32_t *__restrict__ faces, const int32_t *__restrict__ face_offsets,
                                                      int B, int vcap, int fcap, float *__restrict__ boxes) {
  int b, row0, end;
  if (!nsdp::ragged_tile<kBlock>(face_offsets, B, fcap, static_cast<int>(blockIdx.x), b, row0, end)) return;
  const Mesh m = mesh_of(vert_offsets, face_offsets, b, vcap, fcap);
  if (m.fhi <= m.flo) return;                                  // (faces over no vertices: the mesh has no blocks)
  const int f = min(row0 + static_cast<int>(threadIdx.x), end - 1);      // (a partial block: the surplus lanes repeat its last face)
  const size_t fr = static_cast<size_t>(f) * 3;
  const V3 a = corner(verts, m, faces[fr]), c1 = corner(verts, m, faces[fr + 1]), c2 = corner(verts, m, faces[fr + 2]);
  const float lx = wave_min(fminf(fminf(a.x, c1.x), c2.x)), ly = wave_min(fminf(fminf(a.y, c1.y), c2.y)),
              lz = wave_min(fminf(fminf(a.z, c1.z), c2.z));
  const float hx = wave_max(fmaxf(fmaxf(a.x, c1.x), c2.x)), hy = wave_max(fmaxf(fmaxf(a.y, c1.y), c2.y)),
              hz = wave_max(fmaxf(fmaxf(a.z, c1.z), c2.z));
  if (threadIdx.x == 0) {
    float *box = boxes + static_cast<size_t>(m.slot0 + (row0 - m.flo) / kBlock) * 6;
    box[0] = lx, box[1] = ly, box[2] = lz, box[3] = hx, box[4] = hy, box[5] = hz;
  }
}

}  // namespace
