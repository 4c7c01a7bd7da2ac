// Rays against packed triangle meshes (include/nsdp_raycast.h): for every ray the first face it meets and the
// number of faces it crosses.  A twin of surface_distance.hip's search; the blocks, their boxes and the clamps are mesh_blocks.h's.
//
//   boxes_kernel    (mesh_blocks.h) one wave per block of 64 consecutive faces of a mesh: the bounding box of the block's corners
//   init_kernel     one lane per ray: the start key (FLT_MAX, no face) and a zero count -> workspace
//   scan_kernel     one wave per 64 rays of a mesh and per part of the mesh's blocks: a wave-wide vote on the block box pushed
//                   through the corner's own operations as intervals, the block's corners staged once in LDS, every lane tests all
//                   of the block's faces -- three exact edge signs, and the fp64 depth on the covered ones alone; one 64-bit
//                   integer atomic minimum and one i32 atomic add per lane at the end
//   finish_kernel   one lane per ray: key -> t, face; the barycentric weights recomputed for the winning face; the count
//
// Built with -ffp-contract=off: every operation below rounds once, in the order the header documents.
#include <cfloat>
#include <climits>

#include "../../include/nsdp_raycast.h"
#include "common.h"
#include "mesh_blocks.h"
#include "prof.h"
#include "ragged.h"

#pragma clang fp contract(off)

namespace {

constexpr int kRec = 9;                         // a staged face: 9 dwords (a, b, c) -- an odd stride, see scan_kernel
constexpr unsigned long long kNoFace = 0xFFFFFFFFull;
constexpr unsigned long long kStartKey = (0x7F7FFFFFull << 32) | kNoFace;      // (FLT_MAX bits, no face)

// The ray's frame: the permutation as three selectors and the shear.  ok: the largest |d| is not 0.
struct Frame {
  V3 o;
  float Sx, Sy, Sz;
  int kx, ky, kz;
  bool ok;
};

__device__ __forceinline__ float pick(const V3 &v, int k) { return k == 0 ? v.x : (k == 1 ? v.y : v.z); }

__device__ __forceinline__ Frame frame_of(const V3 &o, const V3 &d) {
  Frame f;
  f.o = o;
  const float ax = fabsf(d.x), ay = fabsf(d.y), az = fabsf(d.z);
  f.kz = (ax >= ay && ax >= az) ? 0 : (ay >= az ? 1 : 2);                // the lowest axis among equal |d|
  f.kx = (f.kz + 1) % 3, f.ky = (f.kz + 2) % 3;
  const float dz = pick(d, f.kz);
  if (dz < 0.f) {
    const int s = f.kx;
    f.kx = f.ky, f.ky = s;
  }
  f.ok = fmaxf(fmaxf(ax, ay), az) != 0.f;
  const float den = f.ok ? dz : 1.f;                                     // (no 0 / 0: a zero ray tests nothing)
  f.Sx = pick(d, f.kx) / den, f.Sy = pick(d, f.ky) / den, f.Sz = 1.f / den;
  return f;
}

// a corner in the ray's frame: the header's four lines
__device__ __forceinline__ V3 shear(const Frame &f, const V3 &c) {
  const V3 C = {c.x - f.o.x, c.y - f.o.y, c.z - f.o.z};
  const float Cz = pick(C, f.kz);
  return {pick(C, f.kx) - f.Sx * Cz, pick(C, f.ky) - f.Sy * Cz, f.Sz * Cz};
}

// the sign of the edge function of the ordered pair (P, Q) for the symbolically displaced ray; l, r: the two exact products
__device__ __forceinline__ int edge_sign(const V3 &P, const V3 &Q, double &l, double &r) {
  l = static_cast<double>(Q.x) * static_cast<double>(P.y);
  r = static_cast<double>(Q.y) * static_cast<double>(P.x);
  if (l != r) return l > r ? 1 : -1;
  if (Q.y != P.y) return Q.y > P.y ? 1 : -1;
  if (P.x != Q.x) return P.x > Q.x ? 1 : -1;
  return 0;
}

// Face (a, b, c), corners already sheared: covered?  hit?  -> t (and the weights with kBary).  The one definition the scan and
// the finishing pass use: the same bits.
template <bool kBary>
__device__ __forceinline__ bool hit_face(const V3 &a, const V3 &b, const V3 &c, float &t, float *bary) {
  double lu, ru, lv, rv, lw, rw;
  const int su = edge_sign(b, c, lu, ru), sv = edge_sign(c, a, lv, rv), sw = edge_sign(a, b, lw, rw);
  if (su == 0 || su != sv || sv != sw) return false;
  const double U = lu - ru, V = lv - rv, W = lw - rw;
  const double det = (U + V) + W;
  const double T = (U * static_cast<double>(a.z) + V * static_cast<double>(b.z)) + W * static_cast<double>(c.z);
  if (!((T > 0.0 && det > 0.0) || (T < 0.0 && det < 0.0))) return false;
  t = static_cast<float>(T / det);
  if (kBary) bary[0] = static_cast<float>(U / det), bary[1] = static_cast<float>(V / det), bary[2] = static_cast<float>(W / det);
  return true;
}

// The block box pushed through shear() as intervals: every operation of shear() is monotone in each operand, so the sheared
// corners of the block lie in [xl, xh] x [yl, yh] x [zl, zh] exactly as computed -- no margin.
__device__ __forceinline__ void shear_box(const Frame &f, const float *__restrict__ box, float &xl, float &xh, float &yl, float &yh,
                                          float &zl, float &zh) {
  const V3 lo = {box[0] - f.o.x, box[1] - f.o.y, box[2] - f.o.z}, hi = {box[3] - f.o.x, box[4] - f.o.y, box[5] - f.o.z};
  const float zlo = pick(lo, f.kz), zhi = pick(hi, f.kz);
  const float px0 = f.Sx * zlo, px1 = f.Sx * zhi, py0 = f.Sy * zlo, py1 = f.Sy * zhi, pz0 = f.Sz * zlo, pz1 = f.Sz * zhi;
  xl = pick(lo, f.kx) - fmaxf(px0, px1), xh = pick(hi, f.kx) - fminf(px0, px1);
  yl = pick(lo, f.ky) - fmaxf(py0, py1), yh = pick(hi, f.ky) - fminf(py0, py1);
  zl = fminf(pz0, pz1), zh = fmaxf(pz0, pz1);
}

__device__ __forceinline__ V3 row3(const float *__restrict__ p, int row) {
  const size_t r = static_cast<size_t>(row) * 3;
  return {p[r], p[r + 1], p[r + 2]};
}

__global__ __launch_bounds__(kWave) void raycast_init_kernel(const int32_t *__restrict__ ray_offsets, int B, int qcap,
                                                             unsigned long long *__restrict__ keys, int32_t *__restrict__ counts) {
  int b, row0, end;
  if (!nsdp::ragged_tile<kWave>(ray_offsets, B, qcap, static_cast<int>(blockIdx.x), b, row0, end)) return;
  const int row = row0 + static_cast<int>(threadIdx.x);
  if (row >= end) return;
  keys[row] = kStartKey;
  counts[row] = 0;
}

// kCount: every block on the ray's line is visited and the hits are counted; without it blocks behind the origin or beyond
// the lane's best t are skipped too
template <bool kCount>
__global__ __launch_bounds__(kWave) void raycast_scan_kernel(const float *__restrict__ origins, const float *__restrict__ dirs,
                                                             const int32_t *__restrict__ ray_offsets, const float *__restrict__ verts,
                                                             const int32_t *__restrict__ vert_offsets,
                                                             const int32_t *__restrict__ faces,
                                                             const int32_t *__restrict__ face_offsets, int B, int qcap, int vcap,
                                                             int fcap, int cull, const float *__restrict__ boxes,
                                                             unsigned long long *__restrict__ keys, int32_t *__restrict__ counts) {
  // a face is a record of 9 dwords: lane i writes dwords 9 i .. 9 i + 8 one ds_write_b32 at a time -- the stride is odd, so the 32
  // lanes of a write group fall on 32 different banks; every read is wave-uniform (one address, a broadcast)
  __shared__ float rec[kBlock * kRec];
  int b, row0, end;
  if (!nsdp::ragged_tile<kWave>(ray_offsets, B, qcap, static_cast<int>(blockIdx.x), b, row0, end)) return;
  const Mesh m = mesh_of(vert_offsets, face_offsets, b, vcap, fcap);
  const long long nb = (m.fhi - m.flo + kBlock - 1) / kBlock;
  const int j0 = static_cast<int>(nb * blockIdx.y / gridDim.y), j1 = static_cast<int>(nb * (blockIdx.y + 1) / gridDim.y);
  if (j0 >= j1) return;
  const int lane = static_cast<int>(threadIdx.x);
  const int row = min(row0 + lane, end - 1);
  const Frame fr = frame_of(row3(origins, row), row3(dirs, row));
  const bool live = row0 + lane < end && fr.ok;
  unsigned long long best = kStartKey;
  int count = 0;
  for (int j = j0; j < j1; ++j) {
    if (cull) {
      float xl, xh, yl, yh, zl, zh;
      shear_box(fr, boxes + static_cast<size_t>(m.slot0 + j) * 6, xl, xh, yl, yh, zl, zh);
      bool want = live && xl <= 0.f && xh >= 0.f && yl <= 0.f && yh >= 0.f;
      if (!kCount) want = want && !(zh < 0.f) && !(zl > __uint_as_float(static_cast<unsigned>(best >> 32)));
      if (!__any(want)) continue;
    }
    const int f0 = m.flo + j * kBlock, cnt = min(kBlock, m.fhi - f0);
    __syncthreads();                                           // (the previous block's records have been read)
    if (lane < cnt) {
      const size_t r3 = static_cast<size_t>(f0 + lane) * 3;
      const V3 a = corner(verts, m, faces[r3]), c1 = corner(verts, m, faces[r3 + 1]), c2 = corner(verts, m, faces[r3 + 2]);
      float *r = rec + lane * kRec;
      r[0] = a.x, r[1] = a.y, r[2] = a.z, r[3] = c1.x, r[4] = c1.y, r[5] = c1.z, r[6] = c2.x, r[7] = c2.y, r[8] = c2.z;
    }
    __syncthreads();
    for (int f = 0; f < cnt; ++f) {
      const float *r = rec + f * kRec;
      const V3 A = shear(fr, {r[0], r[1], r[2]}), Bc = shear(fr, {r[3], r[4], r[5]}), C = shear(fr, {r[6], r[7], r[8]});
      float t;
      if (hit_face<false>(A, Bc, C, t, nullptr) && live) {
        const unsigned long long key = (static_cast<unsigned long long>(__float_as_uint(t)) << 32) | static_cast<unsigned>(f0 + f);
        best = key < best ? key : best;
        ++count;
      }
    }
  }
  if (live && best < kStartKey) atomicMin(keys + row, best);
  if (kCount && live && count > 0) atomicAdd(counts + row, count);
}

__global__ __launch_bounds__(kWave) void raycast_finish_kernel(const float *__restrict__ origins, const float *__restrict__ dirs,
                                                               const int32_t *__restrict__ ray_offsets,
                                                               const float *__restrict__ verts,
                                                               const int32_t *__restrict__ vert_offsets,
                                                               const int32_t *__restrict__ faces,
                                                               const int32_t *__restrict__ face_offsets, int B, int qcap, int vcap,
                                                               int fcap, const unsigned long long *__restrict__ keys,
                                                               const int32_t *__restrict__ counts, float *__restrict__ t_out,
                                                               int32_t *__restrict__ face_out, float *__restrict__ bary_out,
                                                               int32_t *__restrict__ count_out) {
  int b, row0, end;
  if (!nsdp::ragged_tile<kWave>(ray_offsets, B, qcap, static_cast<int>(blockIdx.x), b, row0, end)) return;
  const int row = row0 + static_cast<int>(threadIdx.x);
  if (row >= end) return;
  const unsigned long long key = keys[row];
  const unsigned low = static_cast<unsigned>(key & kNoFace);
  const Mesh m = mesh_of(vert_offsets, face_offsets, b, vcap, fcap);
  float bary[3] = {0.f, 0.f, 0.f};
  // (a key no face improved, or a row outside the mesh: FLT_MAX, -1, 0)
  const bool found = low != kNoFace && static_cast<int>(low) >= m.flo && static_cast<int>(low) < m.fhi;
  if (found && bary_out) {
    const size_t r3 = static_cast<size_t>(low) * 3;
    const Frame fr = frame_of(row3(origins, row), row3(dirs, row));
    float t;
    hit_face<true>(shear(fr, corner(verts, m, faces[r3])), shear(fr, corner(verts, m, faces[r3 + 1])),
                   shear(fr, corner(verts, m, faces[r3 + 2])), t, bary);
  }
  t_out[row] = found ? __uint_as_float(static_cast<unsigned>(key >> 32)) : FLT_MAX;
  face_out[row] = found ? static_cast<int32_t>(low) : -1;
  if (bary_out) {
    float *o = bary_out + static_cast<size_t>(row) * 3;
    o[0] = bary[0], o[1] = bary[1], o[2] = bary[2];
  }
  if (count_out) count_out[row] = counts[row];
}

bool sizes_ok(int B, int qcap, int fcap) {
  return B >= 1 && B <= 65535 && qcap >= 1 && fcap >= 1 && qcap <= static_cast<long long>(kMaxRows) * B &&
         fcap <= static_cast<long long>(kMaxRows) * B;
}

}  // namespace

extern "C" size_t nsdp_mesh_ray_cast_workspace_bytes(int B, int qcap, int fcap) {
  if (!sizes_ok(B, qcap, fcap)) return 0;
  return static_cast<size_t>(12) * qcap + static_cast<size_t>(24) * box_slots(B, fcap);
}

extern "C" int nsdp_mesh_ray_cast(const float *origins, const float *dirs, const int32_t *ray_offsets, const float *verts,
                                  const int32_t *vert_offsets, const int32_t *faces, const int32_t *face_offsets, int B, int qcap,
                                  int vcap, int fcap, int flags, void *workspace, float *t_out, int32_t *face_out, float *bary_out,
                                  int32_t *count_out, void *stream) {
  NSDP_REQUIRE(B >= 1 && B <= 65535, "mesh_ray_cast: batch B=%d outside 1 .. 65535", B);
  const long long most = static_cast<long long>(kMaxRows) * B;
  NSDP_REQUIRE(qcap >= 1 && qcap <= most, "mesh_ray_cast: qcap=%d outside 1 .. 2^20 rows per shape (B=%d)", qcap, B);
  NSDP_REQUIRE(vcap >= 1 && vcap <= most, "mesh_ray_cast: vcap=%d outside 1 .. 2^20 rows per shape (B=%d)", vcap, B);
  NSDP_REQUIRE(fcap >= 1 && fcap <= most, "mesh_ray_cast: fcap=%d outside 1 .. 2^20 rows per shape (B=%d)", fcap, B);
  NSDP_REQUIRE((flags & ~NSDP_RAYCAST_NO_CULL) == 0, "mesh_ray_cast: unknown flags=%d (bit 0: no culling)", flags);
  NSDP_REQUIRE(origins && dirs && ray_offsets && verts && vert_offsets && faces && face_offsets && workspace && t_out && face_out,
               "mesh_ray_cast: null pointer");
  NSDP_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 8 == 0, "mesh_ray_cast: the workspace must be 8-byte aligned");
  hipStream_t st = nsdp::as_stream(stream);
  const int cull = (flags & NSDP_RAYCAST_NO_CULL) ? 0 : 1;
  unsigned long long *keys = static_cast<unsigned long long *>(workspace);
  int32_t *counts = reinterpret_cast<int32_t *>(keys + qcap);
  float *boxes = reinterpret_cast<float *>(counts + qcap);
  // the host knows the capacities alone: the grids are sized for them, workgroups without rows return
  const unsigned qt = static_cast<unsigned>(nsdp::ragged_max_tiles(qcap, B, kWave));
  const unsigned ft = static_cast<unsigned>(nsdp::ragged_max_tiles(fcap, B, kBlock));
  // parts of a mesh's blocks: until the grid holds sixteen waves per compute unit (a shape may own every face: cut for that)
  long long parts = (16LL * nsdp::num_cus() + qt - 1) / qt;
  if (parts > ft) parts = ft;
  if (parts > 1024) parts = 1024;
  if (parts < 1) parts = 1;
  NSDP_TRACE("mesh_ray_cast<cull=%d,count=%d,parts=%d>", cull, count_out ? 1 : 0, static_cast<int>(parts));
  if (cull)
    hipLaunchKernelGGL(boxes_kernel, dim3(ft), dim3(kWave), 0, st, verts, vert_offsets, faces, face_offsets, B, vcap, fcap, boxes);
  hipLaunchKernelGGL(raycast_init_kernel, dim3(qt), dim3(kWave), 0, st, ray_offsets, B, qcap, keys, counts);
  if (count_out)
    hipLaunchKernelGGL(raycast_scan_kernel<true>, dim3(qt, static_cast<unsigned>(parts)), dim3(kWave), 0, st, origins, dirs,
                       ray_offsets, verts, vert_offsets, faces, face_offsets, B, qcap, vcap, fcap, cull, boxes, keys, counts);
  else
    hipLaunchKernelGGL(raycast_scan_kernel<false>, dim3(qt, static_cast<unsigned>(parts)), dim3(kWave), 0, st, origins, dirs,
                       ray_offsets, verts, vert_offsets, faces, face_offsets, B, qcap, vcap, fcap, cull, boxes, keys, counts);
  hipLaunchKernelGGL(raycast_finish_kernel, dim3(qt), dim3(kWave), 0, st, origins, dirs, ray_offsets, verts, vert_offsets, faces,
                     face_offsets, B, qcap, vcap, fcap, keys, counts, t_out, face_out, bary_out, count_out);
  return nsdp::launch_status("mesh_ray_cast");
}
