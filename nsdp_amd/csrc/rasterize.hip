// Packed triangle meshes rasterised into depth, face and weight images (include/nsdp_raster.h).  Tile-major: no
// atomics touch the images, and none are used at all.  The blocks of 64 faces and the clamps are mesh_blocks.h's.
//
//   raster_boxes_kernel    one wave per block of 64 consecutive faces of the image's mesh: the box of the snapped corners of the
//                          faces that are not dropped, and the number that are -> workspace
//   raster_tiles_kernel    one workgroup of 256 lanes per 16 x 16 pixels of an image, one pixel per lane: the lanes read 256 block
//                          boxes at a time and vote; each of the four waves recomputes one kept block's corners and stages the
//                          faces whose own box touches the tile -- their three edge functions at the tile's first centre, the
//                          gradients, 1 / W and Z -- in LDS; every lane tests every staged face (exact in fp64: integers below
//                          2^53) and computes the fp64 depth on the covering ones alone; key and count in registers, one store
//   raster_dropped_kernel  one wave per image: the sum of its mesh's blocks' dropped counts
//
// Built with -ffp-contract=off: every operation below rounds once, in the order the header documents.
#include <cfloat>
#include <climits>

#include "../../include/nsdp_raster.h"
#include "common.h"
#include "mesh_blocks.h"
#include "prof.h"
#include "ragged.h"

#pragma clang fp contract(off)

namespace {

constexpr int kTile = 16;                       // a tile is 16 x 16 pixels, one per lane of the workgroup
constexpr int kLanes = kTile * kTile;
constexpr int kWaves = kLanes / kWave;
constexpr float kSnapMax = 16777216.f;          // 2^24: the largest |snapped coordinate| of a good corner
constexpr unsigned long long kNoFace = 0xFFFFFFFFull;
constexpr unsigned long long kStartKey = (0xFF7FFFFFull << 32) | kNoFace;      // (ordered(FLT_MAX), no face)

// a projected, snapped corner; ok: the header's "good"
struct Corner {
  int sx, sy;
  float Z, W;
  bool ok;
};

__device__ __forceinline__ Corner project(const float *__restrict__ M, const V3 &v) {
  const float X = ((M[0] * v.x + M[1] * v.y) + M[2] * v.z) + M[3];
  const float Y = ((M[4] * v.x + M[5] * v.y) + M[6] * v.z) + M[7];
  const float Z = ((M[8] * v.x + M[9] * v.y) + M[10] * v.z) + M[11];
  const float W = ((M[12] * v.x + M[13] * v.y) + M[14] * v.z) + M[15];
  const float px = X / W, py = Y / W;
  const float rx = rintf(px * 256.f), ry = rintf(py * 256.f);
  Corner c;
  // (a NaN fails every comparison: not good)
  c.ok = W > 0.f && isfinite(X) && isfinite(Y) && isfinite(Z) && isfinite(W) && fabsf(rx) <= kSnapMax && fabsf(ry) <= kSnapMax;
  c.sx = c.ok ? static_cast<int>(rx) : 0, c.sy = c.ok ? static_cast<int>(ry) : 0;
  c.Z = Z, c.W = W;
  return c;
}

// the three corners of packed face row f of mesh m under camera M
__device__ __forceinline__ bool face_corners(const float *__restrict__ verts, const int32_t *__restrict__ faces, const Mesh &m,
                                             const float *__restrict__ M, int f, Corner &a, Corner &b, Corner &c) {
  const size_t r3 = static_cast<size_t>(f) * 3;
  a = project(M, corner(verts, m, faces[r3]));
  b = project(M, corner(verts, m, faces[r3 + 1]));
  c = project(M, corner(verts, m, faces[r3 + 2]));
  return a.ok && b.ok && c.ok;
}

__device__ __forceinline__ int wave_min_i(int v) {
  for (int s = 32; s > 0; s >>= 1) v = min(v, __shfl_xor(v, s, kWave));
  return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
  for (int s = 32; s > 0; s >>= 1) v = max(v, __shfl_xor(v, s, kWave));
  return v;
}

__device__ __forceinline__ int mesh_of_image(const int32_t *__restrict__ image_shape, int img, int B) {
  return __builtin_amdgcn_readfirstlane(min(max(image_shape[img], 0), B - 1));
}

__global__ __launch_bounds__(kWave) void raster_boxes_kernel(const float *__restrict__ verts, const int32_t *__restrict__ vert_offsets,
                                                             const int32_t *__restrict__ faces,
                                                             const int32_t *__restrict__ face_offsets, const float *__restrict__ cams,
                                                             const int32_t *__restrict__ image_shape, int B, int vcap, int fcap,
                                                             long long slots, int4 *__restrict__ boxes, int32_t *__restrict__ drops) {
  const int img = static_cast<int>(blockIdx.y), j = static_cast<int>(blockIdx.x);
  const Mesh m = mesh_of(vert_offsets, face_offsets, mesh_of_image(image_shape, img, B), vcap, fcap);
  const int nb = (m.fhi - m.flo + kBlock - 1) / kBlock;
  if (j >= nb) return;
  const int f0 = m.flo + j * kBlock, cnt = min(kBlock, m.fhi - f0);
  const int lane = static_cast<int>(threadIdx.x);
  const bool live = lane < cnt;
  Corner a, b, c;
  const bool ok = face_corners(verts, faces, m, cams + static_cast<size_t>(img) * 16, f0 + min(lane, cnt - 1), a, b, c) && live;
  const int xlo = wave_min_i(ok ? min(min(a.sx, b.sx), c.sx) : INT_MAX), ylo = wave_min_i(ok ? min(min(a.sy, b.sy), c.sy) : INT_MAX);
  const int xhi = wave_max_i(ok ? max(max(a.sx, b.sx), c.sx) : INT_MIN), yhi = wave_max_i(ok ? max(max(a.sy, b.sy), c.sy) : INT_MIN);
  const int dropped = __popcll(__ballot(live && !ok));
  if (lane == 0) {
    const size_t slot = static_cast<size_t>(img) * slots + m.slot0 + j;
    boxes[slot] = make_int4(xlo, ylo, xhi, yhi);         // (no good face: an empty box, lo > hi)
    drops[slot] = dropped;
  }
}

// A staged face: the edge functions of (b, c), (c, a), (a, b) at the tile's first pixel centre and their gradients -- integers,
// exact as doubles -- then 1 / W and Z per corner, the tie-break signs and the packed face row.  15 doubles: lane i writes
// dwords 30 i .. 30 i + 29, an even stride that is no multiple of 32, so the lanes of a write group fall on different banks;
// every read is uniform over the workgroup (one address, a broadcast).
struct Rec {
  double e0[3], gx[3], gy[3], iw[3];
  float z[3];
  int tie[3];
};
static_assert(sizeof(Rec) == 120, "a staged face is 15 doubles");

__device__ __forceinline__ int sign_of(int v) { return (v > 0) - (v < 0); }

__device__ __forceinline__ void stage_edge(Rec &r, int k, const Corner &P, const Corner &Q, int cx0, int cy0) {
  const long long e = static_cast<long long>(Q.sx - cx0) * (P.sy - cy0) - static_cast<long long>(Q.sy - cy0) * (P.sx - cx0);
  const int gx = Q.sy - P.sy, gy = P.sx - Q.sx;
  r.e0[k] = static_cast<double>(e), r.gx[k] = static_cast<double>(gx), r.gy[k] = static_cast<double>(gy);
  r.tie[k] = gx != 0 ? sign_of(gx) : sign_of(gy);
}

__device__ __forceinline__ unsigned ordered(float d) {
  const unsigned u = __float_as_uint(d);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float unordered(unsigned o) { return __uint_as_float((o & 0x80000000u) ? (o ^ 0x80000000u) : ~o); }

template <bool kBary>
__global__ __launch_bounds__(kLanes) void raster_tiles_kernel(const float *__restrict__ verts, const int32_t *__restrict__ vert_offsets,
                                                              const int32_t *__restrict__ faces,
                                                              const int32_t *__restrict__ face_offsets, const float *__restrict__ cams,
                                                              const int32_t *__restrict__ image_shape, int B, int vcap, int fcap, int H,
                                                              int W, int tiles_x, int front, long long slots,
                                                              const int4 *__restrict__ boxes, float *__restrict__ depth_out,
                                                              int32_t *__restrict__ face_out, float *__restrict__ bary_out,
                                                              int32_t *__restrict__ count_out) {
  __shared__ Rec rec[kWaves * kBlock];
  __shared__ int rec_face[kWaves * kBlock];
  __shared__ int list[kLanes];
  __shared__ int voted[kWaves], staged[kWaves];
  const int img = static_cast<int>(blockIdx.y), tile = static_cast<int>(blockIdx.x);
  const int tid = static_cast<int>(threadIdx.x), wave = tid / kWave, lane = tid % kWave;
  const int x0 = (tile % tiles_x) * kTile, y0 = (tile / tiles_x) * kTile;
  const int px = x0 + tid % kTile, py = y0 + tid / kTile;
  const bool inside = px < W && py < H;
  // the centres of the tile's pixels span [cx0, cx1] x [cy0, cy1] in snapped units; this lane's is (cx0 + dx, cy0 + dy)
  const int cx0 = 256 * x0 + 128, cy0 = 256 * y0 + 128, cx1 = cx0 + 256 * (kTile - 1), cy1 = cy0 + 256 * (kTile - 1);
  const double dx = static_cast<double>(256 * (tid % kTile)), dy = static_cast<double>(256 * (tid / kTile));
  const float *__restrict__ M = cams + static_cast<size_t>(img) * 16;
  const Mesh m = mesh_of(vert_offsets, face_offsets, mesh_of_image(image_shape, img, B), vcap, fcap);
  const int nb = (m.fhi - m.flo + kBlock - 1) / kBlock;
  const int4 *__restrict__ my_boxes = boxes + static_cast<size_t>(img) * slots + m.slot0;
  const unsigned long long below = (1ull << lane) - 1;
  unsigned long long best = kStartKey;
  int count = 0;
  float bary[3] = {0.f, 0.f, 0.f};
  for (int base = 0; base < nb; base += kLanes) {
    const int j = base + tid;
    bool want = false;
    if (j < nb) {
      const int4 bx = my_boxes[j];
      want = bx.x <= cx1 && bx.z >= cx0 && bx.y <= cy1 && bx.w >= cy0;
    }
    const unsigned long long vote = __ballot(want);
    if (lane == 0) voted[wave] = __popcll(vote);
    __syncthreads();
    int first = 0, n = 0;
    for (int w = 0; w < kWaves; ++w) {
      if (w < wave) first += voted[w];
      n += voted[w];
    }
    if (want) list[first + __popcll(vote & below)] = j;
    __syncthreads();
    for (int k = 0; k < n; k += kWaves) {
      int kept = 0;
      if (k + wave < n) {                                        // (uniform over the wave)
        const int f0 = m.flo + list[k + wave] * kBlock, cnt = min(kBlock, m.fhi - f0);
        Corner a, b, c;
        bool keep = false;
        if (lane < cnt) {
          keep = face_corners(verts, faces, m, M, f0 + lane, a, b, c);
          keep = keep && min(min(a.sx, b.sx), c.sx) <= cx1 && max(max(a.sx, b.sx), c.sx) >= cx0 &&
                 min(min(a.sy, b.sy), c.sy) <= cy1 && max(max(a.sy, b.sy), c.sy) >= cy0;
        }
        const unsigned long long km = __ballot(keep);
        kept = __popcll(km);
        if (keep) {
          const int at = wave * kBlock + __popcll(km & below);
          Rec &r = rec[at];
          stage_edge(r, 0, b, c, cx0, cy0), stage_edge(r, 1, c, a, cx0, cy0), stage_edge(r, 2, a, b, cx0, cy0);
          r.iw[0] = 1.0 / static_cast<double>(a.W), r.iw[1] = 1.0 / static_cast<double>(b.W), r.iw[2] = 1.0 / static_cast<double>(c.W);
          r.z[0] = a.Z, r.z[1] = b.Z, r.z[2] = c.Z;
          rec_face[at] = f0 + lane;
        }
      }
      if (lane == 0) staged[wave] = kept;
      __syncthreads();
      for (int w = 0; w < kWaves; ++w) {
        const int ns = staged[w];
        for (int f = 0; f < ns; ++f) {
          const Rec &r = rec[w * kBlock + f];
          const double e0 = (r.e0[0] + dx * r.gx[0]) + dy * r.gy[0], e1 = (r.e0[1] + dx * r.gx[1]) + dy * r.gy[1],
                       e2 = (r.e0[2] + dx * r.gx[2]) + dy * r.gy[2];
          const int s0 = e0 > 0.0 ? 1 : (e0 < 0.0 ? -1 : r.tie[0]), s1 = e1 > 0.0 ? 1 : (e1 < 0.0 ? -1 : r.tie[1]),
                    s2 = e2 > 0.0 ? 1 : (e2 < 0.0 ? -1 : r.tie[2]);
          if (s0 == 0 || s0 != s1 || s1 != s2 || (front && s0 < 0)) continue;
          const double ta = fabs(e0) * r.iw[0], tb = fabs(e1) * r.iw[1], tc = fabs(e2) * r.iw[2];
          const double s = (ta + tb) + tc;
          const double num = (ta * static_cast<double>(r.z[0]) + tb * static_cast<double>(r.z[1])) + tc * static_cast<double>(r.z[2]);
          const float d = static_cast<float>(num / s);
          const unsigned long long key = (static_cast<unsigned long long>(ordered(d)) << 32) | static_cast<unsigned>(rec_face[w * kBlock + f]);
          ++count;
          if (key < best) {
            best = key;
            if (kBary) bary[0] = static_cast<float>(ta / s), bary[1] = static_cast<float>(tb / s), bary[2] = static_cast<float>(tc / s);
          }
        }
      }
      __syncthreads();                                           // (the records have been read)
    }
  }
  if (!inside) return;
  const size_t at = (static_cast<size_t>(img) * H + py) * W + px;
  const unsigned low = static_cast<unsigned>(best & kNoFace);
  depth_out[at] = unordered(static_cast<unsigned>(best >> 32));
  face_out[at] = low == kNoFace ? -1 : static_cast<int32_t>(low);
  if (kBary) bary_out[at * 3] = bary[0], bary_out[at * 3 + 1] = bary[1], bary_out[at * 3 + 2] = bary[2];
  if (count_out) count_out[at] = count;
}

__global__ __launch_bounds__(kWave) void raster_dropped_kernel(const int32_t *__restrict__ vert_offsets,
                                                               const int32_t *__restrict__ face_offsets,
                                                               const int32_t *__restrict__ image_shape, int B, int vcap, int fcap,
                                                               long long slots, const int32_t *__restrict__ drops,
                                                               int32_t *__restrict__ dropped_out) {
  const int img = static_cast<int>(blockIdx.x), lane = static_cast<int>(threadIdx.x);
  const Mesh m = mesh_of(vert_offsets, face_offsets, mesh_of_image(image_shape, img, B), vcap, fcap);
  const int nb = (m.fhi - m.flo + kBlock - 1) / kBlock;
  const int32_t *__restrict__ mine = drops + static_cast<size_t>(img) * slots + m.slot0;
  int sum = 0;
  for (int j = lane; j < nb; j += kWave) sum += mine[j];
  for (int s = 32; s > 0; s >>= 1) sum += __shfl_xor(sum, s, kWave);
  if (lane == 0) dropped_out[img] = sum;
}

bool sizes_ok(int B, int I, int fcap) {
  return B >= 1 && B <= 65535 && I >= 1 && I <= 65535 && fcap >= 1 && fcap <= static_cast<long long>(kMaxRows) * B;
}

}  // namespace

extern "C" size_t nsdp_mesh_rasterize_workspace_bytes(int B, int I, int fcap) {
  if (!sizes_ok(B, I, fcap)) return 0;
  return static_cast<size_t>(20) * static_cast<size_t>(I) * static_cast<size_t>(box_slots(B, fcap));
}

extern "C" int nsdp_mesh_rasterize(const float *verts, const int32_t *vert_offsets, const int32_t *faces, const int32_t *face_offsets,
                                   const float *cams, const int32_t *image_shape, int B, int I, int vcap, int fcap, int H, int W,
                                   int flags, void *workspace, float *depth_out, int32_t *face_out, float *bary_out, int32_t *count_out,
                                   int32_t *dropped_out, void *stream) {
  NSDP_REQUIRE(B >= 1 && B <= 65535, "mesh_rasterize: batch B=%d outside 1 .. 65535", B);
  const long long most = static_cast<long long>(kMaxRows) * B;
  NSDP_REQUIRE(I >= 1 && I <= 65535, "mesh_rasterize: I=%d images outside 1 .. 65535", I);
  NSDP_REQUIRE(vcap >= 1 && vcap <= most, "mesh_rasterize: vcap=%d outside 1 .. 2^20 rows per shape (B=%d)", vcap, B);
  NSDP_REQUIRE(fcap >= 1 && fcap <= most, "mesh_rasterize: fcap=%d outside 1 .. 2^20 rows per shape (B=%d)", fcap, B);
  NSDP_REQUIRE(H >= 1 && H <= 4096, "mesh_rasterize: H=%d outside 1 .. 4096", H);
  NSDP_REQUIRE(W >= 1 && W <= 4096, "mesh_rasterize: W=%d outside 1 .. 4096", W);
  NSDP_REQUIRE(static_cast<long long>(I) * H * W < (1LL << 31), "mesh_rasterize: I=%d images of H=%d x W=%d are 2^31 pixels or more", I,
               H, W);
  NSDP_REQUIRE((flags & ~NSDP_RASTER_FRONT_ONLY) == 0, "mesh_rasterize: unknown flags=%d (bit 0: front faces only)", flags);
  NSDP_REQUIRE(verts && vert_offsets && faces && face_offsets && cams && image_shape && workspace && depth_out && face_out &&
                   dropped_out,
               "mesh_rasterize: null pointer");
  NSDP_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0, "mesh_rasterize: the workspace must be 16-byte aligned");
  hipStream_t st = nsdp::as_stream(stream);
  const long long slots = box_slots(B, fcap);
  int4 *boxes = static_cast<int4 *>(workspace);
  int32_t *drops = reinterpret_cast<int32_t *>(boxes + static_cast<size_t>(I) * slots);
  // the host knows the capacities alone: a mesh has at most ceil(fcap / 64) blocks, workgroups beyond its own return
  const unsigned blocks = static_cast<unsigned>((static_cast<long long>(fcap) + kBlock - 1) / kBlock);
  const int tiles_x = (W + kTile - 1) / kTile, tiles_y = (H + kTile - 1) / kTile;
  const int front = (flags & NSDP_RASTER_FRONT_ONLY) ? 1 : 0;
  NSDP_TRACE("mesh_rasterize<bary=%d,count=%d,front=%d>", bary_out ? 1 : 0, count_out ? 1 : 0, front);
  hipLaunchKernelGGL(raster_boxes_kernel, dim3(blocks, static_cast<unsigned>(I)), dim3(kWave), 0, st, verts, vert_offsets, faces,
                     face_offsets, cams, image_shape, B, vcap, fcap, slots, boxes, drops);
  const dim3 grid(static_cast<unsigned>(tiles_x * tiles_y), static_cast<unsigned>(I));
  if (bary_out)
    hipLaunchKernelGGL(raster_tiles_kernel<true>, grid, dim3(kLanes), 0, st, verts, vert_offsets, faces, face_offsets, cams,
                       image_shape, B, vcap, fcap, H, W, tiles_x, front, slots, boxes, depth_out, face_out, bary_out, count_out);
  else
    hipLaunchKernelGGL(raster_tiles_kernel<false>, grid, dim3(kLanes), 0, st, verts, vert_offsets, faces, face_offsets, cams,
                       image_shape, B, vcap, fcap, H, W, tiles_x, front, slots, boxes, depth_out, face_out, bary_out, count_out);
  hipLaunchKernelGGL(raster_dropped_kernel, dim3(static_cast<unsigned>(I)), dim3(kWave), 0, st, vert_offsets, face_offsets, image_shape,
                     B, vcap, fcap, slots, drops, dropped_out);
  return nsdp::launch_status("mesh_rasterize");
}
