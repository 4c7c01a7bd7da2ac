// Self-intersections of packed triangle meshes (include/nsdp_selfintersect.h): for every face the faces of its own
// mesh it passes through, P poses of one topology per call.
//
//   prep_kernel    one wave per block of 64 consecutive faces of a mesh and pose: the faces' corners gathered once (clamped) into
//                  9-float records and the block's bounding box -> workspace; the same grid writes 0 / 0 / -1 over every output
//                  row and zeroes the per-mesh counters, so rows nobody owns are written too
//   pairs_kernel   one workgroup per block, one lane per face.  64 block boxes of the mesh are tested at a time, one per lane,
//                  against the wave's own block box; the ballot is the list of blocks to visit.  A visited block's records, face
//                  boxes, cand and reported rows are staged in LDS (17 dwords a face: an odd stride, the 32 lanes of a write
//                  group fall on 32 banks; every read is wave-uniform, a broadcast); every lane then tests its face box against
//                  each staged face and runs adjacency and the six sub-tests on the survivors.  Three forms:
//                    kCand  pass 1: cand alone (box + adjacency);
//                    kHits  pass 2: the narrow tests where both cand are within the budget;
//                    kBoth  budget = 0: one pass.
//                  Every face finds all of its partners itself, so rows need no atomics; a block adds its pairs with the partner
//                  BEHIND the face (each unordered pair once) and its skipped faces to the mesh's two integer counters.
//                  A lone wave per SIMD runs at the latency of its own instructions, and a mesh of 10 000 faces is 157 blocks
//                  on 1024 SIMDs: the workgroup of a block is 1 .. 8 waves (the host picks the count that fills the chip), each
//                  with a staging area of its own; the visited blocks are dealt round over the waves -- no barrier inside the
//                  walk, a wave reads only what it staged itself -- and wave 0 adds the waves' integer counts at the end.
//
// Built with -ffp-contract=off: every operation below rounds once, in the order the header documents.
#include <climits>

#include "../../include/nsdp_selfintersect.h"
#include "common.h"
#include "prof.h"
#include "ragged.h"

#pragma clang fp contract(off)

namespace {

constexpr int kWave = 64;                       // a block is 64 faces: one lane each
constexpr int kBlock = 64;
constexpr int kRec = 17;                        // a staged face: corners (9), box (6), cand, reported row
constexpr int kMaxRows = 1 << 20;               // rows of one kind a shape may hold
constexpr int kMaxPoses = 65535;                // (a grid's y extent)
constexpr int kMaxWaves = 8;                    // waves of a block's workgroup: 8 * (17 + 4) * 256 B = 43 KB of LDS at the most
constexpr int kFillWaves = 32768;               // 32 waves a SIMD: the chip holds fewer, the surplus shortens the tail of the busiest blocks
enum Form { kCand = 0, kHits = 1, kBoth = 2 };

struct V3 {
  float x, y, z;
};

__device__ __forceinline__ V3 sub(const V3 &a, const V3 &b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ float dot(const V3 &a, const V3 &b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ V3 cross(const V3 &u, const V3 &v) {
  return {u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x};
}
__device__ __forceinline__ bool same(const V3 &a, const V3 &b) { return a.x == b.x && a.y == b.y && a.z == b.z; }
__device__ __forceinline__ bool opposite(float s, float t) { return (s > 0.f && t < 0.f) || (s < 0.f && t > 0.f); }

// The three sub-tests "segment of s against triangle t".  sp / sq of a corner is one value whichever edge it ends, so the
// three signed volumes are formed once; the t's only where they differ in sign -- the same verdict, fewer operations.
__device__ __forceinline__ bool edges_pierce(const V3 s[3], const V3 t[3]) {
  const V3 n = cross(sub(t[1], t[0]), sub(t[2], t[0]));
  const float d[3] = {dot(sub(s[0], t[0]), n), dot(sub(s[1], t[0]), n), dot(sub(s[2], t[0]), n)};
  bool hit = false;
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    const int e1 = (e + 1) % 3;
    if (opposite(d[e], d[e1])) {
      const V3 p = s[e], D = sub(s[e1], p), a = sub(t[0], p), b = sub(t[1], p), c = sub(t[2], p);
      const float t1 = dot(D, cross(a, b)), t2 = dot(D, cross(b, c)), t3 = dot(D, cross(c, a));
      hit = hit || (t1 > 0.f && t2 > 0.f && t3 > 0.f) || (t1 < 0.f && t2 < 0.f && t3 < 0.f);
    }
  }
  return hit;
}

// A shape's rows, clamped as ragged.h clamps them; a mesh without vertices has no faces (surface_distance.hip's rule).
struct Mesh {
  int vlo, vn, flo, fhi, slot0;      // slot0: the workspace slot of the mesh's first block, flo / 64 + b
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
__device__ __forceinline__ int wave_sum(int v) {
  for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, kWave);
  return v;
}

struct Args {
  const float *verts;
  const int32_t *vert_offsets, *faces, *face_offsets, *face_ids;
  int B, vcap, fcap, budget, cull;
  long long slots;                   // box slots per pose
  float *tri;                        // (P, fcap, 9)
  int32_t *candw;                    // (P, fcap): cand by packed row
  float *boxes;                      // (P, slots, 6)
  int32_t *cand_out, *hits_out, *partner_out;
  unsigned long long *pairs_out;
  int32_t *skipped_out;
};

__global__ __launch_bounds__(kWave) void selfint_prep_kernel(const Args a) {
  const int lane = static_cast<int>(threadIdx.x);
  const size_t p = blockIdx.y;
  const long long r = static_cast<long long>(blockIdx.x) * kBlock + lane;
  if (r < a.fcap) {
    const size_t at = p * a.fcap + static_cast<size_t>(r);
    a.cand_out[at] = 0, a.hits_out[at] = 0, a.partner_out[at] = -1;
  }
  if (lane == 0 && static_cast<int>(blockIdx.x) < a.B) {
    a.pairs_out[p * a.B + blockIdx.x] = 0ull;
    a.skipped_out[p * a.B + blockIdx.x] = 0;
  }
  int b, row0, end;
  if (!nsdp::ragged_tile<kBlock>(a.face_offsets, a.B, a.fcap, static_cast<int>(blockIdx.x), b, row0, end)) return;
  const Mesh m = mesh_of(a.vert_offsets, a.face_offsets, b, a.vcap, a.fcap);
  if (m.fhi <= m.flo) return;                                  // (faces over no vertices: the mesh has no blocks)
  const float *verts = a.verts + p * a.vcap * 3;
  const int f = min(row0 + lane, end - 1);                     // (a partial block: the surplus lanes repeat its last face)
  const size_t fr = static_cast<size_t>(f) * 3;
  const V3 c0 = corner(verts, m, a.faces[fr]), c1 = corner(verts, m, a.faces[fr + 1]), c2 = corner(verts, m, a.faces[fr + 2]);
  if (row0 + lane < end) {
    float *o = a.tri + (p * a.fcap + static_cast<size_t>(f)) * 9;
    o[0] = c0.x, o[1] = c0.y, o[2] = c0.z, o[3] = c1.x, o[4] = c1.y, o[5] = c1.z, o[6] = c2.x, o[7] = c2.y, o[8] = c2.z;
  }
  const float lx = wave_min(fminf(fminf(c0.x, c1.x), c2.x)), ly = wave_min(fminf(fminf(c0.y, c1.y), c2.y)),
              lz = wave_min(fminf(fminf(c0.z, c1.z), c2.z));
  const float hx = wave_max(fmaxf(fmaxf(c0.x, c1.x), c2.x)), hy = wave_max(fmaxf(fmaxf(c0.y, c1.y), c2.y)),
              hz = wave_max(fmaxf(fmaxf(c0.z, c1.z), c2.z));
  if (lane == 0) {
    float *box = a.boxes + (p * a.slots + static_cast<size_t>(m.slot0 + (row0 - m.flo) / kBlock)) * 6;
    box[0] = lx, box[1] = ly, box[2] = lz, box[3] = hx, box[4] = hy, box[5] = hz;
  }
}

// the row under which packed face row q of mesh m is reported
__device__ __forceinline__ int reported(const int32_t *__restrict__ face_ids, const Mesh &m, int q) {
  return face_ids ? min(max(face_ids[q], m.flo), m.fhi - 1) : q;
}

template <int kForm>
__global__ __launch_bounds__(kWave * kMaxWaves) void selfint_pairs_kernel(const Args a) {
  extern __shared__ float lds[];      // per wave 64 records of kRec dwords; behind them 4 counts per wave and face
  const int waves = static_cast<int>(blockDim.x) / kWave;
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) / kWave);
  float *rec = lds + wave * (kBlock * kRec);
  int *counts = reinterpret_cast<int *>(lds + waves * (kBlock * kRec));
  int b, row0, end;
  if (!nsdp::ragged_tile<kBlock>(a.face_offsets, a.B, a.fcap, static_cast<int>(blockIdx.x), b, row0, end)) return;
  const Mesh m = mesh_of(a.vert_offsets, a.face_offsets, b, a.vcap, a.fcap);
  if (m.fhi <= m.flo) return;
  const int lane = static_cast<int>(threadIdx.x) % kWave;
  const size_t p = blockIdx.y;
  const float *tri = a.tri + p * a.fcap * 9;
  int32_t *candw = a.candw + p * a.fcap;
  const float *boxes = a.boxes + (p * a.slots + static_cast<size_t>(m.slot0)) * 6;      // the mesh's blocks
  const int nb = (m.fhi - m.flo + kBlock - 1) / kBlock;
  const bool live = row0 + lane < end;
  const int q = min(row0 + lane, end - 1);
  V3 mine[3];
  {
    const float *r = tri + static_cast<size_t>(q) * 9;
    mine[0] = {r[0], r[1], r[2]}, mine[1] = {r[3], r[4], r[5]}, mine[2] = {r[6], r[7], r[8]};
  }
  const V3 lo = {fminf(fminf(mine[0].x, mine[1].x), mine[2].x), fminf(fminf(mine[0].y, mine[1].y), mine[2].y),
                 fminf(fminf(mine[0].z, mine[1].z), mine[2].z)};
  const V3 hi = {fmaxf(fmaxf(mine[0].x, mine[1].x), mine[2].x), fmaxf(fmaxf(mine[0].y, mine[1].y), mine[2].y),
                 fmaxf(fmaxf(mine[0].z, mine[1].z), mine[2].z)};
  const float *own = boxes + static_cast<size_t>((row0 - m.flo) / kBlock) * 6;           // (uniform: scalar loads)
  const float olx = own[0], oly = own[1], olz = own[2], ohx = own[3], ohy = own[4], ohz = own[5];
  const bool skipped = kForm == kHits && candw[q] > a.budget;
  const bool active = live && !skipped;
  int cand = 0, hits = 0, behind = 0, partner = INT_MAX, turn = 0;
  if (__any(active)) {
    for (int j0 = 0; j0 < nb; j0 += kWave) {
      bool want = j0 + lane < nb;
      if (want && a.cull) {
        const float *bx = boxes + static_cast<size_t>(j0 + lane) * 6;
        want = bx[0] <= ohx && olx <= bx[3] && bx[1] <= ohy && oly <= bx[4] && bx[2] <= ohz && olz <= bx[5];
      }
      unsigned long long todo = __ballot(want);
      while (todo) {
        const int j = j0 + __ffsll(static_cast<long long>(todo)) - 1;
        todo &= todo - 1;
        if (turn++ % waves != wave) continue;                    // (wave-uniform: the visited blocks dealt round over the waves)
        const int f0 = m.flo + j * kBlock, cnt = min(kBlock, m.fhi - f0);
        // the staging area is this wave's own: its lanes run in lockstep and the LDS serves a wave's accesses in order, so the
        // records are read behind their writes and rewritten behind their reads without a workgroup barrier
        __builtin_amdgcn_wave_barrier();
        if (lane < cnt) {
          const float *g = tri + static_cast<size_t>(f0 + lane) * 9;
          float *r = rec + lane * kRec;
          const V3 c0 = {g[0], g[1], g[2]}, c1 = {g[3], g[4], g[5]}, c2 = {g[6], g[7], g[8]};
          r[0] = c0.x, r[1] = c0.y, r[2] = c0.z, r[3] = c1.x, r[4] = c1.y, r[5] = c1.z, r[6] = c2.x, r[7] = c2.y, r[8] = c2.z;
          r[9] = fminf(fminf(c0.x, c1.x), c2.x), r[10] = fminf(fminf(c0.y, c1.y), c2.y), r[11] = fminf(fminf(c0.z, c1.z), c2.z);
          r[12] = fmaxf(fmaxf(c0.x, c1.x), c2.x), r[13] = fmaxf(fmaxf(c0.y, c1.y), c2.y), r[14] = fmaxf(fmaxf(c0.z, c1.z), c2.z);
          r[15] = __int_as_float(kForm == kHits ? candw[f0 + lane] : 0);
          r[16] = __int_as_float(reported(a.face_ids, m, f0 + lane));
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        for (int f = 0; active && f < cnt; ++f) {
          const float *r = rec + f * kRec;
          // (b): closed intervals, exact; the face itself is not a partner
          if (!(r[9] <= hi.x && lo.x <= r[12] && r[10] <= hi.y && lo.y <= r[13] && r[11] <= hi.z && lo.z <= r[14]) || f0 + f == q)
            continue;
          const V3 other[3] = {{r[0], r[1], r[2]}, {r[3], r[4], r[5]}, {r[6], r[7], r[8]}};
          bool adjacent = false;                                 // (a): a corner shared as coordinates
#pragma unroll
          for (int u = 0; u < 3; ++u)
#pragma unroll
            for (int v = 0; v < 3; ++v) adjacent = adjacent || same(mine[u], other[v]);
          if (adjacent) continue;
          ++cand;
          if (kForm == kCand || (kForm == kHits && __float_as_int(r[15]) > a.budget)) continue;
          if (edges_pierce(mine, other) || edges_pierce(other, mine)) {      // (c)
            ++hits;
            partner = min(partner, __float_as_int(r[16]));
            behind += f0 + f > q ? 1 : 0;
          }
        }
      }
    }
  }
  // the waves' counts, added by wave 0 (integers: the order does not matter)
  int *mine_out = counts + (wave * kBlock + lane) * 4;
  mine_out[0] = cand, mine_out[1] = hits, mine_out[2] = behind, mine_out[3] = partner;
  __syncthreads();
  if (wave != 0) return;
  for (int w = 1; w < waves; ++w) {
    const int *o = counts + (w * kBlock + lane) * 4;
    cand += o[0], hits += o[1], behind += o[2], partner = min(partner, o[3]);
  }
  if (live) {
    const size_t at = p * a.fcap + static_cast<size_t>(reported(a.face_ids, m, q));
    if (kForm != kHits) a.cand_out[at] = cand;
    if (kForm == kCand) candw[q] = cand;
    if (kForm != kCand) {
      a.hits_out[at] = skipped ? -1 : hits;
      a.partner_out[at] = (skipped || hits == 0) ? -1 : partner;
    }
  }
  if (kForm != kCand) {
    const int pairs = wave_sum(active ? behind : 0);
    const int gone = __popcll(__ballot(live && skipped));
    if (lane == 0 && pairs) atomicAdd(a.pairs_out + p * a.B + b, static_cast<unsigned long long>(pairs));
    if (lane == 0 && gone) atomicAdd(a.skipped_out + p * a.B + b, gone);
  }
}

bool sizes_ok(int P, int B, int fcap) {
  return P >= 1 && P <= kMaxPoses && B >= 1 && B <= 65535 && fcap >= 1 && fcap <= static_cast<long long>(kMaxRows) * B;
}

long long box_slots(int B, int fcap) { return static_cast<long long>(fcap) / kBlock + B + 1; }
inline bool aligned_to(const void *p, size_t to) { return reinterpret_cast<uintptr_t>(p) % to == 0; }

}  // namespace

extern "C" size_t nsdp_mesh_self_intersections_workspace_bytes(int P, int B, int fcap) {
  if (!sizes_ok(P, B, fcap)) return 0;
  return static_cast<size_t>(4) * P * (static_cast<size_t>(10) * fcap + static_cast<size_t>(6) * box_slots(B, fcap));
}

extern "C" int nsdp_mesh_self_intersections(const float *verts, int P, const int32_t *vert_offsets, const int32_t *faces,
                                            const int32_t *face_offsets, const int32_t *face_ids, int B, int vcap, int fcap, int budget,
                                            int flags, void *workspace, int32_t *cand_out, int32_t *hits_out, int32_t *partner_out,
                                            int64_t *pairs_out, int32_t *skipped_out, void *stream) {
  NSDP_REQUIRE(P >= 1 && P <= kMaxPoses, "mesh_self_intersections: P=%d poses outside 1 .. %d", P, kMaxPoses);
  NSDP_REQUIRE(B >= 1 && B <= 65535, "mesh_self_intersections: batch B=%d outside 1 .. 65535", B);
  const long long most = static_cast<long long>(kMaxRows) * B;
  NSDP_REQUIRE(vcap >= 1 && vcap <= most, "mesh_self_intersections: vcap=%d outside 1 .. 2^20 rows per shape (B=%d)", vcap, B);
  NSDP_REQUIRE(fcap >= 1 && fcap <= most, "mesh_self_intersections: fcap=%d outside 1 .. 2^20 rows per shape (B=%d)", fcap, B);
  NSDP_REQUIRE(budget >= 0, "mesh_self_intersections: budget=%d is negative (0: no guard)", budget);
  NSDP_REQUIRE((flags & ~NSDP_SELFINT_NO_CULL) == 0, "mesh_self_intersections: unknown flags=%d (bit 0: no culling by blocks)", flags);
  NSDP_REQUIRE(verts && vert_offsets && faces && face_offsets, "mesh_self_intersections: null pointer (verts / faces / offsets)");
  NSDP_REQUIRE(workspace, "mesh_self_intersections: null pointer (workspace)");
  NSDP_REQUIRE(cand_out && hits_out && partner_out && pairs_out && skipped_out, "mesh_self_intersections: null pointer (outputs)");
  NSDP_REQUIRE(aligned_to(workspace, 16), "mesh_self_intersections: the workspace is not 16-byte aligned");
  NSDP_REQUIRE(aligned_to(verts, 4) && aligned_to(vert_offsets, 4) && aligned_to(faces, 4) && aligned_to(face_offsets, 4) &&
                   aligned_to(face_ids, 4) && aligned_to(cand_out, 4) && aligned_to(hits_out, 4) && aligned_to(partner_out, 4) &&
                   aligned_to(skipped_out, 4),
               "mesh_self_intersections: an index or fp32 operand is not 4-byte aligned");
  NSDP_REQUIRE(aligned_to(pairs_out, 8), "mesh_self_intersections: pairs_out is not 8-byte aligned");
  Args a;
  a.verts = verts, a.vert_offsets = vert_offsets, a.faces = faces, a.face_offsets = face_offsets, a.face_ids = face_ids;
  a.B = B, a.vcap = vcap, a.fcap = fcap, a.budget = budget, a.cull = (flags & NSDP_SELFINT_NO_CULL) ? 0 : 1;
  a.slots = box_slots(B, fcap);
  a.tri = static_cast<float *>(workspace);
  a.candw = reinterpret_cast<int32_t *>(a.tri + static_cast<size_t>(P) * fcap * 9);
  a.boxes = reinterpret_cast<float *>(a.candw + static_cast<size_t>(P) * fcap);
  a.cand_out = cand_out, a.hits_out = hits_out, a.partner_out = partner_out;
  a.pairs_out = reinterpret_cast<unsigned long long *>(pairs_out), a.skipped_out = skipped_out;
  hipStream_t st = nsdp::as_stream(stream);
  // the host knows the capacities alone: the grid is sized for them, workgroups without faces return
  const long long tiles = nsdp::ragged_max_tiles(fcap, B, kBlock);
  const dim3 grid(static_cast<unsigned>(tiles), static_cast<unsigned>(P));
  // waves per block: until the grid holds eight waves per SIMD
  long long waves = (kFillWaves + tiles * P - 1) / (tiles * P);
  waves = waves < 1 ? 1 : (waves > kMaxWaves ? kMaxWaves : waves);
  const dim3 threads(static_cast<unsigned>(kWave * waves));
  const size_t lds = static_cast<size_t>(waves) * kBlock * (kRec + 4) * sizeof(float);
  NSDP_TRACE("mesh_self_intersections<P=%d,B=%d,fcap=%d,budget=%d,cull=%d,waves=%d>", P, B, fcap, budget, a.cull, static_cast<int>(waves));
  hipLaunchKernelGGL(selfint_prep_kernel, grid, dim3(kWave), 0, st, a);
  if (const int rc = nsdp::launch_status("selfint_prep_kernel")) return rc;
  if (budget == 0) {
    hipLaunchKernelGGL(selfint_pairs_kernel<kBoth>, grid, threads, lds, st, a);
    return nsdp::launch_status("selfint_pairs_kernel<both>");
  }
  hipLaunchKernelGGL(selfint_pairs_kernel<kCand>, grid, threads, lds, st, a);
  if (const int rc = nsdp::launch_status("selfint_pairs_kernel<cand>")) return rc;
  hipLaunchKernelGGL(selfint_pairs_kernel<kHits>, grid, threads, lds, st, a);
  return nsdp::launch_status("selfint_pairs_kernel<hits>");
}
