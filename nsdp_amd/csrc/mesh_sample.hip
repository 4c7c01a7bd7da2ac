// Training batches sampled from device-resident mesh sequences (include/nsdp_meshbatch.h): per output row an area-weighted
// face of the canonical frame, a barycentric weight and, for space rows, an offset along the face normal -- drawn from the row's
// own key and applied to the canonical, source and target frame -- written as nsdp_batch_assemble's four tensors in one launch.
//
// mesh_batch_sample: one lane per output row, surface and space rows in one grid, a workgroup inside ONE sample.  MI355X design:
//   * everything a sample shares -- the three frame-table entries, the topology entry, the bounding box, the key's sample part --
//     hangs on blockIdx and the kernel arguments alone: wave-uniform addresses, read through the scalar cache once per wave;
//   * the face pick is a binary search over the canonical frame's thresholds (4 bytes per face: 160 KB at 40 000 faces, resident
//     in L2).  Its first levels hit the same few lines for every lane of every wave; the last ones scatter.  No LDS stage:
//     measured alone, a coarse level of 64 / 256 / 1024 thresholds filled per workgroup takes the search of 32 x 10 240 rows
//     from 0.0158 to 0.0149 / 0.0146 / 0.0161 ms -- 0.0012 ms of this 0.052 ms launch (profiles/mesh_store.txt);
//   * a face is one 16-byte record and a vertex one 16-byte record, so a gather never straddles a line: one load for the face,
//     then nine INDEPENDENT gathers (three corners of three frames) issued before any is used -- nine line fetches in flight
//     per lane.  The source asks for 16 bytes; the padding element is unused, and what hipcc emits for gfx950 is a dwordx3 for
//     the face and for each source and target corner, and two overlapping dwordx2 (x y, y z) for each canonical corner: 15
//     vector loads over 10 lines, beside the dword probes of the search and a dwordx3 for the noise;
//   * a dozen fp32 operations per frame, one correctly rounded sqrt and three divisions: nothing beside the gathers;
//   * outputs are written by the lane that owns the row, 12 or 28 contiguous bytes at a stride of the same size: consecutive
//     lanes fill consecutive bytes, whole lines per wave-instruction triple.
// No LDS, no barrier: surplus lanes simply return.
#include <climits>

#include "../../include/nsdp_batch.h"
#include "../../include/nsdp_meshbatch.h"
#include "batch_rows.h"
#include "common.h"
#include "draw_key.h"
#include "prof.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;

using nsdp::absorb;      // (draw_key.h: shared with the other keyed draw)
using nsdp::mix32;
using nsdp::aligned;     // (batch_rows.h: shared with the other writer of batch rows)
using nsdp::clampll;

struct SampleArgs {
  const float4 *verts;
  const int4 *faces;
  const uint32_t *thr;
  long long vert_rows, face_rows, thr_rows;
  const int64_t *frame_table, *topo_table;
  const int32_t *frame_ids;
  nsdp::RowArgs rows;
  int n_frames, n_topos, B, n, m, surf_blocks;      // blocks [0, surf_blocks) of the grid's x own surface rows, the others space rows
  uint32_t base;                                    // the key after seed, epoch and step (host)
  float sigma1, sigma2;
};

struct FrameRef {
  long long first;      // first vertex record, clamped so that `count` records lie inside the arena
  int count;            // vertices, clamped to the arena and to NSDP_MESH_MAX_ELEMS
};

__device__ __forceinline__ const int64_t *frame_entry(const SampleArgs &a, int id) {
  return a.frame_table + static_cast<size_t>(min(max(id, 0), a.n_frames - 1)) * 6;
}

__device__ __forceinline__ FrameRef frame_ref(const SampleArgs &a, const int64_t *e) {
  FrameRef f;
  const long long cap = a.vert_rows < NSDP_MESH_MAX_ELEMS ? a.vert_rows : NSDP_MESH_MAX_ELEMS;
  f.count = static_cast<int>(clampll(static_cast<int32_t>(e[1] & 0xFFFFFFFFLL), 0, cap));
  f.first = clampll(e[0], 0, a.vert_rows - f.count);
  return f;
}

// vertex `idx` (local, as the face arena holds it) of frame `f`: the index clamped to the frame, the record to the arena
__device__ __forceinline__ float4 load_vertex(const SampleArgs &a, const FrameRef &f, int idx) {
  const long long r = f.first + min(max(idx, 0), max(f.count - 1, 0));
  return a.verts[clampll(r, 0, a.vert_rows - 1)];
}

struct Sampled { float p[3], nrm[3]; };

// the header's per-frame rule: the point at weights (w0, u, v) of triangle (A, B, C) and the triangle's unit normal
__device__ __forceinline__ Sampled sample_triangle(const float4 A, const float4 B, const float4 C, float w0, float u, float v) {
  const float a[3] = {A.x, A.y, A.z}, b[3] = {B.x, B.y, B.z}, c[3] = {C.x, C.y, C.z};
  Sampled o;
  float e1[3], e2[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    o.p[k] = __fadd_rn(__fadd_rn(__fmul_rn(w0, a[k]), __fmul_rn(u, b[k])), __fmul_rn(v, c[k]));
    e1[k] = __fsub_rn(b[k], a[k]);
    e2[k] = __fsub_rn(c[k], a[k]);
  }
  float cr[3];
  cr[0] = __fsub_rn(__fmul_rn(e1[1], e2[2]), __fmul_rn(e1[2], e2[1]));
  cr[1] = __fsub_rn(__fmul_rn(e1[2], e2[0]), __fmul_rn(e1[0], e2[2]));
  cr[2] = __fsub_rn(__fmul_rn(e1[0], e2[1]), __fmul_rn(e1[1], e2[0]));
  // (sqrtf and / of a HIP translation unit are the correctly rounded ones; the __f*_rn forms of sqrt and division are not)
  const float len = __builtin_sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(cr[0], cr[0]), __fmul_rn(cr[1], cr[1])), __fmul_rn(cr[2], cr[2])));
#pragma unroll
  for (int k = 0; k < 3; ++k) o.nrm[k] = len == 0.f ? 0.f : cr[k] / len;
  return o;
}

__global__ __launch_bounds__(kThreads) void mesh_batch_sample_kernel(const SampleArgs a) {
  const int b = static_cast<int>(blockIdx.y);
  const bool surface = static_cast<int>(blockIdx.x) < a.surf_blocks;
  const int j = (static_cast<int>(blockIdx.x) - (surface ? 0 : a.surf_blocks)) * kThreads + static_cast<int>(threadIdx.x);
  if (j >= (surface ? a.n : a.m)) return;
  // ---- what the sample shares (wave-uniform)
  const int32_t *ids = a.frame_ids + b;
  const int64_t *ec = frame_entry(a, ids[0]);
  const FrameRef fc = frame_ref(a, ec), fs = frame_ref(a, frame_entry(a, ids[a.B])), ft = frame_ref(a, frame_entry(a, ids[2 * a.B]));
  const int topo = min(max(static_cast<int>(ec[1] >> 32), 0), a.n_topos - 1);
  const int64_t *et = a.topo_table + static_cast<size_t>(topo) * 2;
  long long cap = a.face_rows < a.thr_rows ? a.face_rows : a.thr_rows;
  cap = cap < NSDP_MESH_MAX_ELEMS ? cap : NSDP_MESH_MAX_ELEMS;
  const int F = static_cast<int>(clampll(et[1], 0, cap));
  const long long face_first = clampll(et[0], 0, a.face_rows - F);
  const uint32_t *T = a.thr + clampll(ec[2], 0, a.thr_rows - F);
  const uint32_t key = absorb(absorb(a.base, static_cast<uint32_t>(b)), surface ? NSDP_DRAW_MESH_SURFACE : NSDP_DRAW_MESH_SPACE);
  // ---- the row's four words
  uint32_t word[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const uint32_t rk = mix32(key + 0x85EBCA6Bu * static_cast<uint32_t>(c + 1));
    word[c] = mix32(mix32(static_cast<uint32_t>(j) ^ rk) + rk);
  }
  // ---- the face: the first f with T[f] > r   (lo, mid < hi <= F throughout: every probe lies inside the F rows)
  const uint32_t r = word[0] >> 1;
  int lo = 0, hi = F;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (T[mid] > r) hi = mid;
    else lo = mid + 1;
  }
  const int f = min(lo, max(F - 1, 0));
  const int4 face = a.faces[clampll(face_first + f, 0, a.face_rows - 1)];
  // ---- nine independent gathers
  const float4 ca = load_vertex(a, fc, face.x), cb = load_vertex(a, fc, face.y), cc = load_vertex(a, fc, face.z);
  const float4 sa = load_vertex(a, fs, face.x), sb = load_vertex(a, fs, face.y), sc = load_vertex(a, fs, face.z);
  const float4 ta = load_vertex(a, ft, face.x), tb = load_vertex(a, ft, face.y), tc = load_vertex(a, ft, face.z);
  // ---- the weights, on integers
  uint32_t iu = word[1] >> 8, iv = word[2] >> 8;
  if (iu + iv > (1u << 24)) iu = (1u << 24) - iu, iv = (1u << 24) - iv;
  const uint32_t iw = (1u << 24) - iu - iv;
  constexpr float kScale = 1.f / 16777216.f;      // 2^-24: the products are exact
  const float w0 = static_cast<float>(iw) * kScale, u = static_cast<float>(iu) * kScale, v = static_cast<float>(iv) * kScale;
  const Sampled c = sample_triangle(ca, cb, cc, w0, u, v), t = sample_triangle(ta, tb, tc, w0, u, v);
  Sampled s = sample_triangle(sa, sb, sc, w0, u, v);      // (the surface row adds its noise to it)
  if (surface) {
    const size_t row = static_cast<size_t>(b) * a.n + j;
    nsdp::write_surface_row(a.rows, a.B, a.n, row, nsdp::cano_box(ec[3], ec[4], ec[5]), c.p, c.nrm, s.p, s.nrm, t.p, t.nrm);
  } else {
    const float t01 = static_cast<float>(word[3] >> 8) * kScale;
    const float tt = __fsub_rn(__fmul_rn(2.f, t01), 1.f);                    // exact: a multiple of 2^-23 in [-1, 1)
    const float d = __fmul_rn(tt, j < a.m / 2 ? a.sigma1 : a.sigma2);
    const size_t row = static_cast<size_t>(b) * a.m + j;
    float cq[3], sq[3], tq[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      cq[k] = __fadd_rn(c.p[k], __fmul_rn(c.nrm[k], d));
      sq[k] = __fadd_rn(s.p[k], __fmul_rn(s.nrm[k], d));
      tq[k] = __fadd_rn(t.p[k], __fmul_rn(t.nrm[k], d));
    }
    nsdp::write_space_row(a.rows, a.B, a.m, row, cq, sq, tq);
  }
}

}  // namespace

extern "C" int nsdp_mesh_batch_sample(const float *vert_arena, long long vert_rows, const int32_t *face_arena, long long face_rows,
                                      const uint32_t *thr_arena, long long thr_rows, const int64_t *frame_table, int n_frames,
                                      const int64_t *topo_table, int n_topos, const int32_t *frame_ids, int B, int n, int m,
                                      uint64_t seed, uint32_t epoch, uint32_t step, float partial_range, float sigma1, float sigma2,
                                      const float *noise, float noise_level, float *surface_out, uint8_t *handle_out,
                                      float *inputs_out, float *space_out, void *stream) {
  SampleArgs a;
  a.rows = {noise, surface_out, inputs_out, space_out, handle_out, partial_range, noise_level};
  if (const int rc = nsdp::batch_sizes_ok("mesh_batch_sample", B, n, m, n_frames)) return rc;
  NSDP_REQUIRE(n_topos >= 1, "mesh_batch_sample: n_topos=%d, the topology table needs a topology", n_topos);
  NSDP_REQUIRE(vert_rows >= 1, "mesh_batch_sample: vert_rows=%lld, the vertex arena needs a record", vert_rows);
  NSDP_REQUIRE(face_rows >= 1, "mesh_batch_sample: face_rows=%lld, the face arena needs a record", face_rows);
  NSDP_REQUIRE(thr_rows >= 1, "mesh_batch_sample: thr_rows=%lld, the threshold arena needs a row", thr_rows);
  if (const int rc = nsdp::batch_values_ok("mesh_batch_sample", a.rows)) return rc;
  NSDP_REQUIRE(nsdp::finite_weight(sigma1) && nsdp::finite_weight(sigma2), "mesh_batch_sample: sigma1 / sigma2 is not finite");
  if (B == 0 || (n == 0 && m == 0)) return 0;
  NSDP_REQUIRE(vert_arena && face_arena && thr_arena, "mesh_batch_sample: null pointer (arenas)");
  NSDP_REQUIRE(frame_table && topo_table && frame_ids, "mesh_batch_sample: null pointer (tables / frame ids)");
  NSDP_REQUIRE(n == 0 || nsdp::surface_outputs_given(a.rows), "mesh_batch_sample: null pointer (surface outputs)");
  NSDP_REQUIRE(m == 0 || space_out, "mesh_batch_sample: null pointer (space output)");
  NSDP_REQUIRE(aligned(vert_arena, 16) && aligned(face_arena, 16), "mesh_batch_sample: an arena is not 16-byte aligned");
  NSDP_REQUIRE(aligned(frame_table, 8) && aligned(topo_table, 8), "mesh_batch_sample: a table is not 8-byte aligned");
  NSDP_REQUIRE(aligned(thr_arena, 4) && aligned(frame_ids, 4) && nsdp::rows_aligned(a.rows),
               "mesh_batch_sample: a threshold, index or fp32 operand is not 4-byte aligned");
  a.verts = reinterpret_cast<const float4 *>(vert_arena), a.faces = reinterpret_cast<const int4 *>(face_arena), a.thr = thr_arena;
  a.vert_rows = vert_rows, a.face_rows = face_rows, a.thr_rows = thr_rows;
  a.frame_table = frame_table, a.topo_table = topo_table, a.frame_ids = frame_ids;
  a.n_frames = n_frames, a.n_topos = n_topos, a.B = B, a.n = n, a.m = m, a.surf_blocks = nsdp::ceil_div(n, kThreads);
  a.base = nsdp::draw_base_key(seed, epoch, step);
  a.sigma1 = sigma1, a.sigma2 = sigma2;
  const dim3 grid(a.surf_blocks + nsdp::ceil_div(m, kThreads), B);
  NSDP_TRACE("mesh_batch_sample<B=%d,n=%d,m=%d>", B, n, m);
  hipLaunchKernelGGL(mesh_batch_sample_kernel, grid, dim3(kThreads), 0, nsdp::as_stream(stream), a);
  return nsdp::launch_status("mesh_batch_sample_kernel");
}
