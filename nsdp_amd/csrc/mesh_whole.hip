// Whole meshes of a batch out of the device-resident mesh store (include/nsdp_meshwhole.h): every vertex of the canonical, source
// and target frame of B samples of different sizes, the handle mask, the 7-wide input rows and the faces, packed back to back.
//
// Two launches, kernel nodes only:
//   offsets  ONE workgroup.  A lane sums the counts of its contiguous share of the B <= 65535 shapes (at most 256 each, read
//            through the frame and topology tables), the 256 partial sums are scanned in LDS (8 steps, one barrier each), and the
//            lane walks its share again to write vert_offsets and face_offsets.  Sums in 64 bits, saturated at the capacity as
//            they are written: min(prefix sum, cap) IS the header's recurrence, the counts being non-negative.
//   rows     one lane per vertex row, then one lane per face row, in one grid: blocks [0, vert_blocks) own vertex rows.  MI355X:
//            * a lane finds its shape by a binary search of the offsets (packed_rows.h, at most 16 steps), ONE search per wave
//              where the wave's rows fall in one shape -- then the three frame-table entries, the topology entry and the box are
//              wave-uniform addresses, read through the scalar cache;
//            * a vertex and a face are 16-byte records: consecutive lanes read consecutive records, four whole lines per wave
//              and frame, one load each; the padding element is not used;
//            * stores are 12 and 28 contiguous bytes per lane at a stride of the same size: consecutive lanes fill consecutive
//              bytes, whole lines per wave;
//            * 16 + 16 + 16 bytes read and 36 + 1 + 28 written per vertex, 16 read and 12 written per face, three compares and
//              three multiplies per row: bandwidth-bound, no LDS, no barrier; a row no shape owns (padding) is written as zeros.
// Built with -ffp-contract=off, as batch_rows.h requires: the handle rule and the input row are that file's text, so a row carries
// the bits nsdp_mesh_batch_sample would give a sample that fell on the vertex.
#include "../../include/nsdp_meshbatch.h"
#include "../../include/nsdp_meshwhole.h"
#include "batch_rows.h"
#include "common.h"
#include "packed_rows.h"      // a row's owner
#include "prof.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kScanThreads = 256;

using nsdp::aligned;
using nsdp::clampll;

struct WholeArgs {
  const float4 *verts;
  const int4 *faces;
  long long vert_rows, face_rows;
  const int64_t *frame_table, *topo_table;
  const int32_t *frame_ids;
  int n_frames, n_topos, B, vcap, fcap, vert_blocks;      // blocks [0, vert_blocks) of the rows grid own vertex rows, the others face rows
  float partial_range;
  int32_t *vert_offsets, *face_offsets, *faces_out;
  float *verts_out, *inputs_out;
  uint8_t *handle_out;
};

__device__ __forceinline__ const int64_t *frame_entry(const WholeArgs &a, int id) {
  return a.frame_table + static_cast<size_t>(min(max(id, 0), a.n_frames - 1)) * 6;
}

// V_b of the header: the count of the canonical frame whose entry is `e`
__device__ __forceinline__ int vertex_count(const WholeArgs &a, const int64_t *e) {
  const long long cap = a.vert_rows < NSDP_MESH_MAX_ELEMS ? a.vert_rows : NSDP_MESH_MAX_ELEMS;
  return static_cast<int>(clampll(static_cast<int32_t>(e[1] & 0xFFFFFFFFLL), 0, cap));
}

// F_b of the header and the first face record of the topology of the canonical frame whose entry is `e`
__device__ __forceinline__ int face_count(const WholeArgs &a, const int64_t *e, long long &first) {
  const int topo = min(max(static_cast<int>(e[1] >> 32), 0), a.n_topos - 1);
  const int64_t *et = a.topo_table + static_cast<size_t>(topo) * 2;
  const long long cap = a.face_rows < NSDP_MESH_MAX_ELEMS ? a.face_rows : NSDP_MESH_MAX_ELEMS;
  const int F = static_cast<int>(clampll(et[1], 0, cap));
  first = clampll(et[0], 0, a.face_rows - F);
  return F;
}

__global__ __launch_bounds__(kScanThreads) void mesh_whole_offsets_kernel(const WholeArgs a) {
  __shared__ long long part[2][2][kScanThreads];      // [buffer][vertices, faces][lane]
  const int t = static_cast<int>(threadIdx.x);
  const int per = (a.B + kScanThreads - 1) / kScanThreads;
  const int b0 = min(t * per, a.B), b1 = min(b0 + per, a.B);
  long long sv = 0, sf = 0, unused;
  for (int b = b0; b < b1; ++b) {
    const int64_t *e = frame_entry(a, a.frame_ids[b]);
    sv += vertex_count(a, e);
    sf += face_count(a, e, unused);
  }
  part[0][0][t] = sv, part[0][1][t] = sf;
  __syncthreads();
  int cur = 0;
  for (int d = 1; d < kScanThreads; d <<= 1) {      // inclusive scan: reads one buffer, writes the other
    long long v = part[cur][0][t], f = part[cur][1][t];
    if (t >= d) v += part[cur][0][t - d], f += part[cur][1][t - d];
    part[cur ^ 1][0][t] = v, part[cur ^ 1][1][t] = f;
    __syncthreads();
    cur ^= 1;
  }
  long long ov = part[cur][0][t] - sv, of = part[cur][1][t] - sf;      // what the lanes below this one hold
  if (t == 0) a.vert_offsets[0] = 0, a.face_offsets[0] = 0;
  for (int b = b0; b < b1; ++b) {
    const int64_t *e = frame_entry(a, a.frame_ids[b]);
    ov += vertex_count(a, e);
    of += face_count(a, e, unused);
    a.vert_offsets[b + 1] = static_cast<int32_t>(ov < a.vcap ? ov : a.vcap);
    a.face_offsets[b + 1] = static_cast<int32_t>(of < a.fcap ? of : a.fcap);
  }
}

__global__ __launch_bounds__(kThreads) void mesh_whole_rows_kernel(const WholeArgs a) {
  int b, first, end;
  if (static_cast<int>(blockIdx.x) < a.vert_blocks) {
    const long long r = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x;
    if (r >= a.vcap) return;
    float c[3] = {0.f, 0.f, 0.f}, s[3] = {0.f, 0.f, 0.f}, t[3] = {0.f, 0.f, 0.f};
    bool handle = false;
    if (owner_of_lane(a.vert_offsets, a.B, a.vcap, r, b)) {
      shape_range(a.vert_offsets, b, a.vcap, first, end);
      const int32_t *ids = a.frame_ids + b;
      const int64_t *ec = frame_entry(a, ids[0]), *es = frame_entry(a, ids[a.B]), *et = frame_entry(a, ids[2 * a.B]);
      const int V = vertex_count(a, ec);
      const long long i = r - first, last = a.vert_rows - 1;      // (i < V where the offsets are this call's; the record is clamped anyway)
      const float4 pc = a.verts[clampll(clampll(ec[0], 0, a.vert_rows - V) + i, 0, last)];
      const float4 ps = a.verts[clampll(clampll(es[0], 0, a.vert_rows - V) + i, 0, last)];
      const float4 pt = a.verts[clampll(clampll(et[0], 0, a.vert_rows - V) + i, 0, last)];
      c[0] = pc.x, c[1] = pc.y, c[2] = pc.z;
      s[0] = ps.x, s[1] = ps.y, s[2] = ps.z;
      t[0] = pt.x, t[1] = pt.y, t[2] = pt.z;
      handle = nsdp::is_handle(c, nsdp::cano_box(ec[3], ec[4], ec[5]), a.partial_range);
    }
    const size_t plane = static_cast<size_t>(a.vcap) * 3;
    float *o = a.verts_out + static_cast<size_t>(r) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      o[k] = c[k];
      o[plane + k] = s[k];
      o[2 * plane + k] = t[k];
    }
    a.handle_out[r] = handle ? 1 : 0;
    nsdp::write_inputs_row(a.inputs_out + static_cast<size_t>(r) * 7, s, t, handle);      // (padding: 0 * 0 = +0)
  } else {
    const long long q = static_cast<long long>(static_cast<int>(blockIdx.x) - a.vert_blocks) * kThreads + threadIdx.x;
    if (q >= a.fcap) return;
    int out[3] = {0, 0, 0};
    if (owner_of_lane(a.face_offsets, a.B, a.fcap, q, b)) {
      shape_range(a.face_offsets, b, a.fcap, first, end);
      const int64_t *ec = frame_entry(a, a.frame_ids[b]);
      const int hi = max(vertex_count(a, ec) - 1, 0);
      long long face_first;
      face_count(a, ec, face_first);
      const int4 rec = a.faces[clampll(face_first + (q - first), 0, a.face_rows - 1)];
      out[0] = clamped(rec.x, 0, hi), out[1] = clamped(rec.y, 0, hi), out[2] = clamped(rec.z, 0, hi);
    }
    int32_t *o = a.faces_out + static_cast<size_t>(q) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = out[k];
  }
}

}  // namespace

extern "C" int nsdp_mesh_batch_whole(const float *vert_arena, long long vert_rows, const int32_t *face_arena, long long face_rows,
                                     const int64_t *frame_table, int n_frames, const int64_t *topo_table, int n_topos,
                                     const int32_t *frame_ids, int B, int vcap, int fcap, float partial_range,
                                     int32_t *vert_offsets, int32_t *face_offsets, float *verts_out, uint8_t *handle_out,
                                     float *inputs_out, int32_t *faces_out, void *stream) {
  NSDP_REQUIRE(B >= 0 && B <= 65535, "mesh_batch_whole: batch B=%d outside [0, 65535]", B);
  NSDP_REQUIRE(vcap >= 1 && vcap < (1 << 27), "mesh_batch_whole: vcap=%d vertex rows outside [1, 2^27)", vcap);
  NSDP_REQUIRE(fcap >= 1 && fcap < (1 << 27), "mesh_batch_whole: fcap=%d face rows outside [1, 2^27)", fcap);
  NSDP_REQUIRE(n_frames >= 1, "mesh_batch_whole: n_frames=%d, the frame table needs a frame", n_frames);
  NSDP_REQUIRE(n_topos >= 1, "mesh_batch_whole: n_topos=%d, the topology table needs a topology", n_topos);
  NSDP_REQUIRE(vert_rows >= 1, "mesh_batch_whole: vert_rows=%lld, the vertex arena needs a record", vert_rows);
  NSDP_REQUIRE(face_rows >= 1, "mesh_batch_whole: face_rows=%lld, the face arena needs a record", face_rows);
  NSDP_REQUIRE(nsdp::finite_weight(partial_range), "mesh_batch_whole: partial_range is not finite");
  if (B == 0) return 0;
  NSDP_REQUIRE(vert_arena && face_arena, "mesh_batch_whole: null pointer (arenas)");
  NSDP_REQUIRE(frame_table && topo_table && frame_ids, "mesh_batch_whole: null pointer (tables / frame ids)");
  NSDP_REQUIRE(vert_offsets && face_offsets, "mesh_batch_whole: null pointer (offsets)");
  NSDP_REQUIRE(verts_out && handle_out && inputs_out && faces_out, "mesh_batch_whole: null pointer (outputs)");
  NSDP_REQUIRE(aligned(vert_arena, 16) && aligned(face_arena, 16), "mesh_batch_whole: an arena is not 16-byte aligned");
  NSDP_REQUIRE(aligned(frame_table, 8) && aligned(topo_table, 8), "mesh_batch_whole: a table is not 8-byte aligned");
  NSDP_REQUIRE(aligned(frame_ids, 4) && aligned(vert_offsets, 4) && aligned(face_offsets, 4) && aligned(verts_out, 4) &&
                   aligned(inputs_out, 4) && aligned(faces_out, 4),
               "mesh_batch_whole: an index or fp32 operand is not 4-byte aligned");
  WholeArgs a;
  a.verts = reinterpret_cast<const float4 *>(vert_arena), a.faces = reinterpret_cast<const int4 *>(face_arena);
  a.vert_rows = vert_rows, a.face_rows = face_rows;
  a.frame_table = frame_table, a.topo_table = topo_table, a.frame_ids = frame_ids;
  a.n_frames = n_frames, a.n_topos = n_topos, a.B = B, a.vcap = vcap, a.fcap = fcap, a.vert_blocks = nsdp::ceil_div(vcap, kThreads);
  a.partial_range = partial_range;
  a.vert_offsets = vert_offsets, a.face_offsets = face_offsets, a.faces_out = faces_out;
  a.verts_out = verts_out, a.inputs_out = inputs_out, a.handle_out = handle_out;
  hipStream_t st = nsdp::as_stream(stream);
  NSDP_TRACE("mesh_batch_whole<B=%d,vcap=%d,fcap=%d>", B, vcap, fcap);
  hipLaunchKernelGGL(mesh_whole_offsets_kernel, dim3(1), dim3(kScanThreads), 0, st, a);
  if (const int rc = nsdp::launch_status("mesh_whole_offsets_kernel")) return rc;
  hipLaunchKernelGGL(mesh_whole_rows_kernel, dim3(a.vert_blocks + nsdp::ceil_div(fcap, kThreads)), dim3(kThreads), 0, st, a);
  return nsdp::launch_status("mesh_whole_rows_kernel");
}
