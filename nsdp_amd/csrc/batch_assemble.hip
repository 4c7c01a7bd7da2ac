// Training batches from a device-resident data set (include/nsdp_batch.h): the row subsets of a batch by a keyed bijection,
// and the reference's per-sample tensor contract for the whole batch in one launch.
//
// subset_draw: one lane per output row.  The lane derives its sample's key and the eight round keys itself (fourteen integer
// mixes: cheaper than a trip through LDS) and walks the Feistel network's cycle back into [0, n): integer work only, O(n_keep)
// per sample where the sort it replaces is O(n_full log n_full) over n_full random keys.
//
// batch_assemble: one lane per KEPT row; a kept row is a few bytes at a random place of a frame of megabytes, so the kernel is
// bound by the number of 64-byte lines it touches and by how many of them a wave has in flight, not by bytes.  MI355X design:
//   * points and normals of a surface row share one record: a lane's canonical, source and target rows are three lines, not six;
//     space records are padded to a power of two so that one never straddles a line;
//   * every record is fetched by naturally aligned dword loads (3 per fp16 surface record, 2 per fp16 space record), and a lane
//     issues all of its loads -- index, frame ids, table entries, then the three records -- before it uses any: three
//     independent line fetches in flight per lane, 192 per wave;
//   * the frame table (48 bytes per frame) and the frame ids are read by every lane of a sample: wave-uniform addresses that
//     stay in the scalar / L1 caches;
//   * outputs are written by the lane that owns the row, 12 or 28 contiguous bytes at a stride of the same size: consecutive
//     lanes fill consecutive bytes, whole lines per wave-instruction triple.
// No LDS, no barrier: surplus lanes simply return.
#include <climits>

#include "../../include/nsdp_batch.h"
#include "batch_rows.h"
#include "common.h"
#include "draw_key.h"
#include "prof.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kRounds = 8;

using nsdp::absorb;      // (draw_key.h: shared with the other keyed draw)
using nsdp::mix32;
using nsdp::aligned;     // (batch_rows.h: shared with the other writer of batch rows)
using nsdp::clampll;

// `base`: the key after seed, epoch and step (host); rows_out[b, j] = pi_b(j mod n)
__global__ __launch_bounds__(kThreads) void subset_draw_kernel(const int32_t *__restrict__ n_full, int n_keep, uint32_t base,
                                                               uint32_t which, int32_t *__restrict__ rows_out) {
  const int j = static_cast<int>(blockIdx.x) * kThreads + static_cast<int>(threadIdx.x);
  if (j >= n_keep) return;
  const uint32_t b = blockIdx.y;
  const uint32_t n = static_cast<uint32_t>(min(max(n_full[b], 1), NSDP_BATCH_MAX_ROWS));
  // 2^w >= n: w = 32 - clz(n - 1) for n > 1; halves of h = ceil(w / 2) bits, at least one
  const int w = n > 1 ? 32 - __clz(static_cast<int>(n - 1)) : 0;
  const int h = max(1, (w + 1) >> 1);
  const uint32_t mask = (1u << h) - 1u;
  const uint32_t key = absorb(absorb(base, b), which);
  uint32_t rk[kRounds];
#pragma unroll
  for (int r = 0; r < kRounds; ++r) rk[r] = mix32(key + 0x85EBCA6Bu * static_cast<uint32_t>(r + 1));
  uint32_t x = static_cast<uint32_t>(j) % n;
  do {
    uint32_t L = x >> h, R = x & mask;
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
      const uint32_t t = L ^ (mix32(R ^ rk[r]) >> (32 - h));
      L = R;
      R = t;
    }
    x = (L << h) | R;
  } while (x >= n);      // (x < 2^(2h) always; the cycle re-enters [0, n) at the latest where it started)
  rows_out[static_cast<size_t>(b) * n_keep + j] = static_cast<int32_t>(x);
}

struct FrameRef {
  long long surf_first, space_first;
  int surf_rows, space_rows;
  nsdp::CanoBox box;
};

// the table entry of frame `id` (clamped), its counts and first records clamped to the arenas
__device__ __forceinline__ FrameRef frame_ref(const int64_t *__restrict__ table, int n_frames, int id, long long surface_rows,
                                              long long space_rows) {
  const int64_t *e = table + static_cast<size_t>(min(max(id, 0), n_frames - 1)) * 6;
  const int64_t w0 = e[0], w1 = e[1], w2 = e[2], w3 = e[3], w4 = e[4], w5 = e[5];
  FrameRef f;
  f.surf_rows = static_cast<int>(clampll(static_cast<int32_t>(w2 & 0xFFFFFFFFLL), 0, min(surface_rows, static_cast<long long>(INT_MAX))));
  f.space_rows = static_cast<int>(clampll(static_cast<int32_t>(w2 >> 32), 0, min(space_rows, static_cast<long long>(INT_MAX))));
  f.surf_first = clampll(w0, 0, surface_rows - f.surf_rows);
  f.space_first = clampll(w1, 0, space_rows - f.space_rows);
  f.box = nsdp::cano_box(w3, w4, w5);
  return f;
}

// record `first + row` of an arena of `rows` records (rows >= 1), the row clamped to the frame, the record to the arena
__device__ __forceinline__ long long record_of(long long first, int count, int row, long long rows) {
  const long long r = first + min(max(row, 0), max(count - 1, 0));
  return clampll(r, 0, rows - 1);
}

__device__ __forceinline__ float half_bits_to_float(uint32_t bits) {
  return static_cast<float>(__builtin_bit_cast(_Float16, static_cast<uint16_t>(bits & 0xFFFFu)));
}

struct Rec6 { float v[6]; };
struct Rec3 { float v[3]; };

template <bool kF16>
__device__ __forceinline__ Rec6 load_surface(const void *__restrict__ arena, long long rec) {
  Rec6 o;
  if constexpr (kF16) {
    const uint32_t *p = static_cast<const uint32_t *>(arena) + rec * 3;      // 12 bytes, 4-byte aligned
    const uint32_t a = p[0], b = p[1], c = p[2];
    o.v[0] = half_bits_to_float(a); o.v[1] = half_bits_to_float(a >> 16);
    o.v[2] = half_bits_to_float(b); o.v[3] = half_bits_to_float(b >> 16);
    o.v[4] = half_bits_to_float(c); o.v[5] = half_bits_to_float(c >> 16);
  } else {
    const float2 *p = static_cast<const float2 *>(arena) + rec * 3;          // 24 bytes, 8-byte aligned
    const float2 a = p[0], b = p[1], c = p[2];
    o.v[0] = a.x; o.v[1] = a.y; o.v[2] = b.x; o.v[3] = b.y; o.v[4] = c.x; o.v[5] = c.y;
  }
  return o;
}

template <bool kF16>
__device__ __forceinline__ Rec3 load_space(const void *__restrict__ arena, long long rec) {
  Rec3 o;
  if constexpr (kF16) {
    const uint2 a = static_cast<const uint2 *>(arena)[rec];                  // 8 bytes, 8-byte aligned
    o.v[0] = half_bits_to_float(a.x); o.v[1] = half_bits_to_float(a.x >> 16); o.v[2] = half_bits_to_float(a.y);
  } else {
    const float4 a = static_cast<const float4 *>(arena)[rec];                // 16 bytes, 16-byte aligned
    o.v[0] = a.x; o.v[1] = a.y; o.v[2] = a.z;
  }
  return o;
}

struct AssembleArgs {
  const void *surface_arena, *space_arena;
  long long surface_rows, space_rows;
  const int64_t *frame_table;
  const int32_t *frame_ids, *surf_idx, *space_idx;
  nsdp::RowArgs rows;
  int n_frames, B, n, m, surf_blocks;      // blocks [0, surf_blocks) of the grid's x own surface rows, the others space rows
};

template <bool kSurfF16, bool kSpaceF16>
__global__ __launch_bounds__(kThreads) void batch_assemble_kernel(const AssembleArgs a) {
  const int b = static_cast<int>(blockIdx.y);
  const int32_t *ids = a.frame_ids + b;
  if (static_cast<int>(blockIdx.x) < a.surf_blocks) {
    const int j = static_cast<int>(blockIdx.x) * kThreads + static_cast<int>(threadIdx.x);
    if (j >= a.n) return;
    const size_t row = static_cast<size_t>(b) * a.n + j;
    const int idx = a.surf_idx[row];
    const FrameRef fc = frame_ref(a.frame_table, a.n_frames, ids[0], a.surface_rows, a.space_rows);
    const FrameRef fs = frame_ref(a.frame_table, a.n_frames, ids[a.B], a.surface_rows, a.space_rows);
    const FrameRef ft = frame_ref(a.frame_table, a.n_frames, ids[2 * a.B], a.surface_rows, a.space_rows);
    const Rec6 c = load_surface<kSurfF16>(a.surface_arena, record_of(fc.surf_first, fc.surf_rows, idx, a.surface_rows));
    Rec6 s = load_surface<kSurfF16>(a.surface_arena, record_of(fs.surf_first, fs.surf_rows, idx, a.surface_rows));
    const Rec6 t = load_surface<kSurfF16>(a.surface_arena, record_of(ft.surf_first, ft.surf_rows, idx, a.surface_rows));
    nsdp::write_surface_row(a.rows, a.B, a.n, row, fc.box, c.v, c.v + 3, s.v, s.v + 3, t.v, t.v + 3);
  } else {
    const int j = (static_cast<int>(blockIdx.x) - a.surf_blocks) * kThreads + static_cast<int>(threadIdx.x);
    if (j >= a.m) return;
    const size_t row = static_cast<size_t>(b) * a.m + j;
    const int idx = a.space_idx ? a.space_idx[row] : j;
    const FrameRef fc = frame_ref(a.frame_table, a.n_frames, ids[0], a.surface_rows, a.space_rows);
    const FrameRef fs = frame_ref(a.frame_table, a.n_frames, ids[a.B], a.surface_rows, a.space_rows);
    const FrameRef ft = frame_ref(a.frame_table, a.n_frames, ids[2 * a.B], a.surface_rows, a.space_rows);
    const Rec3 c = load_space<kSpaceF16>(a.space_arena, record_of(fc.space_first, fc.space_rows, idx, a.space_rows));
    const Rec3 s = load_space<kSpaceF16>(a.space_arena, record_of(fs.space_first, fs.space_rows, idx, a.space_rows));
    const Rec3 t = load_space<kSpaceF16>(a.space_arena, record_of(ft.space_first, ft.space_rows, idx, a.space_rows));
    nsdp::write_space_row(a.rows, a.B, a.m, row, c.v, s.v, t.v);
  }
}

}  // namespace

extern "C" int nsdp_subset_draw(const int32_t *n_full, int B, int n_keep, uint64_t seed, uint32_t epoch, uint32_t step, int which,
                                int32_t *rows_out, void *stream) {
  NSDP_REQUIRE(B >= 0 && B <= 65535, "subset_draw: batch B=%d outside [0, 65535]", B);
  NSDP_REQUIRE(n_keep >= 0 && n_keep <= NSDP_BATCH_MAX_ROWS, "subset_draw: n_keep=%d outside [0, %d]", n_keep, NSDP_BATCH_MAX_ROWS);
  NSDP_REQUIRE(static_cast<long long>(B) * n_keep < (1LL << 31), "subset_draw: B=%d x n_keep=%d rows too large", B, n_keep);
  NSDP_REQUIRE(which == NSDP_DRAW_SURFACE || which == NSDP_DRAW_SPACE, "subset_draw: which=%d is neither the surface (0) nor the space (1) stream", which);
  if (B == 0 || n_keep == 0) return 0;
  NSDP_REQUIRE(n_full && rows_out, "subset_draw: null pointer");
  NSDP_REQUIRE(aligned(n_full, 4) && aligned(rows_out, 4), "subset_draw: a pointer is not 4-byte aligned");
  const uint32_t base = nsdp::draw_base_key(seed, epoch, step);
  NSDP_TRACE("subset_draw<B=%d,n_keep=%d>", B, n_keep);
  hipLaunchKernelGGL(subset_draw_kernel, dim3(nsdp::ceil_div(n_keep, kThreads), B), dim3(kThreads), 0, nsdp::as_stream(stream),
                     n_full, n_keep, base, static_cast<uint32_t>(which), rows_out);
  return nsdp::launch_status("subset_draw_kernel");
}

extern "C" int nsdp_batch_assemble(const void *surface_arena, long long surface_rows, int surface_f16, const void *space_arena,
                                   long long space_rows, int space_f16, const int64_t *frame_table, int n_frames,
                                   const int32_t *frame_ids, int B, const int32_t *surf_idx, int n, const int32_t *space_idx, int m,
                                   float partial_range, const float *noise, float noise_level, float *surface_out,
                                   uint8_t *handle_out, float *inputs_out, float *space_out, void *stream) {
  AssembleArgs a;
  a.rows = {noise, surface_out, inputs_out, space_out, handle_out, partial_range, noise_level};
  if (const int rc = nsdp::batch_sizes_ok("batch_assemble", B, n, m, n_frames)) return rc;
  NSDP_REQUIRE(n == 0 || surface_rows >= 1, "batch_assemble: surface_rows=%lld, the surface arena needs a record", surface_rows);
  NSDP_REQUIRE(m == 0 || space_rows >= 1, "batch_assemble: space_rows=%lld, the space arena needs a record", space_rows);
  if (const int rc = nsdp::batch_values_ok("batch_assemble", a.rows)) return rc;
  if (B == 0 || (n == 0 && m == 0)) return 0;
  NSDP_REQUIRE(frame_table && frame_ids, "batch_assemble: null pointer (frame table / frame ids)");
  NSDP_REQUIRE(n == 0 || (surface_arena && surf_idx && nsdp::surface_outputs_given(a.rows)), "batch_assemble: null pointer (surface operands)");
  NSDP_REQUIRE(m == 0 || (space_arena && space_out), "batch_assemble: null pointer (space operands)");
  NSDP_REQUIRE((n == 0 || aligned(surface_arena, 16)) && (m == 0 || aligned(space_arena, 16)), "batch_assemble: an arena is not 16-byte aligned");
  NSDP_REQUIRE(aligned(frame_table, 8), "batch_assemble: the frame table is not 8-byte aligned");
  NSDP_REQUIRE(aligned(frame_ids, 4) && aligned(surf_idx, 4) && aligned(space_idx, 4) && nsdp::rows_aligned(a.rows),
               "batch_assemble: an index or fp32 operand is not 4-byte aligned");
  a.surface_arena = surface_arena, a.space_arena = space_arena;
  a.surface_rows = surface_rows > 0 ? surface_rows : 0, a.space_rows = space_rows > 0 ? space_rows : 0;      // (of a part without rows: unread)
  a.frame_table = frame_table, a.frame_ids = frame_ids, a.surf_idx = surf_idx, a.space_idx = space_idx;
  a.n_frames = n_frames, a.B = B, a.n = n, a.m = m, a.surf_blocks = nsdp::ceil_div(n, kThreads);
  const dim3 grid(a.surf_blocks + nsdp::ceil_div(m, kThreads), B);
  hipStream_t st = nsdp::as_stream(stream);
  NSDP_TRACE("batch_assemble<B=%d,n=%d,m=%d,f16=%d%d>", B, n, m, surface_f16 != 0, space_f16 != 0);
  if (surface_f16 && space_f16) hipLaunchKernelGGL((batch_assemble_kernel<true, true>), grid, dim3(kThreads), 0, st, a);
  else if (surface_f16) hipLaunchKernelGGL((batch_assemble_kernel<true, false>), grid, dim3(kThreads), 0, st, a);
  else if (space_f16) hipLaunchKernelGGL((batch_assemble_kernel<false, true>), grid, dim3(kThreads), 0, st, a);
  else hipLaunchKernelGGL((batch_assemble_kernel<false, false>), grid, dim3(kThreads), 0, st, a);
  return nsdp::launch_status("batch_assemble_kernel");
}
