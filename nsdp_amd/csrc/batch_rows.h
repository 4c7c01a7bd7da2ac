// The rows of a training batch (include/nsdp_batch.h, include/nsdp_meshbatch.h): the reference's per-sample tensor contract --
// source noise, the handle mask against the canonical box, the six surface planes, the 7-wide input row, the three space planes
// -- and the argument checks that go with it, one definition for batch_assemble.hip (rows fetched from sample pools) and
// mesh_sample.hip (rows sampled from triangles), beside draw_key.h; mesh_whole.hip (include/nsdp_meshwhole.h: every VERTEX of a
// batch's meshes) takes the handle rule and the input row from here as well.  Include it ONLY from translation units built with
// -ffp-contract=off: the arithmetic is one rounding per operation (spelled with the __f*_rn intrinsics), and a row carries the
// same bits from both kernels because both run this text under that flag.
//
// A kernel decides which row a lane owns and where its three points come from; everything behind that is here, once.  All of it
// inlines: a point or a normal is handed over as a pointer to three floats, and they stay in registers.
#pragma once
#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

#include "../../include/nsdp_batch.h"
#include "common.h"

namespace nsdp {

__host__ __device__ __forceinline__ long long clampll(long long v, long long lo, long long hi) { return v < lo ? lo : (v > hi ? hi : v); }

inline bool aligned(const void *p, size_t to) { return reinterpret_cast<uintptr_t>(p) % to == 0; }

// what both launches are told about the rows they write: the member both kernels' argument structs embed
struct RowArgs {
  const float *noise;      // [B, n, 3] or null
  float *surface_out, *inputs_out, *space_out;
  uint8_t *handle_out;
  float partial_range, noise_level;
};

// the part of the canonical frame's box that the handle rule reads: words 3..5 of a frame-table entry hold (min_x, min_y),
// (min_z, max_x), (max_y, max_z) as fp32 bits -- in both table layouts
struct CanoBox { float min_y, min_z, max_y; };

__device__ __forceinline__ CanoBox cano_box(int64_t w3, int64_t w4, int64_t w5) {
  CanoBox box;
  box.min_y = __uint_as_float(static_cast<uint32_t>(static_cast<uint64_t>(w3) >> 32));
  box.min_z = __uint_as_float(static_cast<uint32_t>(static_cast<uint64_t>(w4) & 0xFFFFFFFFu));
  box.max_y = __uint_as_float(static_cast<uint32_t>(static_cast<uint64_t>(w5) & 0xFFFFFFFFu));
  return box;
}

// the reference's handle rule on a canonical point: near the box's low y, its high y or its low z
__device__ __forceinline__ bool is_handle(const float *cano, const CanoBox &box, float partial_range) {
  const bool head = cano[1] < __fadd_rn(box.min_y, partial_range);
  const bool tail = cano[1] > __fsub_rn(box.max_y, partial_range);
  const bool foot = cano[2] < __fadd_rn(box.min_z, partial_range);
  return head | tail | foot;
}

// The 7-wide input row [src | tgt * mask | mask] at `in`: ONE multiply per target component (-x * 0 = -0), whoever writes the row
// (write_surface_row below for sampled rows, mesh_whole.hip for whole meshes).
__device__ __forceinline__ void write_inputs_row(float *in, const float *sp, const float *tp, bool handle) {
  const float mf = handle ? 1.f : 0.f;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    in[k] = sp[k];
    in[3 + k] = __fmul_rn(tp[k], mf);
  }
  in[6] = mf;
}

// Surface row `row` (= b * n + j) of a batch of B x n: the six planes of [6, B, n, 3] (points, then normals, of the canonical,
// source and target frame), the mask byte of [B, n, 1] and the input row [src | tgt * mask | mask] of [B, n, 7], the source
// point with `noise_level * noise[row]` added -- in `sp` itself, which the caller gives up: a copy of it costs the pool kernel two
// registers.  12 and 28 contiguous bytes per lane at a stride of the same size.
__device__ __forceinline__ void write_surface_row(const RowArgs &a, int B, int n, size_t row, const CanoBox &box, const float *cp,
                                                  const float *cn, float *sp, const float *sn, const float *tp,
                                                  const float *tn) {
  if (a.noise) {
    const float *z = a.noise + row * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) sp[k] = __fadd_rn(sp[k], __fmul_rn(a.noise_level, z[k]));
  }
  const bool handle = is_handle(cp, box, a.partial_range);
  const size_t plane = static_cast<size_t>(B) * n * 3;
  float *o = a.surface_out + row * 3;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    o[k] = cp[k];
    o[plane + k] = sp[k];
    o[2 * plane + k] = tp[k];
    o[3 * plane + k] = cn[k];
    o[4 * plane + k] = sn[k];
    o[5 * plane + k] = tn[k];
  }
  a.handle_out[row] = handle ? 1 : 0;
  write_inputs_row(a.inputs_out + row * 7, sp, tp, handle);
}

// Space row `row` (= b * m + j) of a batch of B x m: the three planes of [3, B, m, 3].
__device__ __forceinline__ void write_space_row(const RowArgs &a, int B, int m, size_t row, const float *c, const float *s,
                                                const float *t) {
  const size_t plane = static_cast<size_t>(B) * m * 3;
  float *o = a.space_out + row * 3;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    o[k] = c[k];
    o[plane + k] = s[k];
    o[2 * plane + k] = t[k];
  }
}

// ---- the argument checks both entries open with, `entry` being the name an error message starts with.  An entry judges sizes
// before values before pointers before alignment: batch_sizes_ok, its own sizes, batch_values_ok, its own values, and, once it has
// returned for an empty batch, its pointers (the messages name each entry's own operands) with the two predicates below.
inline int batch_sizes_ok(const char *entry, int B, int n, int m, int n_frames) {
  NSDP_REQUIRE(B >= 0 && B <= 65535, "%s: batch B=%d outside [0, 65535]", entry, B);
  NSDP_REQUIRE(n >= 0 && n <= NSDP_BATCH_MAX_ROWS, "%s: n=%d surface rows outside [0, %d]", entry, n, NSDP_BATCH_MAX_ROWS);
  NSDP_REQUIRE(m >= 0 && m <= NSDP_BATCH_MAX_ROWS, "%s: m=%d space rows outside [0, %d]", entry, m, NSDP_BATCH_MAX_ROWS);
  NSDP_REQUIRE(static_cast<long long>(B) * (n > m ? n : m) < (1LL << 27), "%s: B=%d x max(n=%d, m=%d) rows too large", entry, B, n, m);
  NSDP_REQUIRE(n_frames >= 1, "%s: n_frames=%d, the frame table needs a frame", entry, n_frames);
  return 0;
}

inline int batch_values_ok(const char *entry, const RowArgs &a) {
  NSDP_REQUIRE(finite_weight(a.partial_range), "%s: partial_range is not finite", entry);
  NSDP_REQUIRE(finite_weight(a.noise_level), "%s: noise_level is not finite", entry);
  return 0;
}

inline bool surface_outputs_given(const RowArgs &a) { return a.surface_out && a.handle_out && a.inputs_out; }

// (the noise and the fp32 outputs; a null pointer is aligned)
inline bool rows_aligned(const RowArgs &a) {
  return aligned(a.noise, 4) && aligned(a.surface_out, 4) && aligned(a.inputs_out, 4) && aligned(a.space_out, 4);
}

}  // namespace nsdp
