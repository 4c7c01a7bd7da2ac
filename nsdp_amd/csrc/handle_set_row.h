// One row of a labelled handle set (include/nsdp_handle_sets.h): the label's verdict, the moved or copied target and columns
// 3..6 of the deformation network's input row.  Shared by the rectangular and the packed kernel of handle_sets.hip, which decide
// which source row `ps` and which output row `po` a lane owns and which motion table its (pose, shape) reads.
// Include it ONLY from translation units built with -ffp-contract=off: one rounding per operation.
//
// Loads and stores.  `table` is a uniform base (a kernel argument plus a blockIdx or readfirstlane product); the label picks a
// row of it per lane, so the twelve floats are vector loads from at most 255 * 48 bytes that every wave of the launch shares --
// cache hits after the first.  The point's rows are 12-byte loads.  A 7-float row is 28 bytes: columns 3..6 of it are never
// 16-byte aligned for every row, hence per-dword vector stores, as in handles_rule.h.  Spelled with the __f*_rn intrinsics: no
// fused multiply-add, and the products by 0.0f / 1.0f are real multiplications (0 * NaN = NaN, -0.15f * 0 = -0).
#pragma once

#include "common.h"

namespace {

__device__ __forceinline__ float motion_row(const float *__restrict__ m, float x, float y, float z) {
  return __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m[0], x), __fmul_rn(m[1], y)), __fmul_rn(m[2], z)), m[3]);
}

// TARGETS: `targets_all` holds the handle points' targets at the OUTPUT row and every non-zero label is a handle; otherwise
// `table` holds H motions and labels 1..H are handles (a label above H is a free point: nothing is read outside the table).
// `handle_out` is null for every pose but the first.
template <bool TARGETS>
__device__ __forceinline__ void handle_set_row(long long ps, long long po, const float *__restrict__ src_all,
                                               const uint8_t *__restrict__ labels, const float *__restrict__ table,
                                               const float *__restrict__ targets_all, int H, float *__restrict__ rows_all,
                                               float *__restrict__ tgt_all, uint8_t *__restrict__ handle_out) {
  const int label = labels[ps];
  const bool handle = TARGETS ? label != 0 : (label >= 1 && label <= H);
  const float x = src_all[ps * 3], y = src_all[ps * 3 + 1], z = src_all[ps * 3 + 2];
  float tx = x, ty = y, tz = z;      // a free point: its src row, copied
  if (handle) {
    if (TARGETS) {
      tx = targets_all[po * 3];
      ty = targets_all[po * 3 + 1];
      tz = targets_all[po * 3 + 2];
    } else {
      const float *m = table + (label - 1) * 12;
      tx = motion_row(m, x, y, z);
      ty = motion_row(m + 4, x, y, z);
      tz = motion_row(m + 8, x, y, z);
    }
  }
  const float h = handle ? 1.0f : 0.0f;
  float *row = rows_all + po * 7;
  row[3] = __fmul_rn(tx, h);
  row[4] = __fmul_rn(ty, h);
  row[5] = __fmul_rn(tz, h);
  row[6] = h;
  if (tgt_all) {
    tgt_all[po * 3] = tx;
    tgt_all[po * 3 + 1] = ty;
    tgt_all[po * 3 + 2] = tz;
  }
  if (handle_out) handle_out[ps] = handle ? 1 : 0;
}

}  // namespace
