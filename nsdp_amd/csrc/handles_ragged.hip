// User-handle drags over a packed batch of meshes of different sizes (include/nsdp_handles_ragged.h).  This file is the PACKED
// layout: each shape's rows are read from offsets(B+1) on the device instead of a rectangle.  What a workgroup does with its
// shape's rows and what a lane does with its row is handles_rule.h, the text handles.hip runs; the offsets -- a shape's clamped
// range, a row's owner -- are packed_rows.h, shared with handle_sets.hip; here are the two kernels that name the rows, the
// argument checks and the launches.
//
//   bounds   partial: grid (G, B), G = ceil(n_max / kPointsPerGroup).  Workgroup (g, b) reads shape b's range from the offsets
//            and reduces its share to six keys; where its share is empty (a short or an empty shape) the keys it writes are the
//            identities, so all B * G * 6 words are written.
//            final: handles_rule.h's kernel.  An empty shape gets the identities as floats.
//   rows     one lane per packed row, grid ceil(cap / kThreads).  The wave's first row looks its shape up by a binary search of
//            the clamped offsets with uniform (scalar) loads; lanes whose row lies outside that shape search for themselves.
//            A row no shape owns (padding) returns before any store.
//
// Built with -ffp-contract=off, as handles_rule.h requires: a row carries the bits the rectangular entry gives it on its shape
// alone because both files compile one text of the rule under one flag.
#include "handles_rule.h"
#include "packed_rows.h"      // a shape's clamped range, a row's owner

namespace {

inline bool refused(int B, int cap, int n_max) { return B < 1 || B > 65535 || cap < 1 || n_max < 1 || n_max > kMaxPoints; }

inline int groups_of(int n_max) { return nsdp::ceil_div(n_max, kPointsPerGroup); }

__global__ __launch_bounds__(kThreads) void handle_bounds_ragged_partial_kernel(const float *__restrict__ cano,
                                                                                const int32_t *__restrict__ offsets, int cap,
                                                                                int n_max, int G, uint32_t *__restrict__ part_all) {
  const int b = blockIdx.y, g = blockIdx.x;
  int first, end;
  shape_range(offsets, b, cap, first, end);
  // (rows first .. first + n - 1 lie below end <= cap)
  bounds_partial(cano + static_cast<long long>(first) * 3, min(end - first, n_max), g, G,
                 part_all + (static_cast<long long>(b) * G + g) * 6);
}

template <bool MASKS>
__global__ __launch_bounds__(kThreads) void handle_rows_ragged_kernel(
    const float *__restrict__ cano_all, const float *__restrict__ src_all, const int32_t *__restrict__ offsets,
    const float *__restrict__ bounds_all, const uint32_t *__restrict__ params_all, const uint8_t *__restrict__ handle_mask,
    const uint8_t *__restrict__ move_mask, int B, int cap, float *__restrict__ rows_all, float *__restrict__ tgt_all,
    uint8_t *__restrict__ handle_out, uint8_t *__restrict__ move_out) {
  const long long p = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x;
  if (p >= cap) return;
  int b;
  if (!owner_of_lane(offsets, B, cap, p, b)) return;
  handle_row<MASKS>(p, b, cano_all, src_all, bounds_all, params_all, handle_mask, move_mask, rows_all, tgt_all, handle_out, move_out);
}

}  // namespace

extern "C" size_t nsdp_handle_bounds_ragged_workspace_bytes(int B, int cap, int n_max) {
  if (refused(B, cap, n_max)) return 0;
  return static_cast<size_t>(B) * groups_of(n_max) * 6 * sizeof(uint32_t);
}

extern "C" int nsdp_handle_bounds_ragged(const float *cano, const int32_t *offsets, int B, int cap, int n_max, void *workspace,
                                         float *bounds, void *stream) {
  NSDP_REQUIRE(B >= 1 && B <= 65535, "handle_bounds_ragged: batch %d must be in [1, 65535]", B);
  NSDP_REQUIRE(cap >= 1, "handle_bounds_ragged: cap=%d packed rows must be at least 1", cap);
  NSDP_REQUIRE(n_max >= 1 && n_max <= kMaxPoints, "handle_bounds_ragged: n_max=%d rows per shape must be in [1, %d]", n_max,
               kMaxPoints);
  NSDP_REQUIRE(cano && offsets && bounds, "handle_bounds_ragged: null pointer");
  NSDP_REQUIRE(workspace, "handle_bounds_ragged: null workspace pointer");
  NSDP_REQUIRE(!misaligned4(cano) && !misaligned4(offsets) && !misaligned4(bounds) && !misaligned4(workspace),
               "handle_bounds_ragged: cano, offsets, bounds and the workspace must be 4-byte aligned");
  hipStream_t st = nsdp::as_stream(stream);
  const int G = groups_of(n_max);
  uint32_t *part = static_cast<uint32_t *>(workspace);
  int rc;
  hipLaunchKernelGGL(handle_bounds_ragged_partial_kernel, dim3(G, B), dim3(kThreads), 0, st, cano, offsets, cap, n_max, G, part);
  if ((rc = nsdp::launch_status("handle_bounds_ragged_partial_kernel"))) return rc;
  hipLaunchKernelGGL(handle_bounds_final_kernel, dim3(B), dim3(64), 0, st, part, G, bounds);
  return nsdp::launch_status("handle_bounds_final_kernel");
}

extern "C" int nsdp_handle_rows_ragged(const float *cano, const float *src, const int32_t *offsets, const float *bounds,
                                       const uint32_t *params, const uint8_t *handle_mask, const uint8_t *move_mask, int B,
                                       int cap, float *rows, float *tgt, uint8_t *handle_out, uint8_t *move_out, void *stream) {
  NSDP_REQUIRE(B >= 1 && B <= 65535, "handle_rows_ragged: batch %d must be in [1, 65535]", B);
  NSDP_REQUIRE(cap >= 1, "handle_rows_ragged: cap=%d packed rows must be at least 1", cap);
  NSDP_REQUIRE((handle_mask == nullptr) == (move_mask == nullptr),
               "handle_rows_ragged: handle_mask and move_mask go together (both null: the rule decides)");
  const bool masks = handle_mask != nullptr;
  NSDP_REQUIRE(src && offsets && params && rows, "handle_rows_ragged: null pointer (src, offsets, params and rows are required)");
  NSDP_REQUIRE(masks || (cano && bounds), "handle_rows_ragged: null pointer (the rule reads cano and bounds)");
  NSDP_REQUIRE(!misaligned4(cano) && !misaligned4(src) && !misaligned4(offsets) && !misaligned4(bounds) && !misaligned4(params) &&
                   !misaligned4(rows) && !misaligned4(tgt),
               "handle_rows_ragged: the 32-bit operands must be 4-byte aligned");
  hipStream_t st = nsdp::as_stream(stream);
  const dim3 grid(nsdp::ceil_div(cap, kThreads));
  if (masks)
    hipLaunchKernelGGL(handle_rows_ragged_kernel<true>, grid, dim3(kThreads), 0, st, cano, src, offsets, bounds, params, handle_mask,
                       move_mask, B, cap, rows, tgt, handle_out, move_out);
  else
    hipLaunchKernelGGL(handle_rows_ragged_kernel<false>, grid, dim3(kThreads), 0, st, cano, src, offsets, bounds, params, handle_mask,
                       move_mask, B, cap, rows, tgt, handle_out, move_out);
  return nsdp::launch_status("handle_rows_ragged_kernel");
}
