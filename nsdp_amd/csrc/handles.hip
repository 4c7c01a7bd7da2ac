// User-handle drags on the device (include/nsdp_handles.h): the bounding box of a cloud, and per point the reference's
// handle rule (dataset/utils.py: cano_handle_user_define), the dragged target and columns 3..6 of the deformation network's
// input rows -- with the drag parameters read from device memory, so that a captured graph serves every drag.
//
// This file is the RECTANGULAR layout: B shapes of n points each, row p = b * n + i.  What a workgroup does with its shape's
// points and what a lane does with its row -- the keys and their reductions, the final-bounds kernel, the rule, the target and
// the stores -- is handles_rule.h, shared with handles_ragged.hip; here are the two kernels that name the rows, the argument
// checks and the launches.
//
//   bounds   partial: grid (G, B), G = ceil(n / kPointsPerGroup); workgroup (g, b) reduces its share of shape b to six keys in
//            the workspace.  G <= ceil(n / kThreads), so every workgroup owns at least one point.
//            final: one wave per shape reduces the G partials and stores the six floats.
//   rows     one lane per point, grid (ceil(n / kThreads), B).
//
// Built with -ffp-contract=off, as handles_rule.h requires: one rounding per operation, no fused multiply-add.
#include "handles_rule.h"

namespace {

constexpr int kMaxGroups = 256;            // n = 2^20 at kPointsPerGroup
static_assert(kMaxPoints / kPointsPerGroup == kMaxGroups, "the largest cloud takes the largest grid");

inline bool refused(int B, int n) { return B < 1 || B > 65535 || n < 1 || n > kMaxPoints; }

inline int groups_of(int n) { return nsdp::ceil_div(n, kPointsPerGroup); }

__global__ __launch_bounds__(kThreads) void handle_bounds_partial_kernel(const float *__restrict__ cano_all, int n, int G,
                                                                         uint32_t *__restrict__ part_all) {
  const int b = blockIdx.y, g = blockIdx.x;
  bounds_partial(cano_all + static_cast<long long>(b) * n * 3, n, g, G, part_all + (static_cast<long long>(b) * G + g) * 6);
}

template <bool MASKS>
__global__ __launch_bounds__(kThreads) void handle_rows_kernel(const float *__restrict__ cano_all, const float *__restrict__ src_all,
                                                               const float *__restrict__ bounds_all,
                                                               const uint32_t *__restrict__ params_all,
                                                               const uint8_t *__restrict__ handle_mask,
                                                               const uint8_t *__restrict__ move_mask, int n,
                                                               float *__restrict__ rows_all, float *__restrict__ tgt_all,
                                                               uint8_t *__restrict__ handle_out, uint8_t *__restrict__ move_out) {
  const int b = blockIdx.y;
  const long long il = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x;
  if (il >= n) return;
  const long long p = static_cast<long long>(b) * n + il;      // the point's row in every (B, n, .) operand
  handle_row<MASKS>(p, b, cano_all, src_all, bounds_all, params_all, handle_mask, move_mask, rows_all, tgt_all, handle_out, move_out);
}

}  // namespace

extern "C" size_t nsdp_handle_bounds_workspace_bytes(int B, int n) {
  if (refused(B, n)) return 0;
  return static_cast<size_t>(B) * groups_of(n) * 6 * sizeof(uint32_t);
}

extern "C" int nsdp_handle_bounds(const float *cano, int B, int n, void *workspace, float *bounds, void *stream) {
  NSDP_REQUIRE(B >= 1 && B <= 65535, "handle_bounds: batch %d must be in [1, 65535]", B);
  NSDP_REQUIRE(n >= 1 && n <= kMaxPoints, "handle_bounds: n=%d points per shape must be in [1, %d]", n, kMaxPoints);
  NSDP_REQUIRE(cano && bounds, "handle_bounds: null pointer");
  NSDP_REQUIRE(workspace, "handle_bounds: null workspace pointer");
  NSDP_REQUIRE(!misaligned4(cano) && !misaligned4(bounds) && !misaligned4(workspace),
               "handle_bounds: cano, bounds and the workspace must be 4-byte aligned");
  hipStream_t st = nsdp::as_stream(stream);
  const int G = groups_of(n);
  uint32_t *part = static_cast<uint32_t *>(workspace);
  int rc;
  hipLaunchKernelGGL(handle_bounds_partial_kernel, dim3(G, B), dim3(kThreads), 0, st, cano, n, G, part);
  if ((rc = nsdp::launch_status("handle_bounds_partial_kernel"))) return rc;
  hipLaunchKernelGGL(handle_bounds_final_kernel, dim3(B), dim3(64), 0, st, part, G, bounds);
  return nsdp::launch_status("handle_bounds_final_kernel");
}

extern "C" int nsdp_handle_rows(const float *cano, const float *src, const float *bounds, const uint32_t *params,
                                const uint8_t *handle_mask, const uint8_t *move_mask, int B, int n, float *rows, float *tgt,
                                uint8_t *handle_out, uint8_t *move_out, void *stream) {
  NSDP_REQUIRE(B >= 1 && B <= 65535, "handle_rows: batch %d must be in [1, 65535]", B);
  NSDP_REQUIRE(n >= 1 && n <= kMaxPoints, "handle_rows: n=%d points per shape must be in [1, %d]", n, kMaxPoints);
  NSDP_REQUIRE((handle_mask == nullptr) == (move_mask == nullptr),
               "handle_rows: handle_mask and move_mask go together (both null: the rule decides)");
  const bool masks = handle_mask != nullptr;
  NSDP_REQUIRE(src && params && rows, "handle_rows: null pointer (src, params and rows are required)");
  NSDP_REQUIRE(masks || (cano && bounds), "handle_rows: null pointer (the rule reads cano and bounds)");
  NSDP_REQUIRE(!misaligned4(cano) && !misaligned4(src) && !misaligned4(bounds) && !misaligned4(params) && !misaligned4(rows) &&
                   !misaligned4(tgt),
               "handle_rows: the 32-bit operands must be 4-byte aligned");
  hipStream_t st = nsdp::as_stream(stream);
  const dim3 grid(nsdp::ceil_div(n, kThreads), B);
  if (masks)
    hipLaunchKernelGGL(handle_rows_kernel<true>, grid, dim3(kThreads), 0, st, cano, src, bounds, params, handle_mask, move_mask, n,
                       rows, tgt, handle_out, move_out);
  else
    hipLaunchKernelGGL(handle_rows_kernel<false>, grid, dim3(kThreads), 0, st, cano, src, bounds, params, handle_mask, move_mask, n,
                       rows, tgt, handle_out, move_out);
  return nsdp::launch_status("handle_rows_kernel");
}
