// Labelled handle sets on the device (include/nsdp_handle_sets.h): per point a label, per (pose, shape, handle) a 3 x 4 motion
// -- or per point a target -- and from them the targets, the handle flags and columns 3..6 of the deformation network's input
// rows, for T poses of one source in one launch.
//
// The row body is handle_set_row.h; here are the two kernels that name a lane's rows, the argument checks and the launches.
//
//   rectangular   grid (ceil(n / kThreads), T * B), one lane per (pose, shape, point).  blockIdx.y = t * B + b names the output
//                 rows' rectangle and the motion table, b the source's: both uniform.  The lanes of pose 0 write handle_out.
//   packed        grid ceil(cap / kThreads), one lane per packed row, one pose.  A row's shape comes from packed_rows.h, the
//                 search handles_ragged.hip runs; a row no shape owns returns before any load of src or labels and any store.
//
// The kernel is a stream -- 13 to 25 bytes in, up to 41 out per row and pose -- and at an editing session's sizes a launch:
// nothing here uses LDS, and a lane does one row.
//
// Built with -ffp-contract=off, as handle_set_row.h requires: one rounding per operation, no fused multiply-add.
#include "handle_set_row.h"
#include "packed_rows.h"

#include "../../include/nsdp_handle_sets.h"

namespace {

constexpr int kMaxPoints = 1 << 20;
constexpr int kMaxGridY = 65535;
constexpr int kMaxHandles = 255;
constexpr int kThreads = 256;

inline bool misaligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3) != 0; }

template <bool TARGETS>
__global__ __launch_bounds__(kThreads) void handle_set_rows_kernel(const float *__restrict__ src_all, const uint8_t *__restrict__ labels,
                                                                   const float *__restrict__ motions,
                                                                   const float *__restrict__ targets_all, int B, int n, int H,
                                                                   float *__restrict__ rows_all, float *__restrict__ tgt_all,
                                                                   uint8_t *__restrict__ handle_out) {
  const int tb = blockIdx.y, b = tb % B;      // pose-major: tb = t * B + b
  const long long il = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x;
  if (il >= n) return;
  const long long ps = static_cast<long long>(b) * n + il;       // the point's row in src, labels and handle_out
  const long long po = static_cast<long long>(tb) * n + il;      // and in rows, tgt and targets
  const float *table = TARGETS ? nullptr : motions + static_cast<long long>(tb) * H * 12;
  handle_set_row<TARGETS>(ps, po, src_all, labels, table, targets_all, H, rows_all, tgt_all, tb < B ? handle_out : nullptr);
}

template <bool TARGETS>
__global__ __launch_bounds__(kThreads) void handle_set_rows_ragged_kernel(
    const float *__restrict__ src_all, const int32_t *__restrict__ offsets, const uint8_t *__restrict__ labels,
    const float *__restrict__ motions, const float *__restrict__ targets_all, int B, int cap, int H, float *__restrict__ rows_all,
    float *__restrict__ tgt_all, uint8_t *__restrict__ handle_out) {
  const long long p = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x;
  if (p >= cap) return;
  int b;
  if (!owner_of_lane(offsets, B, cap, p, b)) return;
  const float *table = TARGETS ? nullptr : motions + static_cast<long long>(b) * H * 12;
  handle_set_row<TARGETS>(p, p, src_all, labels, table, targets_all, H, rows_all, tgt_all, handle_out);
}

}  // namespace

extern "C" int nsdp_handle_set_rows(const float *src, const uint8_t *labels, const float *motions, const float *targets, int B, int n,
                                    int H, int T, float *rows, float *tgt, uint8_t *handle_out, void *stream) {
  NSDP_REQUIRE(B >= 1 && B <= kMaxGridY, "handle_set_rows: batch %d must be in [1, %d]", B, kMaxGridY);
  NSDP_REQUIRE(T >= 1 && T <= kMaxGridY, "handle_set_rows: T=%d poses must be in [1, %d]", T, kMaxGridY);
  NSDP_REQUIRE(static_cast<long long>(T) * B <= kMaxGridY, "handle_set_rows: T*B=%lld (pose, shape) pairs must be at most %d",
               static_cast<long long>(T) * B, kMaxGridY);
  NSDP_REQUIRE(n >= 1 && n <= kMaxPoints, "handle_set_rows: n=%d points per shape must be in [1, %d]", n, kMaxPoints);
  NSDP_REQUIRE((motions == nullptr) != (targets == nullptr),
               "handle_set_rows: exactly one of motions and targets (got %s)", motions ? "both" : "neither");
  NSDP_REQUIRE(targets || (H >= 1 && H <= kMaxHandles), "handle_set_rows: H=%d handles must be in [1, %d] with motions", H,
               kMaxHandles);
  NSDP_REQUIRE(src && labels && rows, "handle_set_rows: null pointer (src, labels and rows are required)");
  NSDP_REQUIRE(!misaligned4(src) && !misaligned4(motions) && !misaligned4(targets) && !misaligned4(rows) && !misaligned4(tgt),
               "handle_set_rows: the 32-bit operands must be 4-byte aligned");
  hipStream_t st = nsdp::as_stream(stream);
  const dim3 grid(nsdp::ceil_div(n, kThreads), T * B);
  if (targets)
    hipLaunchKernelGGL(handle_set_rows_kernel<true>, grid, dim3(kThreads), 0, st, src, labels, motions, targets, B, n, H, rows, tgt,
                       handle_out);
  else
    hipLaunchKernelGGL(handle_set_rows_kernel<false>, grid, dim3(kThreads), 0, st, src, labels, motions, targets, B, n, H, rows, tgt,
                       handle_out);
  return nsdp::launch_status("handle_set_rows_kernel");
}

extern "C" int nsdp_handle_set_rows_ragged(const float *src, const int32_t *offsets, const uint8_t *labels, const float *motions,
                                           const float *targets, int B, int cap, int H, float *rows, float *tgt,
                                           uint8_t *handle_out, void *stream) {
  NSDP_REQUIRE(B >= 1 && B <= kMaxGridY, "handle_set_rows_ragged: batch %d must be in [1, %d]", B, kMaxGridY);
  NSDP_REQUIRE(cap >= 1, "handle_set_rows_ragged: cap=%d packed rows must be at least 1", cap);
  NSDP_REQUIRE((motions == nullptr) != (targets == nullptr),
               "handle_set_rows_ragged: exactly one of motions and targets (got %s)", motions ? "both" : "neither");
  NSDP_REQUIRE(targets || (H >= 1 && H <= kMaxHandles), "handle_set_rows_ragged: H=%d handles must be in [1, %d] with motions", H,
               kMaxHandles);
  NSDP_REQUIRE(src && offsets && labels && rows,
               "handle_set_rows_ragged: null pointer (src, offsets, labels and rows are required)");
  NSDP_REQUIRE(!misaligned4(src) && !misaligned4(offsets) && !misaligned4(motions) && !misaligned4(targets) && !misaligned4(rows) &&
                   !misaligned4(tgt),
               "handle_set_rows_ragged: the 32-bit operands must be 4-byte aligned");
  hipStream_t st = nsdp::as_stream(stream);
  const dim3 grid(nsdp::ceil_div(cap, kThreads));
  if (targets)
    hipLaunchKernelGGL(handle_set_rows_ragged_kernel<true>, grid, dim3(kThreads), 0, st, src, offsets, labels, motions, targets, B,
                       cap, H, rows, tgt, handle_out);
  else
    hipLaunchKernelGGL(handle_set_rows_ragged_kernel<false>, grid, dim3(kThreads), 0, st, src, offsets, labels, motions, targets, B,
                       cap, H, rows, tgt, handle_out);
  return nsdp::launch_status("handle_set_rows_ragged_kernel");
}
