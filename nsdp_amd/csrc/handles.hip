// User-handle drags on the device (include/nsdp_handles.h): the bounding box of a cloud, and per point the reference's
// handle rule (dataset/utils.py: cano_handle_user_define), the dragged target and columns 3..6 of the deformation network's
// input rows -- with the drag parameters read from device memory, so that a captured graph serves every drag.
//
//   bounds   partial: grid (G, B), G = ceil(n / kPointsPerGroup) capped at kMaxGroups.  A workgroup strides over its shape's
//            points, keeps six running extremes per lane as order-preserving integer keys of the fp32 bits, reduces them over
//            the wave by shuffles and over its four waves through LDS, and writes its six keys to the workspace.  G <= ceil(n /
//            kThreads), so every workgroup owns at least one point and every workspace word is written.
//            final: one wave per shape reduces the G partials and stores the six floats.
//            Integer min / max on the keys is a total order: the result is the same for every split of the points.
//   rows     one lane per point, grid (ceil(n / kThreads), B).  The shape's parameters and bounds are uniform loads; the point's
//            rows are 12-byte loads and the stores are per-dword vector stores (a [n, 7] row is 28 bytes: columns 3..6 of it are
//            never 16-byte aligned for every row).
//
// This file is built with -ffp-contract=off and the arithmetic is spelled with the __f*_rn intrinsics: one rounding per
// operation, no fused multiply-add, and the products by 0.0f / 1.0f are real multiplications (0 * NaN = NaN, -0.15f * 0 = -0).
#include "common.h"

#include "../../include/nsdp_handles.h"

namespace {

constexpr int kMaxPoints = 1 << 20;
constexpr int kThreads = 256;
constexpr int kPointsPerGroup = 4096;      // sixteen points per lane
constexpr int kMaxGroups = 256;            // n = 2^20 at kPointsPerGroup
static_assert(kMaxPoints / kPointsPerGroup == kMaxGroups, "the largest cloud takes the largest grid");

inline bool refused(int B, int n) { return B < 1 || B > 65535 || n < 1 || n > kMaxPoints; }

inline int groups_of(int n) {
  const int g = nsdp::ceil_div(n, kPointsPerGroup);
  return g < kMaxGroups ? g : kMaxGroups;
}

// fp32 bits -> unsigned key with key(a) < key(b) exactly when a sorts before b (negative values mirrored, -0 below +0)
__device__ __forceinline__ uint32_t key_of(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float value_of(uint32_t key) {
  return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
}

__device__ __forceinline__ void wave_extremes(uint32_t (&lo)[3], uint32_t (&hi)[3]) {
#pragma unroll
  for (int off = 32; off; off >>= 1) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      lo[c] = min(lo[c], static_cast<uint32_t>(__shfl_xor(static_cast<int>(lo[c]), off)));
      hi[c] = max(hi[c], static_cast<uint32_t>(__shfl_xor(static_cast<int>(hi[c]), off)));
    }
  }
}

__global__ __launch_bounds__(kThreads) void handle_bounds_partial_kernel(const float *__restrict__ cano_all, int n, int G,
                                                                         uint32_t *__restrict__ part_all) {
  __shared__ uint32_t red[kThreads / 64][6];
  const int b = blockIdx.y, g = blockIdx.x;
  const float *cano = cano_all + static_cast<long long>(b) * n * 3;
  uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
  for (long long i = static_cast<long long>(g) * kThreads + threadIdx.x; i < n; i += static_cast<long long>(G) * kThreads) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const uint32_t k = key_of(cano[i * 3 + c]);
      lo[c] = min(lo[c], k);
      hi[c] = max(hi[c], k);
    }
  }
  wave_extremes(lo, hi);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      red[wave][c] = lo[c];
      red[wave][3 + c] = hi[c];
    }
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int c = threadIdx.x;
    uint32_t v = red[0][c];
#pragma unroll
    for (int w = 1; w < kThreads / 64; ++w) v = c < 3 ? min(v, red[w][c]) : max(v, red[w][c]);
    part_all[(static_cast<long long>(b) * G + g) * 6 + c] = v;
  }
}

__global__ __launch_bounds__(64) void handle_bounds_final_kernel(const uint32_t *__restrict__ part_all, int G,
                                                                 float *__restrict__ bounds_all) {
  const int b = blockIdx.x;
  const uint32_t *part = part_all + static_cast<long long>(b) * G * 6;
  uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
  for (int g = threadIdx.x; g < G; g += 64) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      lo[c] = min(lo[c], part[g * 6 + c]);
      hi[c] = max(hi[c], part[g * 6 + 3 + c]);
    }
  }
  wave_extremes(lo, hi);
  if (threadIdx.x == 0) {
    float *bounds = bounds_all + static_cast<long long>(b) * 6;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      bounds[c] = value_of(lo[c]);
      bounds[3 + c] = value_of(hi[c]);
    }
  }
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
  const uint32_t *prm = params_all + static_cast<long long>(b) * NSDP_HANDLE_PARAM_WORDS;
  const float dx = __uint_as_float(prm[NSDP_HANDLE_DX]), dy = __uint_as_float(prm[NSDP_HANDLE_DY]),
              dz = __uint_as_float(prm[NSDP_HANDLE_DZ]);
  bool handle, move;
  if (MASKS) {
    handle = handle_mask[p] != 0;
    move = move_mask[p] != 0;
  } else {
    const int part = static_cast<int>(prm[NSDP_HANDLE_PART]);
    const bool clip = prm[NSDP_HANDLE_CLIPTAIL] != 0;
    const float r = __uint_as_float(prm[NSDP_HANDLE_RANGE]);
    const float *bounds = bounds_all + static_cast<long long>(b) * 6;
    const float lo_y = bounds[1], lo_z = bounds[2], hi_y = bounds[4];
    const float x = cano_all[p * 3], y = cano_all[p * 3 + 1], z = cano_all[p * 3 + 2];
    const bool head = y < __fadd_rn(lo_y, r);
    bool tail = y > __fsub_rn(hi_y, r);
    if (clip) tail = tail && z > -r;
    const bool foot = z < __fadd_rn(lo_z, r);
    handle = head || tail || foot;
    const bool left = foot && x > 0.0f, right = foot && x < 0.0f, front = foot && y < 0.0f, behind = foot && y > 0.0f;
    switch (part) {
      case NSDP_HANDLE_HEAD: move = head; break;
      case NSDP_HANDLE_TAIL: move = tail; break;
      case NSDP_HANDLE_FRONTLEFTFOOT: move = left && front; break;
      case NSDP_HANDLE_FRONTRIGHTFOOT: move = right && front; break;
      case NSDP_HANDLE_BEHINDLEFTFOOT: move = left && behind; break;
      case NSDP_HANDLE_BEHINDRIGHTFOOT: move = right && behind; break;
      default: move = false; break;
    }
  }
  const float m = move ? 1.0f : 0.0f, h = handle ? 1.0f : 0.0f;
  const float tx = __fadd_rn(src_all[p * 3], __fmul_rn(dx, m));
  const float ty = __fadd_rn(src_all[p * 3 + 1], __fmul_rn(dy, m));
  const float tz = __fadd_rn(src_all[p * 3 + 2], __fmul_rn(dz, m));
  float *row = rows_all + p * 7;
  row[3] = __fmul_rn(tx, h);
  row[4] = __fmul_rn(ty, h);
  row[5] = __fmul_rn(tz, h);
  row[6] = h;
  if (tgt_all) {
    tgt_all[p * 3] = tx;
    tgt_all[p * 3 + 1] = ty;
    tgt_all[p * 3 + 2] = tz;
  }
  if (handle_out) handle_out[p] = handle ? 1 : 0;
  if (move_out) move_out[p] = move ? 1 : 0;
}

inline bool misaligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3) != 0; }

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
