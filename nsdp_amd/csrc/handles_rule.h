// What the two layouts of the user-handle drags share (handles.hip: a rectangle; handles_ragged.hip: packed rows): the handle
// rule and the dragged target of one row, the order-preserving keys of the bounding box with their reductions, and the limits.
// Include it ONLY from translation units built with -ffp-contract=off: the rule's arithmetic is one rounding per operation, and
// a row carries the same bits in both layouts because both run this text under that flag.
//
// A layout decides which row a lane owns and which shape that row belongs to; everything behind that is here, once.
#pragma once

#include "common.h"

#include "../../include/nsdp_handles.h"
#include "../../include/nsdp_handles_ragged.h"

namespace {

constexpr int kMaxPoints = 1 << 20;
constexpr int kThreads = 256;
constexpr int kPointsPerGroup = 4096;      // sixteen points per lane
constexpr uint32_t kKeyMax = 0xffffffffu, kKeyMin = 0u;      // the identities of min and max over the keys

inline bool misaligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3) != 0; }

// fp32 bits -> unsigned key with key(a) < key(b) exactly when a sorts before b (negative values mirrored, -0 below +0, NaNs
// outermost).  Integer min / max on the keys is a total order: a box is the same for every split of the points.
__device__ __forceinline__ uint32_t key_of(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float value_of(uint32_t key) {
  return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
}
// (what a shape without rows gets as its box)
static_assert(NSDP_HANDLE_BOUNDS_EMPTY_MIN_BITS == 0x7fffffffu && NSDP_HANDLE_BOUNDS_EMPTY_MAX_BITS == 0xffffffffu,
              "value_of(kKeyMax) and value_of(kKeyMin)");

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

// The body of a partial-bounds kernel, for workgroup g of the G that share one shape (kThreads lanes, every lane of the
// workgroup calls it): strides over the shape's n rows from `cano` (its first row), keeps six running extremes per lane as keys,
// reduces them over the wave by shuffles and over the four waves through LDS, and writes six keys to `part`.  A workgroup
// without rows (n <= g * kThreads) writes the identities.
__device__ __forceinline__ void bounds_partial(const float *__restrict__ cano, int n, int g, int G, uint32_t *__restrict__ part) {
  __shared__ uint32_t red[kThreads / 64][6];
  uint32_t lo[3] = {kKeyMax, kKeyMax, kKeyMax}, hi[3] = {kKeyMin, kKeyMin, kKeyMin};
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
    part[c] = v;
  }
}

// One wave per shape reduces its G partials and stores the six floats (a shape without rows: the identities as floats).
__global__ __launch_bounds__(64) void handle_bounds_final_kernel(const uint32_t *__restrict__ part_all, int G,
                                                                 float *__restrict__ bounds_all) {
  const int b = blockIdx.x;
  const uint32_t *part = part_all + static_cast<long long>(b) * G * 6;
  uint32_t lo[3] = {kKeyMax, kKeyMax, kKeyMax}, hi[3] = {kKeyMin, kKeyMin, kKeyMin};
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

// Row p of shape b: the reference's handle rule (dataset/utils.py: cano_handle_user_define) or the caller's masks, the dragged
// target src + d * m and columns 3..6 of the deformation network's input row.  The shape's parameters and bounds are uniform
// loads; the point's rows are 12-byte loads and the stores are per-dword vector stores (a 7-float row is 28 bytes: columns
// 3..6 of it are never 16-byte aligned for every row).  Spelled with the __f*_rn intrinsics: no fused multiply-add, and the
// products by 0.0f / 1.0f are real multiplications (0 * NaN = NaN, -0.15f * 0 = -0).
template <bool MASKS>
__device__ __forceinline__ void handle_row(long long p, int b, const float *__restrict__ cano_all, const float *__restrict__ src_all,
                                           const float *__restrict__ bounds_all, const uint32_t *__restrict__ params_all,
                                           const uint8_t *__restrict__ handle_mask, const uint8_t *__restrict__ move_mask,
                                           float *__restrict__ rows_all, float *__restrict__ tgt_all,
                                           uint8_t *__restrict__ handle_out, uint8_t *__restrict__ move_out) {
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

}  // namespace
