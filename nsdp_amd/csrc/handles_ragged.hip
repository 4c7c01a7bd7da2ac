// User-handle drags over a packed batch of meshes of different sizes (include/nsdp_handles_ragged.h): the kernels of
// handles.hip with each shape's rows read from offsets(B+1) on the device instead of a rectangle.
//
//   bounds   partial: grid (G, B), G = ceil(n_max / kPointsPerGroup).  Workgroup (g, b) reads shape b's range from the offsets,
//            strides over its rows like the rectangular kernel and writes six order-preserving keys; where its share is empty
//            (a short or an empty shape) the keys it writes are the identities, so all B * G * 6 words are written.
//            final: one wave per shape reduces the G partials.  An empty shape gets the identities as floats.
//   rows     one lane per packed row, grid ceil(cap / kThreads).  The wave's first row looks its shape up by a binary search of
//            the clamped offsets with uniform (scalar) loads; lanes whose row lies outside that shape search for themselves.
//            A row no shape owns (padding) returns before any store.
//
// Built with -ffp-contract=off; the arithmetic is handles.hip's, spelled with the __f*_rn intrinsics, so a row carries the bits
// the rectangular entry gives it on its shape alone.
#include "common.h"

#include "../../include/nsdp_handles.h"
#include "../../include/nsdp_handles_ragged.h"

namespace {

constexpr int kMaxPoints = 1 << 20;
constexpr int kThreads = 256;
constexpr int kPointsPerGroup = 4096;      // sixteen points per lane
constexpr uint32_t kKeyMax = 0xffffffffu, kKeyMin = 0u;      // the identities of min and max over the keys

inline bool refused(int B, int cap, int n_max) { return B < 1 || B > 65535 || cap < 1 || n_max < 1 || n_max > kMaxPoints; }

inline int groups_of(int n_max) { return nsdp::ceil_div(n_max, kPointsPerGroup); }

// fp32 bits -> unsigned key with key(a) < key(b) exactly when a sorts before b (handles.hip's: -0 below +0, NaNs outermost)
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

__device__ __forceinline__ int clamped(int v, int lo, int hi) { return min(max(v, lo), hi); }

// Rows [first, end) of shape b (0 <= b < B): 0 <= first <= end <= cap whatever `offsets` holds.
__device__ __forceinline__ void shape_range(const int32_t *__restrict__ offsets, int b, int cap, int &first, int &end) {
  first = clamped(offsets[b], 0, cap);
  end = clamped(offsets[b + 1], first, cap);
}

__global__ __launch_bounds__(kThreads) void handle_bounds_ragged_partial_kernel(const float *__restrict__ cano,
                                                                                const int32_t *__restrict__ offsets, int cap,
                                                                                int n_max, int G, uint32_t *__restrict__ part_all) {
  __shared__ uint32_t red[kThreads / 64][6];
  const int b = blockIdx.y, g = blockIdx.x;
  int first, end;
  shape_range(offsets, b, cap, first, end);
  const int n = min(end - first, n_max);
  uint32_t lo[3] = {kKeyMax, kKeyMax, kKeyMax}, hi[3] = {kKeyMin, kKeyMin, kKeyMin};
  for (long long i = static_cast<long long>(g) * kThreads + threadIdx.x; i < n; i += static_cast<long long>(G) * kThreads) {
    const float *p = cano + (first + i) * 3;      // (first + i < end <= cap)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const uint32_t k = key_of(p[c]);
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

__global__ __launch_bounds__(64) void handle_bounds_ragged_final_kernel(const uint32_t *__restrict__ part_all, int G,
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
static_assert(NSDP_HANDLE_BOUNDS_EMPTY_MIN_BITS == 0x7fffffffu && NSDP_HANDLE_BOUNDS_EMPTY_MAX_BITS == 0xffffffffu,
              "value_of(kKeyMax) and value_of(kKeyMin)");

// The shape that owns packed row p: the last b in [0, B) whose clamped first row is <= p, if p is below that shape's clamped
// end.  Binary search for the first j in [1, B] with offsets[j] > p (B <= 65535: at most 16 steps).  false: no shape owns p.
__device__ __forceinline__ bool owner_of(const int32_t *__restrict__ offsets, int B, int cap, int p, int &b, int &first, int &end) {
  int lo = 1, hi = B + 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (clamped(offsets[mid], 0, cap) > p)
      hi = mid;
    else
      lo = mid + 1;
  }
  if (lo > B) return false;      // p is at or beyond offsets[B]
  b = lo - 1;
  shape_range(offsets, b, cap, first, end);
  return p >= first && p < end;
}

template <bool MASKS>
__global__ __launch_bounds__(kThreads) void handle_rows_ragged_kernel(
    const float *__restrict__ cano_all, const float *__restrict__ src_all, const int32_t *__restrict__ offsets,
    const float *__restrict__ bounds_all, const uint32_t *__restrict__ params_all, const uint8_t *__restrict__ handle_mask,
    const uint8_t *__restrict__ move_mask, int B, int cap, float *__restrict__ rows_all, float *__restrict__ tgt_all,
    uint8_t *__restrict__ handle_out, uint8_t *__restrict__ move_out) {
  const long long p = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x;
  if (p >= cap) return;
  // the wave's first row (always below cap here: lane 0 is the wave's lowest row), looked up with uniform loads
  const int p0 = __builtin_amdgcn_readfirstlane(static_cast<int>(p));
  int b = 0, first = 0, end = 0;
  bool owned = owner_of(offsets, B, cap, p0, b, first, end);
  b = __builtin_amdgcn_readfirstlane(b);
  if (!owned || p >= end) owned = owner_of(offsets, B, cap, static_cast<int>(p), b, first, end);
  if (!owned) return;
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
  hipLaunchKernelGGL(handle_bounds_ragged_final_kernel, dim3(B), dim3(64), 0, st, part, G, bounds);
  return nsdp::launch_status("handle_bounds_ragged_final_kernel");
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
