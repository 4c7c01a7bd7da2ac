// Device helpers shared by the bf16-matrix-pipe kernels (x3_kernel.h, wgrad_bf16x3.hip, gemm_bf16.hip), the decoder chains
// (chain_f32.h) and the weight packs (pack_bodies.h): the vector types, the three-plane bf16 split, the MFMA wrapper, the
// compile-time loop and the hand-placed LDS reads with their wait.  Helpers that only one file uses stay in that file.
#pragma once
#include <type_traits>

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;
using f32x2 = __attribute__((ext_vector_type(2))) float;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned;
using bf16x2 = __attribute__((ext_vector_type(2))) __bf16;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;

// two fp32 values -> the packed (lo, hi) bf16 pairs of their three split planes (round to nearest, exact residuals)
__device__ __forceinline__ void split3(float x0, float x1, unsigned &h, unsigned &m, unsigned &l) {
  h = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{x0, x1}, bf16x2));
  const float r0 = x0 - __builtin_bit_cast(float, h << 16), r1 = x1 - __builtin_bit_cast(float, h & 0xffff0000u);
  m = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{r0, r1}, bf16x2));
  const float s0 = r0 - __builtin_bit_cast(float, m << 16), s1 = r1 - __builtin_bit_cast(float, m & 0xffff0000u);
  l = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{s0, s1}, bf16x2));
}

__device__ __forceinline__ f32x4 mfma_bf16(u32x4 a, u32x4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

template <int I, int N, typename F>
__device__ __forceinline__ void static_for(F &&f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}

// Fragments come back from LDS through hand-placed reads (the compiler sinks ordinary LDS loads below the MFMA block of a
// step, exposing their latency every step); lgkmcnt is awaited by hand, the fragment registers being in/out operands of the
// wait so that their users depend on it.
template <int OFF>
__device__ __forceinline__ void lds_read(u32x4 &dst, unsigned lane_addr) {
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(lane_addr), "n"(OFF));
}
// (lane i of a 16-lane group gets column i of the 4 x 16 bf16 block the group's lanes address: half an operand of a transpose)
template <int OFF>
__device__ __forceinline__ void tr_read(unsigned long long &dst, unsigned addr) {
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF));
}
__device__ __forceinline__ void lds_wait3(u32x4 &a, u32x4 &b, u32x4 &c) {
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a), "+v"(b), "+v"(c));
}

}  // namespace
