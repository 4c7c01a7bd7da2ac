// The transposed bf16-operand MFMA layer of the register-resident decoder chain (decoder_fused_bf16.hip): the layer of
// chain_f32.h with the two matrix operands rounded to bf16 and everything else -- accumulators, biases, residual adds -- kept
// in fp32.  One wave, 16 rows, Y^T = W X^T on v_mfma_f32_16x16x32_bf16.  Included after chain_f32.h (static_for, Steps, the
// hand-issued loads and pin() are shared).
//
// Operand layout.  The instruction's C/D layout is the fp32 one (column = lane & 15 = query row, row = 4 g + reg = channel
// 4 g + reg of the tile), and its B operand of lane (li, g) is k = 8 g + j, j < 8.  With the k permutation
//     hardware slot 8 g + j  <->  channel 16 t0 + 4 g + j (j < 4),  16 t1 + 4 g + (j - 4) (j >= 4)
// of a block of two neighbouring 16-channel tiles (t0, t1) = (2 kb, 2 kb + 1), the four fp32 accumulators of t0 followed by
// those of t1, converted pairwise with v_cvt_pk_bf16_f32 (round to nearest even), ARE lane (li, g)'s B fragment of k block kb:
// no lane movement between layers, as in the fp32 chain.  The weights are permuted the same way once on the host
// (hip_decoder._frag_bf16).  An odd tile count (208 = 13 tiles) ends with one v_mfma_f32_16x16x16_bf16 on the last tile
// alone (B = its four channels per lane, k = 4 g + j) rather than a zero-padded 14th tile: the chain is bound by the weight
// feed, and the half block is half the bytes.
//
// Weights: [out tile][k block][lane = 16 g + li][8] bf16 (1 KiB per block), the half block [lane][4] (512 B) last, so one out
// tile is NTIN * 512 bytes.

using u32x2 = __attribute__((ext_vector_type(2))) unsigned;      // (u32x4, bf16x8: mfma_util.h, through chain_f32.h)
using s16x4 = __attribute__((ext_vector_type(4))) short;

#ifndef NSDP_DEC16_PREFETCH
#define NSDP_DEC16_PREFETCH 6
#endif
#ifndef NSDP_DEC16_RING
#define NSDP_DEC16_RING 8
#endif
constexpr int kPrefetch16 = NSDP_DEC16_PREFETCH;   // steps (two fragments each) in flight ahead of the MFMAs
constexpr int kRing16 = NSDP_DEC16_RING;
static_assert(kPrefetch16 < kRing16, "a ring slot is reloaded only after its step has been consumed");

template <int IMM>
__device__ __forceinline__ void wload(u32x4 &dst, const void *uniform_base, unsigned lane_byte_off) {
  asm volatile("global_load_dwordx4 %0, %1, %2 offset:%3" : "=v"(dst) : "v"(lane_byte_off), "s"(uniform_base), "n"(IMM));
}
template <int IMM>
__device__ __forceinline__ void wload(u32x2 &dst, const void *uniform_base, unsigned lane_byte_off) {
  asm volatile("global_load_dwordx2 %0, %1, %2 offset:%3" : "=v"(dst) : "v"(lane_byte_off), "s"(uniform_base), "n"(IMM));
}
template <int N, typename T>
__device__ __forceinline__ void wwait(T &a, T &b) {
  asm volatile("s_waitcnt vmcnt(%2)" : "+v"(a), "+v"(b) : "n"(N));
}
template <int N, typename T>
__device__ __forceinline__ void wwait(T &a) {
  asm volatile("s_waitcnt vmcnt(%1)" : "+v"(a) : "n"(N));
}

// The B operand of a layer: an fp32 activation vector rounded to bf16, two tiles (one K = 32 block) per u32x4.  With an odd
// tile count the last entry holds the last tile in its low half (the K = 16 instruction reads only that).
template <int NT>
struct Packed {
  u32x4 b[(NT + 1) / 2];
};

__device__ __forceinline__ unsigned cvt_pk_bf16(float lo, float hi) {
  unsigned r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
  return r;
}

template <bool RELU>
__device__ __forceinline__ void cvt_tile(const f32x4 &v, unsigned &lo, unsigned &hi) {
  f32x4 x = v;
  if (RELU) { x[0] = fmaxf(x[0], 0.f); x[1] = fmaxf(x[1], 0.f); x[2] = fmaxf(x[2], 0.f); x[3] = fmaxf(x[3], 0.f); }
  lo = cvt_pk_bf16(x[0], x[1]);
  hi = cvt_pk_bf16(x[2], x[3]);
}

// C -> B: the only place an activation is rounded (after the ReLU where the layer has one).
template <int NT, bool RELU>
__device__ __forceinline__ void pack(const f32x4 *v, Packed<NT> &p) {
#pragma unroll
  for (int kb = 0; kb < NT / 2; ++kb) {
    unsigned a, b, c, d;
    cvt_tile<RELU>(v[2 * kb], a, b);
    cvt_tile<RELU>(v[2 * kb + 1], c, d);
    p.b[kb] = u32x4{a, b, c, d};
  }
  if constexpr (NT & 1) {
    unsigned a, b;
    cvt_tile<RELU>(v[NT - 1], a, b);
    p.b[NT / 2] = u32x4{a, b, 0u, 0u};
  }
}

// v_out[ot] = act( W[ot*16 + ., :] * x + bias )  for NTOUT output tiles, NTIN input tiles; ACC: v_out is also the start value
// (fused residual add, in fp32).  The step structure is Steps<NTOUT, k blocks> of chain_f32.h: a step feeds two independent
// accumulators with ONE MFMA each (the two tiles of a pair at the same k block; for the odd last tile the even and the odd k
// blocks of that tile, summed at the end).  A 16-cycle MFMA per KiB of weights is four times what the L2 -> register path of
// one wave per SIMD delivers, so the ring is what sets the pace: kPrefetch16 steps = 2 x kPrefetch16 KiB in flight per wave.
template <int NTOUT, int NTIN, bool RELU_OUT, bool ACC>
__device__ __forceinline__ void dense_bf16(const void *__restrict__ W, const float *__restrict__ bias, const Packed<NTIN> &x,
                                           f32x4 *v_out, int li, int g) {
  constexpr int NKB = (NTIN + 1) / 2;
  constexpr bool kHalf = (NTIN & 1) != 0;         // the last k block is one tile: K = 16
  using S = Steps<NTOUT, NKB>;
  const char *Wb = static_cast<const char *>(W);
  const unsigned lane = 16u * g + li;
  const unsigned wl = lane * 16u, wlh = lane * 8u;
  const unsigned bl = 16u * g;
  u32x4 ra[kRing16], rb[kRing16];
  u32x2 ha[kRing16], hb[kRing16];                 // (half blocks; only the slots of such steps exist after SROA)
  auto half = [](int kb) constexpr { return kHalf && kb == NKB - 1; };
  auto issue = [&](auto I) {
    constexpr int s = decltype(I)::value;
    constexpr int r = s % kRing16;
    const char *pa = Wb + (S::tile_a(s) * NTIN) * 512 + S::kb_a(s) * 1024;
    if constexpr (half(S::kb_a(s))) wload<0>(ha[r], pa, wlh); else wload<0>(ra[r], pa, wl);
    if constexpr (S::has_b(s)) {
      const char *pb = Wb + (S::tile_b(s) * NTIN) * 512 + S::kb_b(s) * 1024;
      if constexpr (half(S::kb_b(s))) wload<0>(hb[r], pb, wlh); else wload<0>(rb[r], pb, wl);
    }
  };
  auto mma = [&](auto KB, const auto &frag, f32x4 acc) -> f32x4 {
    constexpr int kb = decltype(KB)::value;
    if constexpr (half(kb)) {
      const u32x2 xb = u32x2{x.b[kb][0], x.b[kb][1]};
      return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(s16x4, frag), __builtin_bit_cast(s16x4, xb), acc, 0, 0, 0);
    } else {
      return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, frag), __builtin_bit_cast(bf16x8, x.b[kb]), acc, 0, 0, 0);
    }
  };
  constexpr int kPro = kPrefetch16 < S::kSteps ? kPrefetch16 : S::kSteps;
  static_for<0, kPro>(issue);
  float4 ba = ldg4(bias + S::tile_a(0) * 16, bl);
  float4 bb = ldg4(bias + S::tile_b(0) * 16, bl);
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  static_for<0, S::kSteps>([&](auto I) {
    constexpr int s = decltype(I)::value;
    constexpr int r = s % kRing16;
    if constexpr (s + kPrefetch16 < S::kSteps) issue(std::integral_constant<int, s + kPrefetch16>{});
    if constexpr (S::first(s)) {
      acc0 = ACC ? v_out[S::tile_a(s)] : f32x4{0.f, 0.f, 0.f, 0.f};
      acc0[0] += ba.x; acc0[1] += ba.y; acc0[2] += ba.z; acc0[3] += ba.w;
      if constexpr (S::tail(s)) {
        acc1 = f32x4{0.f, 0.f, 0.f, 0.f};
      } else {
        acc1 = ACC ? v_out[S::tile_b(s)] : f32x4{0.f, 0.f, 0.f, 0.f};
        acc1[0] += bb.x; acc1[1] += bb.y; acc1[2] += bb.z; acc1[3] += bb.w;
      }
      constexpr int sn = S::next_first(s);          // bias of the next accumulator group, one group ahead
      if constexpr (sn < S::kSteps) {
        ba = ldg4(bias + S::tile_a(sn) * 16, bl);
        bb = ldg4(bias + S::tile_b(sn) * 16, bl);
      }
    }
    constexpr int kYounger = S::loads_after(s, kPrefetch16);
    constexpr int kba = S::kb_a(s), kbb = S::kb_b(s);
    // one wait for both fragments of the step (their loads were issued back to back), then the independent MFMA pair
    if constexpr (S::has_b(s)) {
      if constexpr (half(kba) && half(kbb)) {
        wwait<kYounger>(ha[r], hb[r]);
      } else if constexpr (half(kbb)) {             // (tail step whose odd k block is the half one)
        wwait<kYounger>(hb[r]);
        wwait<kYounger>(ra[r]);
      } else {
        wwait<kYounger>(ra[r], rb[r]);
      }
      if constexpr (half(kba)) acc0 = mma(std::integral_constant<int, kba>{}, ha[r], acc0);
      else acc0 = mma(std::integral_constant<int, kba>{}, ra[r], acc0);
      if constexpr (half(kbb)) acc1 = mma(std::integral_constant<int, kbb>{}, hb[r], acc1);
      else acc1 = mma(std::integral_constant<int, kbb>{}, rb[r], acc1);
    } else {
      if constexpr (half(kba)) {
        wwait<kYounger>(ha[r]);
        acc0 = mma(std::integral_constant<int, kba>{}, ha[r], acc0);
      } else {
        wwait<kYounger>(ra[r]);
        acc0 = mma(std::integral_constant<int, kba>{}, ra[r], acc0);
      }
    }
    if constexpr (S::last(s)) {
      if constexpr (S::tail(s)) { acc0[0] += acc1[0]; acc0[1] += acc1[1]; acc0[2] += acc1[2]; acc0[3] += acc1[3]; }
      if (RELU_OUT) {
        acc0[0] = fmaxf(acc0[0], 0.f); acc0[1] = fmaxf(acc0[1], 0.f); acc0[2] = fmaxf(acc0[2], 0.f); acc0[3] = fmaxf(acc0[3], 0.f);
        acc1[0] = fmaxf(acc1[0], 0.f); acc1[1] = fmaxf(acc1[1], 0.f); acc1[2] = fmaxf(acc1[2], 0.f); acc1[3] = fmaxf(acc1[3], 0.f);
      }
      v_out[S::tile_a(s)] = acc0;
      if constexpr (!S::tail(s)) v_out[S::tile_b(s)] = acc1;
    }
    pin(acc0, acc1);
  });
}
