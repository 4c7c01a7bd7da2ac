// Fused cross-attention decoder forward for gfx950 with bf16 MFMA operands (inference / no-grad path, opt-in:
// hip_decoder.MODE = "bf16").
//
// The kernel of decoder_fused.hip -- one wave owns 16 query points and walks the whole decoder for them in registers, every
// dense layer in the transposed form Y^T = W X^T with the accumulators of layer L being the B operand of layer L + 1 -- on
// v_mfma_f32_16x16x32_bf16 (16 cycles for 8 x the flops of the 32-cycle v_mfma_f32_16x16x4_f32).  chain_bf16.h has the
// operand layout and the k permutation that keeps the accumulator -> operand property.
//
// Numerical contract.  Rounded to bf16 (round to nearest even), ONLY as MFMA operands: the weights of fc_delta.2,
// fc_gamma.0/.2, init_enc, fc_c[i], blocks[i].fc_0/.fc_1, fc_out (once, when packed on the host) and the activation vector
// entering each of those layers (at the C -> B conversion, after the ReLU where there is one).  fp32: fc_delta.0 (K = 3 + bias
// on the relative coordinate: thirteen 16x16x4_f32 MFMAs per slot, as in the fp32 kernel), every accumulator and bias add,
// `pos` where it is added to the key difference and to the value row, the qk / vtab / a_g / v_g tables, the online-softmax
// state, the residual stream `net` across the five blocks (rounded only as a copy when it feeds fc_0 / fc_out), the output.
//
// 208 = 13 tiles is odd: the reduction ends with one v_mfma_f32_16x16x16_bf16 on the 13th tile instead of padding to 224.
// Registers do not decide it (the packed operand is 28 VGPRs either way: the K = 32 instruction wants four aligned registers,
// and the kernel takes 196 VGPRs + 102 AGPRs of the 256 + 256); the weight feed does -- the chain waits for its fragments,
// not for the matrix pipe, and the half block is 512 B per out tile instead of a KiB of which half is zeros (-7 % weight
// bytes on the 13-tile layers).
//
// Every query row is independent of every other: a row's result is the same bits whatever batch, offset or slice it arrives
// in (rows past NQ are computed on a clamped index and never stored).  No barriers.
#include <type_traits>
#include "common.h"
#include "prof.h"

namespace {

#include "chain_f32.h"
#include "chain_bf16.h"

constexpr int DT = 13;   // 16-channel tiles of the attention width (200 -> 208)
constexpr int HT = 8;    // tiles of the MLP width (128)
constexpr int DP = DT * 16;
constexpr int HP = HT * 16;

struct DecParams {
  const float *xyz_q;      // [B,NQ,3]
  const float *anchors;    // [B,A,3]
  const int32_t *idx;      // [B,NQ,KN]
  const float *qk;         // [B,A,DP]   q - w_ks(anchor_feats), zero padded
  const float *vtab;       // [B,A,DP]   w_vs(anchor_feats)
  const float *a_g;        // [B,DP]     logits of the global token
  const float *v_g;        // [B,DP]
  const float *wd0;        // [DP,4]     fc_delta.0 weight | bias
  // W: bf16, fragment-major with the k permutation of chain_bf16.h; biases fp32
  const uint16_t *wd2; const float *bd2;     // [DP,DP], [DP]
  const uint16_t *wg0; const float *bg0;
  const uint16_t *wg2; const float *bg2;
  const uint16_t *winit; const float *binit; // [HP,DP], [HP]
  const uint16_t *wc; const float *bc;       // [5][HP,DP], [5][HP]
  const uint16_t *w0; const float *b0;       // [5][HP,HP], [5][HP]
  const uint16_t *w1; const float *b1;
  const uint16_t *wout; const float *bout;   // [16,HP], [16]
  float *out;              // [B,NQ,3]
  int B, NQ, A, KN;
};

struct Vec {                    // one activation vector per row: NT tiles x 4 channels per lane
  f32x4 t[DT];
};

constexpr int kWaves = 2;   // waves per workgroup: 2 x 39 KiB of private softmax state -> two workgroups per CU

__global__ __launch_bounds__(kWaves * 64) void decoder_fused_fwd_bf16_kernel(DecParams p) {
  // As in the fp32 kernel the per-channel online-softmax state (running max / sum / weighted value: 156 registers) lives in
  // a wave-private LDS slab, laid out [quantity][tile][lane] as float4 = conflict-free ds_read/write_b128, touched once per
  // neighbour slot.  No barriers anywhere.
  __shared__ float4 state[kWaves][3][DT][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int b = blockIdx.y;
  const int q0 = (blockIdx.x * kWaves + wave) * 16;
  if (q0 >= p.NQ) return;                          // no barriers in this kernel
  int q = q0 + li;
  const bool qvalid = q < p.NQ;
  q = qvalid ? q : (p.NQ - 1);
  const size_t qrow = static_cast<size_t>(b) * p.NQ + q;

  const float qx = p.xyz_q[qrow * 3 + 0], qy = p.xyz_q[qrow * 3 + 1], qz = p.xyz_q[qrow * 3 + 2];
  const float *anch = p.anchors + static_cast<size_t>(b) * p.A * 3;
  const float *qkb = p.qk + static_cast<size_t>(b) * p.A * DP;
  const float *vtb = p.vtab + static_cast<size_t>(b) * p.A * DP;

  // online-softmax state per (tile, channel): running max, running sum, running weighted value.
  // It starts from the global token (logits a_g, value v_g, position encoding 0), model/decoder/blocks.py:73-86
  float4 (*S)[DT][64] = state[wave];
#pragma unroll
  for (int t = 0; t < DT; ++t) {
    S[0][t][lane] = *reinterpret_cast<const float4 *>(p.a_g + static_cast<size_t>(b) * DP + t * 16 + 4 * g);
    S[1][t][lane] = make_float4(1.f, 1.f, 1.f, 1.f);
    S[2][t][lane] = *reinterpret_cast<const float4 *>(p.v_g + static_cast<size_t>(b) * DP + t * 16 + 4 * g);
  }

  for (int slot = 0; slot < p.KN; ++slot) {
    // The weights are loop-invariant, and LICM would hoist every one of the ~1000 weight-fragment loads of
    // an iteration out of the slot loop (thousands of live registers -> scratch spills).  Laundering the
    // base pointers through an opaque offset once per iteration makes the loads iteration-dependent again.
    // (an opaque zero offset, not the pointers themselves: those must keep their global address space)
    int opaque0 = 0;
    asm volatile("" : "+s"(opaque0));
    const float *wd0 = p.wd0 + opaque0, *bd2 = p.bd2 + opaque0, *bg0 = p.bg0 + opaque0, *bg2 = p.bg2 + opaque0;
    const uint16_t *wd2 = p.wd2 + opaque0, *wg0 = p.wg0 + opaque0, *wg2 = p.wg2 + opaque0;
    const int a = p.idx[qrow * p.KN + slot];
    // relative coordinate, augmented with 1 for the bias column: lane group g carries component g
    const float rel = g == 0 ? qx - anch[a * 3 + 0]
                    : g == 1 ? qy - anch[a * 3 + 1]
                    : g == 2 ? qz - anch[a * 3 + 2] : 1.0f;
    Vec va, pos;
    Packed<DT> x;
    // delta0: [DP x 4] * [4 x 16 rows], ReLU -- fp32 operands (the relative coordinate is a position)
#pragma unroll
    for (int ot = 0; ot < DT; ++ot) {
      const float w = wd0[(ot * 16 + li) * 4 + g];
      f32x4 acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w, rel, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
      acc[0] = fmaxf(acc[0], 0.f); acc[1] = fmaxf(acc[1], 0.f); acc[2] = fmaxf(acc[2], 0.f); acc[3] = fmaxf(acc[3], 0.f);
      va.t[ot] = acc;
    }
    pack<DT, false>(va.t, x);
    dense_bf16<DT, DT, false, false>(wd2, bd2, x, pos.t, li, g);                    // pos = delta2(h1)
    const float *qka = qkb + static_cast<size_t>(a) * DP + 4 * g;
#pragma unroll
    for (int t = 0; t < DT; ++t) {                                                   // u = (q - k_a) + pos
      const float4 k4 = *reinterpret_cast<const float4 *>(qka + t * 16);
      va.t[t] = f32x4{k4.x + pos.t[t][0], k4.y + pos.t[t][1], k4.z + pos.t[t][2], k4.w + pos.t[t][3]};
    }
    pack<DT, false>(va.t, x);
    dense_bf16<DT, DT, true, false>(wg0, bg0, x, va.t, li, g);                      // h2 = relu(gamma0(u))
    pack<DT, false>(va.t, x);
    dense_bf16<DT, DT, false, false>(wg2, bg2, x, va.t, li, g);                     // logits = gamma2(h2)
    const float *vta = vtb + static_cast<size_t>(a) * DP + 4 * g;
#pragma unroll
    for (int t = 0; t < DT; ++t) {
      const float4 v4 = *reinterpret_cast<const float4 *>(vta + t * 16);
      const float sv[4] = {v4.x + pos.t[t][0], v4.y + pos.t[t][1], v4.z + pos.t[t][2], v4.w + pos.t[t][3]};
      const float4 m4 = S[0][t][lane], l4 = S[1][t][lane], y4 = S[2][t][lane];
      float mm[4] = {m4.x, m4.y, m4.z, m4.w}, ll[4] = {l4.x, l4.y, l4.z, l4.w}, yy[4] = {y4.x, y4.y, y4.z, y4.w};
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float av = va.t[t][c];
        const float mn = fmaxf(mm[c], av);
        const float sc = __expf(mm[c] - mn);
        const float w = __expf(av - mn);
        ll[c] = ll[c] * sc + w;
        yy[c] = yy[c] * sc + w * sv[c];
        mm[c] = mn;
      }
      S[0][t][lane] = make_float4(mm[0], mm[1], mm[2], mm[3]);
      S[1][t][lane] = make_float4(ll[0], ll[1], ll[2], ll[3]);
      S[2][t][lane] = make_float4(yy[0], yy[1], yy[2], yy[3]);
    }
  }
  Vec y;
#pragma unroll
  for (int t = 0; t < DT; ++t) {                                                     // lat = y / l
    const float4 l4 = S[1][t][lane], y4 = S[2][t][lane];
    y.t[t] = f32x4{y4.x / l4.x, y4.y / l4.y, y4.z / l4.z, y4.w / l4.w};
  }

  // MLP tail on [HP]-wide vectors (crosstransformer_decoder.py:63-69).  `net` is the fp32 residual stream: it lives in
  // accumulators across the five blocks and is rounded only as the copy that feeds fc_0 / fc_out.
  Packed<DT> lat;
  pack<DT, false>(y.t, lat);
  Packed<HT> xh;
  f32x4 net[HT], h[HT];
  dense_bf16<HT, DT, false, false>(p.winit, p.binit, lat, net, li, g);
#pragma unroll 1
  for (int i = 0; i < 5; ++i) {
    dense_bf16<HT, DT, false, true>(p.wc + static_cast<size_t>(i) * HP * DP, p.bc + i * HP, lat, net, li, g);
    pack<HT, true>(net, xh);
    dense_bf16<HT, HT, false, false>(p.w0 + static_cast<size_t>(i) * HP * HP, p.b0 + i * HP, xh, h, li, g);
    pack<HT, true>(h, xh);
    dense_bf16<HT, HT, false, true>(p.w1 + static_cast<size_t>(i) * HP * HP, p.b1 + i * HP, xh, net, li, g);
  }
  f32x4 o[1];
  pack<HT, true>(net, xh);
  dense_bf16<1, HT, false, false>(p.wout, p.bout, xh, o, li, g);
  if (g == 0 && qvalid) {   // output channels 0..2 live in lane group 0, registers 0..2
    float *dst = p.out + qrow * 3;
    dst[0] = o[0][0]; dst[1] = o[0][1]; dst[2] = o[0][2];
  }
}

}  // namespace

extern "C" int nsdp_decoder_fused_fwd_bf16(const float *xyz_q, const float *anchors, const int32_t *idx,
                                           const float *qk, const float *vtab, const float *a_g, const float *v_g,
                                           const void *const *weights, int n_weights, int B, int NQ, int A,
                                           int KN, int D, int H, float *out, void *stream) {
  if (static_cast<long long>(B) * NQ <= 0) return 0;
  NSDP_REQUIRE(D == 200 && H == 128, "decoder_fused_fwd_bf16: built for dim=200, hidden_dim=128 (got %d, %d)", D, H);
  NSDP_REQUIRE(n_weights == 17, "decoder_fused_fwd_bf16: expected 17 packed weight pointers, got %d", n_weights);
  NSDP_REQUIRE(xyz_q && anchors && idx && qk && vtab && a_g && v_g && weights && out, "decoder_fused_fwd_bf16: null pointer");
  NSDP_REQUIRE(B <= 65535, "decoder_fused_fwd_bf16: batch too large");
  DecParams p;
  p.xyz_q = xyz_q; p.anchors = anchors; p.idx = idx; p.qk = qk; p.vtab = vtab; p.a_g = a_g; p.v_g = v_g;
  auto wf = [&](int i) { return static_cast<const float *>(weights[i]); };
  auto wh = [&](int i) { return static_cast<const uint16_t *>(weights[i]); };
  p.wd0 = wf(0);
  p.wd2 = wh(1); p.bd2 = wf(2);
  p.wg0 = wh(3); p.bg0 = wf(4);
  p.wg2 = wh(5); p.bg2 = wf(6);
  p.winit = wh(7); p.binit = wf(8);
  p.wc = wh(9); p.bc = wf(10);
  p.w0 = wh(11); p.b0 = wf(12);
  p.w1 = wh(13); p.b1 = wf(14);
  p.wout = wh(15); p.bout = wf(16);
  p.out = out;
  p.B = B; p.NQ = NQ; p.A = A; p.KN = KN;
  hipStream_t st = nsdp::as_stream(stream);
  // the same algorithmic work and bytes as the fp32 kernel: 2.484 MFLOP per query
  nsdp::prof::Scope scope(nsdp::prof::kDecoderFwdB16, st, 2.484e6 * static_cast<double>(B) * NQ,
                          static_cast<double>(B) * NQ * (24.0 + 4.0 * KN));
  hipLaunchKernelGGL(decoder_fused_fwd_bf16_kernel, dim3(nsdp::ceil_div(NQ, 16 * kWaves), B), dim3(kWaves * 64), 0, st, p);
  return nsdp::launch_status("decoder_fused_fwd_bf16_kernel");
}
