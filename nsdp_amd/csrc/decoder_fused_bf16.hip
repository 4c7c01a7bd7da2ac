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
#include "ragged.h"

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
  // packed (ragged) form, ragged.h: xyz_q [cap,3], idx [cap,KN], out [cap,3]; NQ unused
  const int32_t *offsets;  // [B+1] device
  int cap;
};

struct Vec {                    // one activation vector per row: NT tiles x 4 channels per lane
  f32x4 t[DT];
};

constexpr int kWaves = 2;   // waves per workgroup: 2 x 39 KiB of private softmax state -> two workgroups per CU

#define NSDP_DEC_KERNEL decoder_fused_fwd_bf16_kernel
#define NSDP_DEC_RAGGED false
#include "decoder_bf16_body.h"
#undef NSDP_DEC_KERNEL
#undef NSDP_DEC_RAGGED
#define NSDP_DEC_KERNEL decoder_fused_ragged_bf16_kernel
#define NSDP_DEC_RAGGED true
#include "decoder_bf16_body.h"
#undef NSDP_DEC_KERNEL
#undef NSDP_DEC_RAGGED

// host side of both entry points: argument checks and the parameter block (NQ / offsets, cap are the caller's to set)
static int fill_params(const char *who, DecParams &p, const float *xyz_q, const float *anchors, const int32_t *idx,
                       const float *qk, const float *vtab, const float *a_g, const float *v_g, const void *const *weights,
                       int n_weights, int B, int A, int KN, int D, int H, float *out) {
  NSDP_REQUIRE(D == 200 && H == 128, "%s: built for dim=200, hidden_dim=128 (got %d, %d)", who, D, H);
  NSDP_REQUIRE(n_weights == 17, "%s: expected 17 packed weight pointers, got %d", who, n_weights);
  NSDP_REQUIRE(xyz_q && anchors && idx && qk && vtab && a_g && v_g && weights && out, "%s: null pointer", who);
  NSDP_REQUIRE(B <= 65535, "%s: batch too large", who);
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
  p.B = B; p.NQ = 0; p.A = A; p.KN = KN;
  p.offsets = nullptr; p.cap = 0;
  return 0;
}

}  // namespace

extern "C" int nsdp_decoder_fused_fwd_bf16(const float *xyz_q, const float *anchors, const int32_t *idx,
                                      const float *qk, const float *vtab, const float *a_g, const float *v_g,
                                      const void *const *weights, int n_weights, int B, int NQ, int A,
                                      int KN, int D, int H, float *out, void *stream) {
  if (static_cast<long long>(B) * NQ <= 0) return 0;
  DecParams p;
  if (int rc = fill_params("decoder_fused_fwd_bf16", p, xyz_q, anchors, idx, qk, vtab, a_g, v_g, weights, n_weights, B, A, KN, D, H, out)) return rc;
  p.NQ = NQ;
  hipStream_t st = nsdp::as_stream(stream);
  // the same algorithmic work and bytes as the fp32 kernel: 2.484 MFLOP per query
  nsdp::prof::Scope scope(nsdp::prof::kDecoderFwdB16, st, 2.484e6 * static_cast<double>(B) * NQ,
                          static_cast<double>(B) * NQ * (24.0 + 4.0 * KN));
  hipLaunchKernelGGL(decoder_fused_fwd_bf16_kernel, dim3(nsdp::ceil_div(NQ, 16 * kWaves), B), dim3(kWaves * 64), 0, st, p);
  return nsdp::launch_status("decoder_fused_fwd_bf16_kernel");
}

extern "C" int nsdp_decoder_fused_fwd_bf16_ragged(const float *xyz_q, const int32_t *offsets, const float *anchors,
                                             const int32_t *idx, const float *qk, const float *vtab, const float *a_g,
                                             const float *v_g, const void *const *weights, int n_weights, int B,
                                             int cap, int A, int KN, int D, int H, float *out, void *stream) {
  if (static_cast<long long>(B) * cap <= 0) return 0;
  DecParams p;
  if (int rc = fill_params("decoder_fused_fwd_bf16_ragged", p, xyz_q, anchors, idx, qk, vtab, a_g, v_g, weights, n_weights, B, A, KN, D, H, out)) return rc;
  NSDP_REQUIRE(offsets, "decoder_fused_fwd_bf16_ragged: null pointer (offsets)");
  NSDP_REQUIRE(A >= 1, "decoder_fused_fwd_bf16_ragged: no anchors");
  p.offsets = offsets; p.cap = cap;
  hipStream_t st = nsdp::as_stream(stream);
  // the host does not know how many of the cap rows are real (offsets live on the device and are not read back): the work
  // and the bytes are accounted with cap, an UPPER bound -- rates derived from them are upper bounds too
  nsdp::prof::Scope scope(nsdp::prof::kDecoderFwdB16, st, 2.484e6 * static_cast<double>(cap),
                          static_cast<double>(cap) * (24.0 + 4.0 * KN));
  const int tiles = static_cast<int>(nsdp::ragged_max_tiles(cap, B, 16));
  hipLaunchKernelGGL(decoder_fused_ragged_bf16_kernel, dim3(nsdp::ceil_div(tiles, kWaves)), dim3(kWaves * 64), 0, st, p);
  return nsdp::launch_status("decoder_fused_ragged_bf16_kernel");
}
