// Fused cross-attention decoder forward WITH its 3x3 Jacobian d out / d q (the deformation gradient) for gfx950: the chain of
// decoder_fused.hip differentiated in forward mode (inference / no-grad path, fp32 operands).
//
// The query position enters the decoder only through rel = q - anchor, and every layer of the chain is Y^T = W X^T with the
// 16 MFMA columns as independent rows.  A tangent goes through a linear layer as the same product without the bias, and through
// a ReLU as itself under the VALUE's mask.  So one wave owns 4 query points x 4 columns: MFMA column li = 4 qi + c carries the
// value of query qi for c = 0 and its tangent in direction e_{c-1} for c = 1..3.  The value of a tangent lane is lane 0 of its
// quad in the same lane group g (row = lane & 15, quads are aligned), one DPP quad broadcast away.  Per lane the register
// footprint is that of the forward kernel: the tangents are other lanes, not more registers.
//
// The value columns evaluate, expression for expression, what decoder_fused_fwd_kernel evaluates (an MFMA column depends on
// nothing but its own B column): `out` has the bits of nsdp_decoder_fused_fwd.  Where a value lane and a tangent lane differ, the
// differing OPERAND is selected per lane and the forward kernel's expression keeps its shape (under -ffp-contract=fast a
// reshaped expression could be contracted into a different fused multiply-add than the forward kernel's).
//
// Softmax over the 8 tokens, per channel, with w_i = exp(a_i - m): lat = sum w_i v_i / sum w_i, so
//   dlat = (sum w_i (dv_i + v_i da_i)  -  lat * sum w_i da_i) / sum w_i
// (the running maximum cancels).  Value lanes keep (m, l, y) exactly as the forward kernel; tangent lanes keep (m, L', Y') with
// L' = sum w da, Y' = sum w (dv + v da), rescaled by the same sc as the value's l and y: m is recomputed in every lane from the
// broadcast value logit (the start value a_g does not depend on the column, so all four lanes of a quad hold the same m).
// The global token's logits and value do not depend on q: L' = Y' = 0 at the start.
#include <type_traits>
#include "common.h"
#include "ragged.h"

namespace {

#include "chain_f32.h"

constexpr int DT = 13;   // 16-channel tiles of the attention width (200 -> 208)
constexpr int HT = 8;    // tiles of the MLP width (128)
constexpr int DP = DT * 16;
constexpr int HP = HT * 16;
constexpr int kCols = 4;            // columns per query: value + 3 tangents
constexpr int kQueries = 16 / kCols;  // queries per wave

struct JacParams {
  const float *xyz_q;      // [B,NQ,3]
  const float *anchors;    // [B,A,3]
  const int32_t *idx;      // [B,NQ,KN]
  const float *qk;         // [B,A,DP]
  const float *vtab;       // [B,A,DP]
  const float *a_g;        // [B,DP]
  const float *v_g;        // [B,DP]
  const float *wd0;
  const float *wd2, *bd2;
  const float *wg0, *bg0, *wg2, *bg2;
  const float *winit, *binit;
  const float *wc, *bc;
  const float *w0, *b0, *w1, *b1;
  const float *wout, *bout;
  float *out;              // [B,NQ,3]
  float *jac;              // [B,NQ,3,3]
  int B, NQ, A, KN;
  const int32_t *offsets;  // packed form: [B+1] device
  int cap;
};

struct Vec {
  f32x4 t[DT];
};

constexpr int kWaves = 2;

// lane 0 of the caller's quad (the value column of a tangent lane; a value lane reads itself)
__device__ __forceinline__ float quad0(float x) {
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, x), 0x00 /* quad_perm:[0,0,0,0] */, 0xf, 0xf, true));
}

// per-lane select of a whole fragment, component by component (a select of two float4 OBJECTS is lowered through a stack slot)
__device__ __forceinline__ f32x4 sel4(bool c, f32x4 a, f32x4 b) {
  return f32x4{c ? a[0] : b[0], c ? a[1] : b[1], c ? a[2] : b[2], c ? a[3] : b[3]};
}
__device__ __forceinline__ float4 sel4(bool c, float4 a, float4 b) {
  return make_float4(c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z, c ? a.w : b.w);
}

// ReLU of one column element: a value lane clamps itself as the forward kernel does, a tangent lane passes where its value is
// positive (derivative 0 at exactly 0)
__device__ __forceinline__ float relu_col(float x, bool isval) {
  const float v = quad0(x);
  const float own = fmaxf(x, 0.f);
  const float tan = v > 0.f ? x : 0.f;
  return isval ? own : tan;
}
__device__ __forceinline__ void relu_col(f32x4 &a, bool isval) {
  a[0] = relu_col(a[0], isval); a[1] = relu_col(a[1], isval); a[2] = relu_col(a[2], isval); a[3] = relu_col(a[3], isval);
}

// dense<> of chain_f32.h for [value | tangent] columns: the same steps, prefetch ring and MFMA order; the bias goes to value
// columns only, ReLU takes the value's mask in tangent columns, an ACC residual is linear and applies to every column.
template <int NTOUT, int NTIN, bool RELU_IN, bool RELU_OUT, bool ACC>
__device__ __forceinline__ void dense_jt(const float *__restrict__ W, const float *__restrict__ bias, const f32x4 *v_in,
                                         f32x4 *v_out, int li, int g, bool isval) {
  auto ldbias = [&](int tile, unsigned bl) -> float4 {
    const float4 b4 = ldg4(bias + tile * 16, bl);
    return sel4(isval, b4, make_float4(0.f, 0.f, 0.f, 0.f));
  };
  using S = Steps<NTOUT, NTIN>;
  f32x4 x[NTIN];
#pragma unroll
  for (int kb = 0; kb < NTIN; ++kb) {
    x[kb] = v_in[kb];
    if (RELU_IN) relu_col(x[kb], isval);
  }
  const unsigned wl = (16u * g + li) * 16u;
  const unsigned bl = 16u * g;
  f32x4 ra[kRing], rb[kRing];
  auto issue = [&](auto I) {
    constexpr int s = decltype(I)::value;
    wload<0>(ra[s % kRing], W + (S::tile_a(s) * NTIN + S::kb_a(s)) * 256, wl);
    if constexpr (S::has_b(s)) wload<0>(rb[s % kRing], W + (S::tile_b(s) * NTIN + S::kb_b(s)) * 256, wl);
  };
  constexpr int kPro = kPrefetch < S::kSteps ? kPrefetch : S::kSteps;
  static_for<0, kPro>(issue);
  float4 ba = ldbias(S::tile_a(0), bl);
  float4 bb = ldbias(S::tile_b(0), bl);
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  static_for<0, S::kSteps>([&](auto I) {
    constexpr int s = decltype(I)::value;
    if constexpr (s + kPrefetch < S::kSteps) issue(std::integral_constant<int, s + kPrefetch>{});
    if constexpr (S::first(s)) {
      acc0 = ACC ? v_out[S::tile_a(s)] : f32x4{0.f, 0.f, 0.f, 0.f};
      acc0[0] += ba.x; acc0[1] += ba.y; acc0[2] += ba.z; acc0[3] += ba.w;
      if constexpr (S::tail(s)) {
        acc1 = f32x4{0.f, 0.f, 0.f, 0.f};
      } else {
        acc1 = ACC ? v_out[S::tile_b(s)] : f32x4{0.f, 0.f, 0.f, 0.f};
        acc1[0] += bb.x; acc1[1] += bb.y; acc1[2] += bb.z; acc1[3] += bb.w;
      }
      constexpr int sn = S::next_first(s);
      if constexpr (sn < S::kSteps) {
        ba = ldbias(S::tile_a(sn), bl);
        bb = ldbias(S::tile_b(sn), bl);
      }
    }
    constexpr int kYounger = S::loads_after(s, kPrefetch);
    const f32x4 xa = x[S::kb_a(s)];
    if constexpr (S::has_b(s)) {
      wwait<kYounger>(ra[s % kRing], rb[s % kRing]);
      const f32x4 a4 = ra[s % kRing], b4 = rb[s % kRing];
      const f32x4 xb = x[S::kb_b(s)];
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[0], xa[0], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(b4[0], xb[0], acc1, 0, 0, 0);
      pin(acc0, acc1);
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[1], xa[1], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(b4[1], xb[1], acc1, 0, 0, 0);
      pin(acc0, acc1);
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[2], xa[2], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(b4[2], xb[2], acc1, 0, 0, 0);
      pin(acc0, acc1);
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[3], xa[3], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(b4[3], xb[3], acc1, 0, 0, 0);
    } else {
      wwait<kYounger>(ra[s % kRing]);
      const f32x4 a4 = ra[s % kRing];
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[0], xa[0], acc0, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[1], xa[1], acc0, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[2], xa[2], acc0, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[3], xa[3], acc0, 0, 0, 0);
    }
    if constexpr (S::last(s)) {
      if constexpr (S::tail(s)) { acc0[0] += acc1[0]; acc0[1] += acc1[1]; acc0[2] += acc1[2]; acc0[3] += acc1[3]; }
      if (RELU_OUT) {
        relu_col(acc0, isval);
        relu_col(acc1, isval);
      }
      v_out[S::tile_a(s)] = acc0;
      if constexpr (!S::tail(s)) v_out[S::tile_b(s)] = acc1;
    }
    pin(acc0, acc1);
  });
}

template <bool Ragged>
__global__ __launch_bounds__(kWaves * 64) void decoder_jacobian_fwd_kernel(JacParams p) {
  // the wave-private softmax slab of the forward kernel, [quantity][tile][lane] float4: (m, l, y) in value lanes,
  // (m, L', Y') in tangent lanes.  No barriers anywhere.
  __shared__ float4 state[kWaves][3][DT][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int qi = li >> 2, col = li & 3;
  const bool isval = col == 0;
  int b;
  size_t qrow;
  bool qvalid;
  if constexpr (Ragged) {
    int row0, end;
    const int tile = __builtin_amdgcn_readfirstlane(static_cast<int>(blockIdx.x * kWaves + wave));
    if (!nsdp::ragged_tile<kQueries>(p.offsets, p.B, p.cap, tile, b, row0, end)) return;
    const int q = row0 + qi;                       // a shape's last tile is partial: lanes clamped to its last row, not stored
    qvalid = q < end;
    qrow = static_cast<size_t>(qvalid ? q : end - 1);
  } else {
    b = blockIdx.y;
    const int q0 = (blockIdx.x * kWaves + wave) * kQueries;
    if (q0 >= p.NQ) return;                        // no barriers in this kernel
    int q = q0 + qi;
    qvalid = q < p.NQ;
    q = qvalid ? q : (p.NQ - 1);
    qrow = static_cast<size_t>(b) * p.NQ + q;
  }

  const float qx = p.xyz_q[qrow * 3 + 0], qy = p.xyz_q[qrow * 3 + 1], qz = p.xyz_q[qrow * 3 + 2];
  const float *anch = p.anchors + static_cast<size_t>(b) * p.A * 3;
  const float *qkb = p.qk + static_cast<size_t>(b) * p.A * DP;
  const float *vtb = p.vtab + static_cast<size_t>(b) * p.A * DP;
  // B operand of a tangent column at delta0: e_{col-1}, 0 in the bias slot
  const float unit = g == col - 1 ? 1.0f : 0.0f;

  float4 (*S)[DT][64] = state[wave];
#pragma unroll
  for (int t = 0; t < DT; ++t) {
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 vg4 = *reinterpret_cast<const float4 *>(p.v_g + static_cast<size_t>(b) * DP + t * 16 + 4 * g);
    S[0][t][lane] = *reinterpret_cast<const float4 *>(p.a_g + static_cast<size_t>(b) * DP + t * 16 + 4 * g);
    S[1][t][lane] = sel4(isval, make_float4(1.f, 1.f, 1.f, 1.f), z4);
    S[2][t][lane] = sel4(isval, vg4, z4);
  }

  for (int slot = 0; slot < p.KN; ++slot) {
    // (see decoder_fused.hip: an opaque zero offset per iteration keeps LICM from hoisting a slot's ~1000 weight loads)
    int opaque0 = 0;
    asm volatile("" : "+s"(opaque0));
    const float *wd0 = p.wd0 + opaque0, *wd2 = p.wd2 + opaque0, *bd2 = p.bd2 + opaque0, *wg0 = p.wg0 + opaque0,
                *bg0 = p.bg0 + opaque0, *wg2 = p.wg2 + opaque0, *bg2 = p.bg2 + opaque0;
    int a = p.idx[qrow * p.KN + slot];
    if constexpr (Ragged) a = min(max(a, 0), p.A - 1);
    const float rel = g == 0 ? qx - anch[a * 3 + 0]
                    : g == 1 ? qy - anch[a * 3 + 1]
                    : g == 2 ? qz - anch[a * 3 + 2] : 1.0f;
    const float bop = isval ? rel : unit;
    Vec va, vb, pos;
#pragma unroll
    for (int ot = 0; ot < DT; ++ot) {
      const float w = wd0[(ot * 16 + li) * 4 + g];
      f32x4 acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w, bop, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
      relu_col(acc, isval);
      va.t[ot] = acc;
    }
    dense_jt<DT, DT, false, false, false>(wd2, bd2, va.t, pos.t, li, g, isval);      // pos = delta2(h1)
    const float *qka = qkb + static_cast<size_t>(a) * DP + 4 * g;
#pragma unroll
    for (int t = 0; t < DT; ++t) {                                                   // u = (q - k_a) + pos; du = dpos
      const float4 k4 = *reinterpret_cast<const float4 *>(qka + t * 16);
      const f32x4 u = f32x4{k4.x + pos.t[t][0], k4.y + pos.t[t][1], k4.z + pos.t[t][2], k4.w + pos.t[t][3]};
      va.t[t] = sel4(isval, u, pos.t[t]);
    }
    dense_jt<DT, DT, false, true, false>(wg0, bg0, va.t, vb.t, li, g, isval);        // h2 = relu(gamma0(u))
    dense_jt<DT, DT, false, false, false>(wg2, bg2, vb.t, va.t, li, g, isval);       // logits = gamma2(h2)
    const float *vta = vtb + static_cast<size_t>(a) * DP + 4 * g;
#pragma unroll
    for (int t = 0; t < DT; ++t) {
      const float4 v4 = *reinterpret_cast<const float4 *>(vta + t * 16);
      const float sv[4] = {v4.x + pos.t[t][0], v4.y + pos.t[t][1], v4.z + pos.t[t][2], v4.w + pos.t[t][3]};
      const float4 m4 = S[0][t][lane], l4 = S[1][t][lane], y4 = S[2][t][lane];
      float mm[4] = {m4.x, m4.y, m4.z, m4.w}, ll[4] = {l4.x, l4.y, l4.z, l4.w}, yy[4] = {y4.x, y4.y, y4.z, y4.w};
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float da = va.t[t][c];          // a value lane's logit, a tangent lane's logit tangent
        const float av = quad0(da);           // the value's logit in every lane of the quad
        const float svv = quad0(sv[c]);       // the value's v + pos (a tangent lane's own sv is not used)
        const float dv = pos.t[t][c];         // tangent lanes: d(v + pos) = dpos
        const float mn = fmaxf(mm[c], av);
        const float sc = __expf(mm[c] - mn);
        const float w = __expf(av - mn);
        // the forward kernel's two expressions with the addend / factor selected per lane BEFORE them: each product keeps
        // one use, so contraction forms the fused multiply-adds it forms there (a product shared by a value form and a
        // tangent form would be fused the other way round)
        const float wl = isval ? w : w * da;                  // value: w;       tangent: w da
        const float fy = isval ? sv[c] : dv + svv * da;       // value: v + pos; tangent: dv + v da
        ll[c] = ll[c] * sc + wl;
        yy[c] = yy[c] * sc + w * fy;
        mm[c] = mn;
      }
      S[0][t][lane] = make_float4(mm[0], mm[1], mm[2], mm[3]);
      S[1][t][lane] = make_float4(ll[0], ll[1], ll[2], ll[3]);
      S[2][t][lane] = make_float4(yy[0], yy[1], yy[2], yy[3]);
    }
  }
  Vec y;
#pragma unroll
  for (int t = 0; t < DT; ++t) {                                 // lat = y / l;  dlat = (Y' - lat L') / l
    const float4 l4 = S[1][t][lane], y4 = S[2][t][lane];
    const f32x4 lat = f32x4{y4.x / l4.x, y4.y / l4.y, y4.z / l4.z, y4.w / l4.w};
    const float lv[4] = {quad0(l4.x), quad0(l4.y), quad0(l4.z), quad0(l4.w)};
    const float latv[4] = {quad0(lat[0]), quad0(lat[1]), quad0(lat[2]), quad0(lat[3])};
    const f32x4 dlat = f32x4{(y4.x - latv[0] * l4.x) / lv[0], (y4.y - latv[1] * l4.y) / lv[1],
                             (y4.z - latv[2] * l4.z) / lv[2], (y4.w - latv[3] * l4.w) / lv[3]};
    y.t[t] = sel4(isval, lat, dlat);
  }

  f32x4 net[HT], h[HT];
  dense_jt<HT, DT, false, false, false>(p.winit, p.binit, y.t, net, li, g, isval);
#pragma unroll 1
  for (int i = 0; i < 5; ++i) {
    dense_jt<HT, DT, false, false, true>(p.wc + static_cast<size_t>(i) * HP * DP, p.bc + i * HP, y.t, net, li, g, isval);
    dense_jt<HT, HT, true, false, false>(p.w0 + static_cast<size_t>(i) * HP * HP, p.b0 + i * HP, net, h, li, g, isval);
    dense_jt<HT, HT, true, false, true>(p.w1 + static_cast<size_t>(i) * HP * HP, p.b1 + i * HP, h, net, li, g, isval);
  }
  f32x4 o[1];
  dense_jt<1, HT, true, false, false>(p.wout, p.bout, net, o, li, g, isval);
  if (g == 0 && qvalid) {   // output channels 0..2 live in lane group 0, registers 0..2
    if (isval) {
      float *dst = p.out + qrow * 3;
      dst[0] = o[0][0]; dst[1] = o[0][1]; dst[2] = o[0][2];
    } else {                // jac[i][j] = d out_i / d q_j: tangent column j + 1, register i
      float *dst = p.jac + qrow * 9 + (col - 1);
      dst[0] = o[0][0]; dst[3] = o[0][1]; dst[6] = o[0][2];
    }
  }
}

// host side of both entry points: argument checks (those of the fused forward entries) and the parameter block
static int fill_params(const char *who, JacParams &p, const float *xyz_q, const float *anchors, const int32_t *idx,
                       const float *qk, const float *vtab, const float *a_g, const float *v_g, const float *const *weights,
                       int n_weights, int B, int A, int KN, int D, int H, float *out, float *jac) {
  NSDP_REQUIRE(D == 200 && H == 128, "%s: built for dim=200, hidden_dim=128 (got %d, %d)", who, D, H);
  NSDP_REQUIRE(n_weights == 17, "%s: expected 17 packed weight pointers, got %d", who, n_weights);
  NSDP_REQUIRE(xyz_q && anchors && idx && qk && vtab && a_g && v_g && weights && out && jac, "%s: null pointer", who);
  NSDP_REQUIRE(B <= 65535, "%s: batch too large", who);
  p.xyz_q = xyz_q; p.anchors = anchors; p.idx = idx; p.qk = qk; p.vtab = vtab; p.a_g = a_g; p.v_g = v_g;
  p.wd0 = weights[0];
  p.wd2 = weights[1]; p.bd2 = weights[2];
  p.wg0 = weights[3]; p.bg0 = weights[4];
  p.wg2 = weights[5]; p.bg2 = weights[6];
  p.winit = weights[7]; p.binit = weights[8];
  p.wc = weights[9]; p.bc = weights[10];
  p.w0 = weights[11]; p.b0 = weights[12];
  p.w1 = weights[13]; p.b1 = weights[14];
  p.wout = weights[15]; p.bout = weights[16];
  p.out = out; p.jac = jac;
  p.B = B; p.NQ = 0; p.A = A; p.KN = KN;
  p.offsets = nullptr; p.cap = 0;
  return 0;
}

}  // namespace

extern "C" int nsdp_decoder_jacobian_fwd(const float *xyz_q, const float *anchors, const int32_t *idx, const float *qk,
                                         const float *vtab, const float *a_g, const float *v_g, const float *const *weights,
                                         int n_weights, int B, int NQ, int A, int KN, int D, int H, float *out, float *jac,
                                         void *stream) {
  if (static_cast<long long>(B) * NQ <= 0) return 0;
  JacParams p;
  if (int rc = fill_params("decoder_jacobian_fwd", p, xyz_q, anchors, idx, qk, vtab, a_g, v_g, weights, n_weights, B, A, KN, D, H, out, jac)) return rc;
  p.NQ = NQ;
  hipStream_t st = nsdp::as_stream(stream);
  hipLaunchKernelGGL(decoder_jacobian_fwd_kernel<false>, dim3(nsdp::ceil_div(NQ, kQueries * kWaves), B), dim3(kWaves * 64), 0, st, p);
  return nsdp::launch_status("decoder_jacobian_fwd_kernel");
}

extern "C" int nsdp_decoder_jacobian_fwd_ragged(const float *xyz_q, const int32_t *offsets, const float *anchors,
                                                const int32_t *idx, const float *qk, const float *vtab, const float *a_g,
                                                const float *v_g, const float *const *weights, int n_weights, int B, int cap,
                                                int A, int KN, int D, int H, float *out, float *jac, void *stream) {
  if (static_cast<long long>(B) * cap <= 0) return 0;
  JacParams p;
  if (int rc = fill_params("decoder_jacobian_fwd_ragged", p, xyz_q, anchors, idx, qk, vtab, a_g, v_g, weights, n_weights, B, A, KN, D, H, out, jac)) return rc;
  NSDP_REQUIRE(offsets, "decoder_jacobian_fwd_ragged: null pointer (offsets)");
  NSDP_REQUIRE(A >= 1, "decoder_jacobian_fwd_ragged: no anchors");
  p.offsets = offsets; p.cap = cap;
  hipStream_t st = nsdp::as_stream(stream);
  const int tiles = static_cast<int>(nsdp::ragged_max_tiles(cap, B, kQueries));
  hipLaunchKernelGGL(decoder_jacobian_fwd_kernel<true>, dim3(nsdp::ceil_div(tiles, kWaves)), dim3(kWaves * 64), 0, st, p);
  return nsdp::launch_status("decoder_jacobian_fwd_kernel<ragged>");
}
