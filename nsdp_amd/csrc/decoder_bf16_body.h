// The body of the two bf16-operand decoder kernels of decoder_fused_bf16.hip, included once per kernel with
//   NSDP_DEC_KERNEL  the kernel's name
//   NSDP_DEC_RAGGED  false: the rectangular [B,NQ] form, shape = blockIdx.y;  true: a packed query set -- the wave's tile
//                    index is mapped to (shape, first row, end row of the shape) from p.offsets on the device (ragged.h).
// Everything after that mapping is the one body, so a row gets the same bits in either form.  Two kernels of two names, not
// two instantiations of a template (the register / scratch audit of the rectangular kernel identifies it by its name alone),
// and textual inclusion, not a shared __device__ function (through one, the rectangular kernel's schedule came out
// different from the one it has as a kernel of its own: 32 more accumulator moves).
__global__ __launch_bounds__(kWaves * 64) void NSDP_DEC_KERNEL(DecParams p) {
  constexpr bool Ragged = NSDP_DEC_RAGGED;
  // As in the fp32 kernel the per-channel online-softmax state (running max / sum / weighted value: 156 registers) lives in
  // a wave-private LDS slab, laid out [quantity][tile][lane] as float4 = conflict-free ds_read/write_b128, touched once per
  // neighbour slot.  No barriers anywhere.
  __shared__ float4 state[kWaves][3][DT][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, g = lane >> 4;
  int b;
  size_t qrow;
  bool qvalid;
  if constexpr (Ragged) {
    // (surplus tiles return; no barriers in this kernel.  b is wave-uniform by construction: scalar table bases)
    int row0, end;
    const int tile = __builtin_amdgcn_readfirstlane(static_cast<int>(blockIdx.x * kWaves + wave));
    if (!nsdp::ragged_tile<16>(p.offsets, p.B, p.cap, tile, b, row0, end)) return;
    const int q = row0 + li;                       // a shape's last tile is partial: lanes clamped to its last row, not stored
    qvalid = q < end;
    qrow = static_cast<size_t>(qvalid ? q : end - 1);
  } else {
    b = blockIdx.y;
    const int q0 = (blockIdx.x * kWaves + wave) * 16;
    if (q0 >= p.NQ) return;                        // no barriers in this kernel
    int q = q0 + li;
    qvalid = q < p.NQ;
    q = qvalid ? q : (p.NQ - 1);
    qrow = static_cast<size_t>(b) * p.NQ + q;
  }

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
    int a = p.idx[qrow * p.KN + slot];
    if constexpr (Ragged) a = min(max(a, 0), p.A - 1);   // (the packed form promises in-bounds accesses whatever its inputs hold)
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
