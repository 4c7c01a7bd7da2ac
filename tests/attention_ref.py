"""fp64 reference, first-order error envelope and fp32 emulation of the vector-attention glue (csrc/attention.hip).

Plain torch, any device.  Three things live here:

* ``pre_reference`` / ``post_reference``: the operation in fp64, forward and every gradient, built by autograd from
  ``torch.softmax`` (not from the saved-lse formulation the kernels use).  Inputs are the exact upcasts of the fp32 / bf16
  tensors the kernel receives.
* the envelope ``env`` of every output: the first-order rounding bound of the formula the kernel header states, evaluated in
  fp64 from the reference's intermediates.  With u = 2^-24, u_s = u (fp32 storage) or 2^-9 (bf16 storage of y, u, da, dpos),
  w_j = exp(a_j - lse), s_j the values, yb = sum_j w_j s_j, r the residual, c_j = 3 + |a_j - lse| + |lse| + |a_j|:

      env(dpos_j) = u |dy| w_j c_j + u_s |dpos_j|
      env(da_j)   = u |dy| w_j (c_j |s_j - yb| + S_j + Yb + sum_i w_i S_i) + u_s |dy| w_j (|y| + |r|) [residual] + u_s |da_j|
      env(y)      = u sum_j w_j S_j c_j + u_s (|y| + |r|)
      env(u)      = u (|q - k| + |u|) + u_s |u|

  S_j = |s_j| and Yb = |yb| for the plain form.  The ``sub=(kf, q)`` form builds its values as u + (v + k)[idx] - q, whose
  roundings are those of the larger intermediates: S_j = |v + k| + |(v + k) - q| + |s_j| forward, |v + k| + |u + (v + k)|
  backward, and Yb = |y - r| + |y - r + q| (``_sub_magnitudes``).  [residual]: the kernel recovers yb = y - r from the STORED y,
  so with a residual the storage rounding of y enters at the scale |y| + |r|; without one only bf16 storage adds anything
  (u_s - u) |y| (the fp32 rounding of y is the Yb term).  A floor of 1e-40 is added.
  Flushed weights: the kernels take exp through the hardware exp2 (__expf), whose results below the smallest normal fp32,
  2^-126, come back as zero -- an absolute error of the weight of up to 2^-126, forty orders below the largest weight of the
  softmax, but not below u w_j c_j.  Where the reference weight is under 2^-125 (a - lse < -86.6) the envelope therefore adds
  2^-126 |dy| to env(dpos_j), 2^-126 |dy| |s_j - yb| to env(da_j) and 2^-126 S_j to env(y); sums inherit it through their
  addends.  (Measured before the term was there: every conditioning case at logit spread 30, and none other, was outside the
  bound, by up to 2^-126 |dy| / 1e-40 = 117 |dy| envelopes, on all four backward forms alike; torch's CPU exp keeps
  subnormal results, so the fp32 emulation did not show it.)
  Summed outputs (dvf, dkf, dq, da_g, dv_g): env = sum env(addend) + L u sum |addend|, L the number of addends of the entry
  (rigorous in any order; addends that are exactly zero do not count: adding them rounds nothing), + u_s |sum| where the
  result is stored in bf16.
  The metric is E = max over elements of |got - ref64| / env, per tensor.
* ``emulate_post`` / ``emulate_pre``: the same formulas in plain torch fp32 as the header describes them (online softmax,
  saved lse, yb = y - r).  tests/test_attention_ref_cpu.py measures them against the fp64 reference.

E_EMUL below is the largest E that emulation reaches over the conditioning sweep ``conditioning_cases`` (logit spread
{0, 1, 30} x common offset {0, +1000, -1000} x residual scale {0, 1, 2^6, 2^12}, plus a global token 40 above the largest and
40 below the smallest logit) on the shapes ``SWEEP_SHAPES``, fp32 and bf16 storage: a correct fp32 implementation of the
stated formulas stays within E_EMUL envelopes.  Measured: 1.77 with fp32 storage (da, the (2, 37, 50, 10, 120) shape, spread 1,
no offset, no residual) and 1.99 with bf16 storage (y, da, dpos: half an ulp of a bf16 is 2^-8 of the value, twice u_s);
E_EMUL = 2.0 is that maximum rounded up.  The GPU tests allow 4 max(1, E_EMUL): __expf / __logf against a correctly
rounded exp (a few ulp each) and another summation order.
"""
from __future__ import annotations

import torch

U32 = 2.0 ** -24
U_BF16 = 2.0 ** -9
FLOOR = 1e-40
FLUSH = 2.0 ** -126          # the smallest normal fp32: results of the hardware exp2 below it come back as zero
E_EMUL = 2.0          # measured: see tests/test_attention_ref_cpu.py::test_emulation_stays_inside_the_envelope
GPU_FACTOR = 4.0


def gpu_bound():
    return GPU_FACTOR * max(1.0, E_EMUL)


def storage_unit(dtype):
    return U_BF16 if dtype is torch.bfloat16 else U32


def gather(x, idx):
    """x [B,N,d], idx [B,n,k] -> [B,n,k,d]."""
    B, n, k = idx.shape
    d = x.shape[-1]
    return torch.gather(x, 1, idx.reshape(B, n * k, 1).expand(-1, -1, d).long()).reshape(B, n, k, d)


def scatter(src, idx, N):
    """src [B,n,k,d] -> [B,N,d]: the sum of the rows by idx [B,n,k] (index_add in the dtype of src)."""
    B, n, k, d = src.shape
    out = torch.zeros(B, N, d, dtype=src.dtype, device=src.device)
    out.scatter_add_(1, idx.long().reshape(B, n * k, 1).expand(-1, -1, d), src.reshape(B, n * k, d))
    return out


def counts(idx, N):
    """[B,N,1] float64: the number of (centre, neighbour) entries of each source row."""
    B = idx.shape[0]
    out = torch.zeros(B, N, dtype=torch.float64, device=idx.device)
    out.scatter_add_(1, idx.long().reshape(B, -1), torch.ones(B, idx[0].numel(), dtype=torch.float64, device=idx.device))
    return out.unsqueeze(-1)


def _d(t):
    return None if t is None else t.detach().double()


# ----------------------------------------------------------------------------------------------------------------------
# attn_pre
# ----------------------------------------------------------------------------------------------------------------------
def pre_reference(q, kf, pos, idx, du=None, acc=None):
    """u = q - kf[idx] + pos (q [B,n,d] or [B,1,d]) and, given du, the gradients dq, dkf, dpos (``acc``: d(pos) parked by
    attn_post, to which the kernel adds du).  Returns (ref, env): dicts of fp64 tensors."""
    us = storage_unit(pos.dtype)
    uo = us if pos.dtype is torch.bfloat16 else 0.0
    q64, kf64, pos64 = _d(q), _d(kf), _d(pos)
    N = kf.shape[1]
    qk = q64.unsqueeze(2) - gather(kf64, idx)
    u = qk + pos64
    ref = {"u": u}
    env = {"u": U32 * (qk.abs() + u.abs()) + us * u.abs() + FLOOR}
    if du is None:
        return ref, env
    du64 = _d(du)
    mag = du64.abs()
    if q.shape[1] == 1 and pos.shape[1] != 1:
        dq = du64.sum(dim=(1, 2)).unsqueeze(1)
        L, m = float(pos.shape[1] * pos.shape[2]), mag.sum(dim=(1, 2)).unsqueeze(1)
    else:
        dq, L, m = du64.sum(dim=2), float(pos.shape[2]), mag.sum(dim=2)
    ref["dq"] = dq
    env["dq"] = L * U32 * m + uo * dq.abs() + FLOOR
    ref["dkf"] = -scatter(du64, idx, N)
    env["dkf"] = counts(idx, N) * U32 * scatter(mag, idx, N) + uo * ref["dkf"].abs() + FLOOR
    if acc is not None:          # (without it d(pos) is du itself, handed through)
        ref["dpos"] = du64 + _d(acc)
        env["dpos"] = us * ref["dpos"].abs() + FLOOR
    return ref, env


def emulate_pre(q, kf, pos, idx, du=None):
    """The kernels' arithmetic in torch fp32, rounded to the storage type where the kernels store."""
    st = pos.dtype
    f = lambda t: t.detach().float()
    u = ((f(q).unsqueeze(2) - gather(f(kf), idx)) + f(pos)).to(st)
    out = {"u": u}
    if du is not None:
        g = f(du)
        per_shape = q.shape[1] == 1 and pos.shape[1] != 1
        dq = g.sum(dim=(1, 2)).unsqueeze(1) if per_shape else g.sum(dim=2)
        dkf = -scatter(g, idx, kf.shape[1])
        out.update(dq=dq.to(st), dkf=dkf.to(st))
    return out


# ----------------------------------------------------------------------------------------------------------------------
# attn_post
# ----------------------------------------------------------------------------------------------------------------------
def _sub_magnitudes(vf64, pos64, idx, sub):
    """Values of the sub=(kf, q) form and the magnitudes at which they are rounded: (s, S_fwd, S_bwd, qpt).  ``pos`` holds
    u = q_i - k_j + pos; the table is v + k (- q when q is one vector per shape), qpt the per-point q the kernels subtract."""
    kf, q = sub
    kf64, q64 = _d(kf), _d(q)
    per_shape = q.shape[1] == 1 and pos64.shape[1] != 1
    vk = vf64 + kf64 if kf is not None else vf64
    vk_mag = vk.abs() if kf is not None else torch.zeros_like(vk)       # (rounding of the host's v + k)
    if per_shape:
        tab = vk - q64
        g_tab, g_mag = gather(tab, idx), gather(vk_mag + tab.abs(), idx)
        s = pos64 + g_tab
        S = g_mag + s.abs()
        return s, S, S, None
    g_vk, g_mag = gather(vk, idx), gather(vk_mag, idx)
    t = g_vk - q64.unsqueeze(2)
    s = pos64 + t
    return s, g_mag + t.abs() + s.abs(), g_mag + (pos64 + g_vk).abs(), q64


def post_reference(a, vf, pos, idx, a_g=None, v_g=None, residual=None, dy=None, sub=None, want_dvf=True):
    """y = sum_j softmax_j(a) (vf[idx] + pos) [+ global token] [+ residual] in fp64 and, given dy, da, dvf, dpos, da_g, dv_g
    by autograd (the residual's gradient is dy itself, handed through: the callers compare it bit for bit).  Returns
    (ref, env): dicts of fp64 tensors keyed by output name.  ``want_dvf=False`` leaves the value table's gradient out (tens of
    millions of fp64 atomics onto a four-row table, for a caller that checks the scatter elsewhere)."""
    st = a.dtype
    us = storage_unit(st)
    uo = us if st is torch.bfloat16 else 0.0
    B, n, k, d = a.shape
    leaf = lambda t: None if t is None else t.detach().double().requires_grad_(True)
    a64, vf64, pos64, ag64, vg64, r64 = map(leaf, (a, vf, pos, a_g, v_g, residual))
    N = vf.shape[1] if vf is not None else 1
    qpt = None
    if sub is not None:
        s, S_f, S_b, qpt = _sub_magnitudes(vf64, pos64, idx, sub)
        S_f, S_b = S_f.detach(), S_b.detach()
    else:
        s = pos64 if vf is None else gather(vf64, idx) + pos64
        S_f = S_b = s.detach().abs()
    acat, scat = a64, s
    if a_g is not None:
        acat = torch.cat([a64, ag64[:, None, None, :].expand(B, n, 1, d)], dim=2)
        scat = torch.cat([s, vg64[:, None, None, :].expand(B, n, 1, d)], dim=2)
        tok = vg64.detach().abs()[:, None, None, :].expand(B, n, 1, d)
        S_f, S_b = torch.cat([S_f, tok], dim=2), torch.cat([S_b, tok], dim=2)
    w = torch.softmax(acat, dim=2)
    yb = (w * scat).sum(dim=2)
    y = yb if residual is None else yb + r64
    ref = {"y": y.detach()}
    with torch.no_grad():
        lse = torch.logsumexp(acat, dim=2, keepdim=True)
        c = 3.0 + (acat - lse).abs() + lse.abs() + acat.abs()
        rmag = 0.0 if residual is None else r64.abs()
        ymag = y.abs() + rmag
        flushed = (w < 2.0 * FLUSH).double() * FLUSH          # |error| of a weight the hardware exp2 returns as zero
        env = {"y": U32 * (w * S_f * c).sum(dim=2) + (flushed * S_f).sum(dim=2) + us * ymag + FLOOR}
    if dy is None:
        return ref, env
    dy64 = _d(dy)
    ins = {"da": a64, "dvf": vf64, "dpos": pos64, "da_g": ag64, "dv_g": vg64}
    ins = {kk: v for kk, v in ins.items() if v is not None and (kk != "dvf" or want_dvf)}
    grads = torch.autograd.grad(y, list(ins.values()), dy64)
    ref.update({kk: g.detach() for kk, g in zip(ins, grads)})
    with torch.no_grad():
        wd, ybd, sd = w.detach(), yb.detach().unsqueeze(2), scat.detach()
        gm = dy64.abs().unsqueeze(2)
        if qpt is not None:          # backward of the per-point sub form: yb + q_i against u + (v + k)[idx]
            Yb = (yb.detach().abs() + (yb.detach() + qpt).abs()).unsqueeze(2)
        else:
            Yb = ybd.abs()
        gate = us if residual is not None else us - U32
        dpos_all = wd * dy64.unsqueeze(2)
        da_all = dpos_all * (sd - ybd)
        e_w = U32 * gm * wd * c + flushed * gm
        e_da = (U32 * gm * wd * (c * (sd - ybd).abs() + S_b + Yb + (wd * S_b).sum(dim=2, keepdim=True))
                + gate * gm * wd * ymag.unsqueeze(2) + flushed * gm * (sd - ybd).abs())
        env["dpos"] = e_w[:, :, :k] + us * dpos_all[:, :, :k].abs() + FLOOR
        env["da"] = e_da[:, :, :k] + us * da_all[:, :, :k].abs() + FLOOR
        if vf is not None and want_dvf:
            env["dvf"] = (scatter(env["dpos"], idx, N) + counts(idx, N) * U32 * scatter(dpos_all[:, :, :k].abs(), idx, N)
                          + uo * ref["dvf"].abs() + FLOOR)
        if a_g is not None:          # the token's addends: one per centre, partial sums kept in fp32
            for name, add, e in (("da_g", da_all[:, :, k], e_da[:, :, k]), ("dv_g", dpos_all[:, :, k], e_w[:, :, k])):
                L = (add != 0).sum(dim=1).double() + 1.0          # (adding an exact zero rounds nothing)
                env[name] = e.sum(dim=1) + L * U32 * add.abs().sum(dim=1) + uo * ref[name].abs() + FLOOR
        # the closed form the envelope is built on is the autograd gradient (a check of this file, not of a kernel)
        # (to a thousandth of an envelope: the two fp64 evaluations cancel differently)
        assert bool(((da_all[:, :, :k] - ref["da"]).abs() <= 1e-3 * env["da"]).all())
        assert bool(((dpos_all[:, :, :k] - ref["dpos"]).abs() <= 1e-3 * env["dpos"]).all())
    return ref, env


def emulate_post(a, vf, pos, idx, a_g=None, v_g=None, residual=None, dy=None, sub=None):
    """attn_post_fwd / attn_post_bwd as the header of csrc/attention.hip states them, in torch fp32: the online softmax over
    the neighbours (the global token first), lse = m + log(l), y = acc / l + r rounded to the storage type; backward from
    the stored y and the fp32 lse: yb = y - r, w_j = exp(a_j - lse), dpos_j = w_j dy, da_j = dpos_j (s_j - yb)."""
    st = a.dtype
    f = lambda t: None if t is None else t.detach().float()
    af, vff, posf, agf, vgf, rf = map(f, (a, vf, pos, a_g, v_g, residual))
    B, n, k, d = a.shape
    N = vf.shape[1] if vf is not None else 1
    qpt = None
    if sub is not None:
        kf, q = f(sub[0]), f(sub[1])
        per_shape = q.shape[1] == 1 and n != 1
        tab = vff + kf if kf is not None else vff
        if per_shape:
            tab = tab - q
        else:
            qpt = q
        g = gather(tab, idx)
        sv = posf + (g - qpt.unsqueeze(2)) if qpt is not None else posf + g
        sv_b = posf + g
    else:
        sv = posf if vf is None else posf + gather(vff, idx)
        sv_b = sv
    if a_g is not None:
        m = agf[:, None, :].expand(B, n, d).clone()
        acc = vgf[:, None, :].expand(B, n, d).clone()
        l = torch.ones(B, n, d)
    else:
        m = torch.full((B, n, d), float("-inf"))
        l = torch.zeros(B, n, d)
        acc = torch.zeros(B, n, d)
    m, l, acc = m.to(a.device), l.to(a.device), acc.to(a.device)
    for j in range(k):
        mn = torch.maximum(m, af[:, :, j])
        sc, wj = torch.exp(m - mn), torch.exp(af[:, :, j] - mn)
        l = l * sc + wj
        acc = acc * sc + wj * sv[:, :, j]
        m = mn
    lse = m + torch.log(l)
    y = acc / l
    if residual is not None:
        y = y + rf
    y = y.to(st)
    out = {"y": y}
    if dy is None:
        return out
    g = f(dy)
    yb = y.float()
    if residual is not None:
        yb = yb - rf
    if qpt is not None:
        yb = yb + qpt
    ds = torch.exp(af - lse.unsqueeze(2)) * g.unsqueeze(2)
    da = ds * (sv_b - yb.unsqueeze(2))
    out.update(da=da.to(st), dpos=ds.to(st))
    if vf is not None:
        out["dvf"] = scatter(ds, idx, N).to(st)
    if a_g is not None:
        dsg = torch.exp(agf[:, None, :] - lse) * g
        out["da_g"] = (dsg * (vgf[:, None, :] - yb)).sum(dim=1).to(st)
        out["dv_g"] = dsg.sum(dim=1).to(st)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# comparison
# ----------------------------------------------------------------------------------------------------------------------
def measure(got, ref, env):
    """{name: E} for every tensor of ``ref`` (``got`` must hold them all; shapes must agree)."""
    out = {}
    for name, r in ref.items():
        g = got[name]
        assert g is not None and tuple(g.shape) == tuple(r.shape), (name, None if g is None else tuple(g.shape), tuple(r.shape))
        ratio = (g.detach().double() - r).abs() / env[name]
        ratio = torch.nan_to_num(ratio, nan=float("inf"))
        out[name] = float(ratio.max()) if ratio.numel() else 0.0
    return out


def assert_within(got, ref, env, bound, what=""):
    """Every tensor within ``bound`` envelopes of the reference, element by element; returns {name: E}."""
    E = measure(got, ref, env)
    bad = {kk: v for kk, v in E.items() if not v <= bound}
    assert not bad, f"{what}: outside {bound:g} envelopes: {bad} (all: {E})"
    return E


# ----------------------------------------------------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------------------------------------------------
SWEEP_SHAPES = {           # (B, n, N, k, d), token: one shape per form of the `post` backward
    "lds": ((3, 20, 5, 3, 8), True),
    "stream": ((2, 37, 50, 10, 120), False),
    "atomic": ((2, 37, 50, 10, 120), False),
    "det": ((2, 33, 100, 5, 208), True),
}
SPREADS, OFFSETS, RSCALES = (0.0, 1.0, 30.0), (0.0, 1000.0, -1000.0), (0.0, 1.0, 2.0 ** 6, 2.0 ** 12)


def conditioning_cases(token):
    """(spread, offset, residual scale, token logit) of the sweep; token logit: None / "rand" / "hi" (largest neighbour
    logit + 40: the neighbours' weights underflow) / "lo" (smallest - 40: the token's gradient is ~1e-17 of the others)."""
    cases = [(sp, off, rs, "rand" if token else None) for sp in SPREADS for off in OFFSETS for rs in RSCALES]
    if token:
        cases += [(1.0, 0.0, 1.0, "hi"), (1.0, 0.0, 1.0, "lo"), (30.0, 1000.0, 0.0, "hi"), (30.0, -1000.0, 2.0 ** 6, "lo")]
    return cases


def make_post_case(shape, seed, dtype=torch.float32, device="cpu", spread=1.0, offset=0.0, rscale=1.0, token=None,
                   has_v=True, hot=False):
    """Inputs of one attn_post call in the storage type ``dtype``: dict(a, vf, pos, idx, a_g, v_g, residual, dy)."""
    B, n, N, k, d = shape
    g = torch.Generator().manual_seed(seed)
    big = B * n * k * d > (1 << 22)
    if big:                      # (drawn on the device: tens of millions of elements)
        g = torch.Generator(device=device).manual_seed(seed)
        mk = lambda *s: torch.randn(*s, generator=g, device=device)
        idx = torch.randint(0, N, (B, n, k), generator=g, device=device, dtype=torch.int32)
    else:
        mk = lambda *s: torch.randn(*s, generator=g).to(device)
        idx = torch.randint(0, N, (B, n, k), generator=g, dtype=torch.int32).to(device)
    if hot:
        idx[:, :, 0] = min(5, N - 1)
    a = (mk(B, n, k, d) * spread + offset).to(dtype)
    c = dict(a=a, vf=mk(B, N, d).to(dtype) if has_v else None, pos=mk(B, n, k, d).to(dtype), idx=idx, a_g=None, v_g=None,
             residual=(mk(B, n, d) * rscale).to(dtype) if rscale else None, dy=mk(B, n, d).to(dtype))
    if token:
        af = a.float()
        if token == "hi":
            a_g = af.amax(dim=(1, 2)) + 40.0
        elif token == "lo":
            a_g = af.amin(dim=(1, 2)) - 40.0
        else:
            a_g = mk(B, d) * spread + offset
        c["a_g"], c["v_g"] = a_g.to(dtype), mk(B, d).to(dtype)
    return c
