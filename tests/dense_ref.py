"""fp64 reference, per-element error envelope and CPU emulations of the dense-layer kernels (csrc/gemm.hip, gemm_bf16x3.hip /
x3_kernel.h, wgrad_bf16x3.hip, gemm_bf16.hip, k4*.h).

Plain torch, any device.  Four things live here:

* ``forward_reference`` / ``wgrad_reference``: the two operations in fp64 from the exact upcasts of the tensors the kernel
  receives,

      y  = post(pre(x) W^T + b +- residual) * (out_mask > 0) + addend + (gq[r / g_div] - gk[shape(r) * nsrc + gidx[r]])
           (the one-table gather form adds gk[shape(r) * nsrc + gidx[r]], a table that holds the difference already)
      dW = (dy * (mask > 0))^T pre(x) (+ existing),   db = column sums of dy * (mask > 0) (+ existing)

  pre = the mask prologue ``x * (mask > 0)`` and / or ReLU, post = ReLU.
* the envelope ``env`` of every output element: the first-order rounding bound of a dot product in fp32, evaluated in fp64.
  With u = 2^-24, u_s the unit of the output storage (u, or 2^-9 for bf16), x' = pre(x), the sums over the reduction index:

      env(y)  = gate * (u (sum |x'||w| + |b| + |res|) + floor) + u (|addend| + |gq| + |gk|) + u_s |y|
      env(dW) = u (sum |dy'||x'| + |existing|) + floor,      env(db) = u (sum |dy'| + |existing|) + M 2^-149
      floor   = 2^-126 sum (|x'| [w != 0] + |w| [x' != 0]) + K 2^-149           (K: the number of addends)

  gate = [out_mask > 0] (a gated element is an exact zero).  There is no absolute constant and no scaling by the tensor's
  maximum: an element whose envelope is zero must be exact.  ``floor`` is the absolute term of the bf16x3 split on the flush-safe
  side: a plane (h, m, l) of an operand that falls under the smallest normal bf16, 2^-126, may be lost whole, an absolute error
  of the operand of up to 2^-126, times the other operand; the fp32 accumulator below 2^-126 rounds at 2^-149 per addend.
  The metric is E = max over elements of |got - ref64| / env.
* ``emulate_forward`` / ``emulate_wgrad``: the kernels' documented arithmetic on the CPU, per family
    "x3"    the bf16x3 split, x = h + m + l by round-to-nearest bf16 of the exact residuals, the six products h wh, h wm, m wh,
            m wm, h wl, l wh (exact in the matrix pipe), k blocks of 32, fp32 accumulators;
    "f32"   the exact-fp32 chain (MFMA blocks of 4);
    "bf16"  bf16 operands (exact products), k blocks of 32, fp32 accumulators, bf16 or fp32 output;
  each in two accumulation models -- "block": the products of one k block and plane are summed exactly and rounded once into
  the accumulator; "product": every product is rounded into the accumulator on its own.  How the matrix pipe rounds inside a
  block is not documented, so E_EMUL of a family is the larger of the two.  Weight gradients follow the documented structure:
  32-row slabs, a run of slabs per workgroup into one partial, then a fixed-order sum of the partials.
  ``drop=i`` leaves product i of the six out (the mutation of tests/test_dense_ref_cpu.py).
* ``make_case``: the one case generator, see KINDS.

E_EMUL per family, kind and K in {36, 200, 256} is the largest E the two models reach (tests/test_dense_ref_cpu.py measures
and asserts it); the GPU tests allow BOUND = 2 max(1, E_EMUL): a factor 2 over the reference's own emulation for the accumulation
order nobody has pinned down.  It is never fitted to a kernel's output.
"""
from __future__ import annotations

import torch

U32 = 2.0 ** -24
U_BF16 = 2.0 ** -9
TINY = 2.0 ** -126          # the smallest normal fp32 / bf16
DENORM = 2.0 ** -149        # the smallest fp32 subnormal
F32, BF = torch.float32, torch.bfloat16
GPU_FACTOR = 2.0

KINDS = ("unit", "rows", "elems", "cancel", "tiny", "floor", "ints", "predicates")
BOUNDED_KINDS = ("unit", "rows", "elems", "cancel", "tiny")          # the kinds every bounded GPU case runs
PLANES = ((0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0))           # (plane of x, plane of w): h wh, h wm, m wh, m wm, h wl, l wh
PLANE_NAMES = ("h*wh", "h*wm", "m*wh", "m*wm", "h*wl", "l*wh")

# Measured by tests/test_dense_ref_cpu.py::test_emulations_stay_inside_the_envelope (CPU emulation, the larger of the two
# accumulation models, over the conditioning shapes and every case of the GPU file), rounded up to the next half.  Forward:
# per family, kind and reduction length class (K <= 64 / <= 200 / <= 256, named 36 / 200 / 256); weight gradients (the
# reduction runs over thousands of rows in per-workgroup partials): per family and kind.
E_EMUL = {
    "fwd": {
        "x3": {
            "unit": {36: 6.5, 200: 7.0, 256: 7.5},
            "rows": {36: 6.5, 200: 8.0, 256: 6.5},
            "elems": {36: 6.5, 200: 9.0, 256: 9.5},
            "cancel": {36: 6.5, 200: 6.5, 256: 6.0},
            "tiny": {36: 6.5, 200: 5.5, 256: 6.0},
            "floor": {36: 0.5, 200: 0.5, 256: 0.5},
        },
        "f32": {
            "unit": {36: 3.0, 200: 4.0, 256: 4.5},
            "rows": {36: 2.5, 200: 3.5, 256: 4.0},
            "elems": {36: 4.0, 200: 7.0, 256: 8.5},
            "cancel": {36: 2.0, 200: 2.5, 256: 4.0},
            "tiny": {36: 2.5, 200: 3.5, 256: 4.5},
            "floor": {36: 0.5, 200: 0.5, 256: 0.5},
        },
        "bf16": {
            "unit": {36: 2.5, 200: 2.5, 256: 3.0},
            "rows": {36: 2.5, 200: 2.5, 256: 2.5},
            "elems": {36: 3.5, 200: 7.5, 256: 8.0},
            "cancel": {36: 2.0, 200: 2.0, 256: 2.0},
            "tiny": {36: 2.5, 200: 2.5, 256: 2.5},
            "floor": {36: 1.0, 200: 0.5, 256: 0.5},
        },
    },
    "wgrad": {
        "x3": {"unit": 1.5, "rows": 4.0, "elems": 9.5, "cancel": 1.5, "tiny": 1.5, "floor": 0.5},
        "f32": {"unit": 3.0, "rows": 3.5, "elems": 7.0, "cancel": 1.5, "tiny": 2.5, "floor": 2.0},
        "bf16": {"unit": 2.0, "rows": 5.5, "elems": 7.5, "cancel": 1.0, "tiny": 2.0, "floor": 0.5},
    },
}


def k_class(K):
    return 36 if K <= 64 else 200 if K <= 200 else 256


def e_emul(op, family, kind, K=None):
    e = E_EMUL[op][family][kind]
    return e[k_class(K)] if op == "fwd" else e


def bound(op, family, kind, K=None):
    """The GPU bound of one family, kind (and reduction length), in envelopes."""
    return GPU_FACTOR * max(1.0, e_emul(op, family, kind, K))


def storage_unit(dtype):
    return U_BF16 if dtype is BF else U32


def _d(t):
    return None if t is None else t.detach().double()


# ----------------------------------------------------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------------------------------------------------
def special_values(dtype):
    """The values at which implementations of ``mask > 0`` / ``max(x, 0)`` differ: signed zeros, the smallest subnormals of the
    storage type (2^-149 fp32, 2^-133 bf16), and one ordinary value of either sign."""
    t = DENORM if dtype is F32 else 2.0 ** -133
    return torch.tensor([-0.0, 0.0, t, -t, 1.0, -1.0], dtype=torch.float64)


class _Draw:
    """Random tensors of one case: on the CPU, or on the device for tensors of tens of millions of elements."""

    def __init__(self, seed, device, big):
        self.dev = torch.device(device)
        self.gdev = self.dev if big else torch.device("cpu")
        self.g = torch.Generator(device=self.gdev).manual_seed(seed)

    def randn(self, *s):
        return torch.randn(*s, generator=self.g, device=self.gdev).to(self.dev)

    def uniform(self, *s):
        return (torch.rand(*s, generator=self.g, device=self.gdev) * 2.0 - 1.0).to(self.dev)

    def ints(self, lo, hi, *s):
        return torch.randint(lo, hi + 1, s, generator=self.g, device=self.gdev).float().to(self.dev)

    def pow2(self, lo, hi, *s):
        return torch.pow(2.0, self.ints(lo, hi, *s).double()).float()

    def pick(self, values, *s):
        i = torch.randint(0, values.numel(), s, generator=self.g, device=self.gdev).to(self.dev)
        return values.to(self.dev)[i]          # (fp64: the caller casts to the storage type, which holds every value)


def make_case(kind, M, K, N, flags=(), seed=0, device="cpu", dtype=F32, op="fwd"):
    """Inputs of one dense-layer call as a dict.  ``op`` "fwd": x [M,K], w [N,K] and, by ``flags`` ("bias", "res", "res-": the
    residual subtracted, "mask", "relu_in", "relu_out", "omask", "addend", "gather", "gather1"), b, res, res_sign, mask [M,K],
    out_mask [M,N], addend [M,N], gather = (gq, g_div, gk, gidx, rows_per_shape, nsrc).  ``op`` "wgrad": dy [M,N], x [M,K] and, by
    flags ("mask", "relu_x", "acc"), mask [M,N], acc_w [N,K], acc_b [N]: an existing gradient of 2^20 times the update, element
    by element (integers of [-8, 8] in the exact kinds).  ``dtype`` bf16: the activations (x, res, masks, dy) in bf16 and a weight
    that holds bf16 values (the bf16 kernels round their weight pack).

    kind       inputs
    unit       randn, w / sqrt(K)
    rows       row scales 2^j, j uniform in [-40, 40], on x (and res, addend) / on dy; bias with column scales of the same range
    elems      element scales 2^j, j in [-12, 12], on both operands
    cancel     |y| <= 2^-10 sum |x||w|: pairs of columns k, k + K / 2 (another k block: the accumulators carry the large partial
               sums) holding (x, 3 x (1 + 2^-11 t)), |t| <= 1, with the weights (w, -w / 3) -- a factor 3, not 1, so that the bf16
               planes of a pair are unrelated and a lost plane cannot cancel with itself; masks equal within a pair; bias,
               residual and addend 2^-12 of a unit.  Weight gradients: pairs of rows m, m + M / 2
    tiny       every row at 2^-100
    floor      every row at 2^-118
    ints       integers of [-8, 8] for every operand, bias, residual, addend and tables included
    predicates ints, with masks and pre-ReLU inputs drawn from special_values(dtype)
    """
    assert kind in KINDS and op in ("fwd", "wgrad")
    flags = tuple(flags)
    d = _Draw(seed, device, M * max(K, N) > (1 << 22))
    exact = kind in ("ints", "predicates")
    st = lambda t: None if t is None else t.to(dtype)
    rs = {"tiny": 2.0 ** -100, "floor": 2.0 ** -118}.get(kind, 1.0)
    mk = (lambda *s: d.ints(-8, 8, *s)) if exact else d.randn
    special = special_values(dtype)
    c = {"kind": kind, "op": op, "flags": flags, "dtype": dtype, "M": M, "K": K, "N": N}

    def mask_like(*s):
        return d.pick(special, *s).to(dtype) if kind == "predicates" else st(mk(*s))

    if op == "wgrad":
        dy, x = mk(M, N), mk(M, K)
        if kind == "rows":
            dy = dy * d.pow2(-40, 40, M, 1)
        elif kind == "elems":
            dy, x = dy * d.pow2(-12, 12, M, N), x * d.pow2(-12, 12, M, K)
        elif kind == "cancel":
            h = M // 2          # (row i pairs with row i + M / 2: the partner lies in another slab, mostly another workgroup)
            dy[h:2 * h] = -dy[:h] / 3.0
            x[h:2 * h] = 3.0 * x[:h] * (1.0 + 2.0 ** -11 * d.uniform(h, K))
            if M % 2:
                dy[M - 1] = 0.0
        dy = dy * rs
        mask = mask_like(M, N) if "mask" in flags else None
        if kind == "cancel" and mask is not None:
            mask[M // 2:2 * (M // 2)] = mask[:M // 2]
        if kind == "predicates" and "relu_x" in flags:
            x = d.pick(special, M, K).float()
        c.update(dy=st(dy), x=st(x), mask=mask, relu_x="relu_x" in flags, acc_w=None, acc_b=None)
        if "acc" in flags:
            if exact:
                c["acc_w"], c["acc_b"] = d.ints(-8, 8, N, K), d.ints(-8, 8, N)
            else:
                ref, _ = wgrad_reference(c)
                sgn = lambda *s: torch.where(d.uniform(*s) < 0, -1.0, 1.0).double()
                c["acc_w"] = (ref["dw"] * 2.0 ** 20 * sgn(N, K)).float()
                c["acc_b"] = (ref["db"] * 2.0 ** 20 * sgn(N)).float()
        return c

    x = mk(M, K)
    w = mk(N, K) if exact else mk(N, K) * K ** -0.5
    side = 2.0 ** -12 if kind == "cancel" else 1.0
    row = None
    if kind == "rows":
        row = d.pow2(-40, 40, M, 1)
        x = x * row
    elif kind == "elems":
        x, w = x * d.pow2(-12, 12, M, K), w * d.pow2(-12, 12, N, K)
    elif kind == "cancel":
        assert K % 2 == 0
        x[:, K // 2:] = 3.0 * x[:, :K // 2] * (1.0 + 2.0 ** -11 * d.uniform(M, K // 2))
        w[:, K // 2:] = -w[:, :K // 2] / 3.0
    x = x * rs
    if kind == "predicates" and "relu_in" in flags:
        x = d.pick(special, M, K).float()
    if dtype is BF:
        w = w.to(BF).float()

    def rowwise(*s):          # a per-row operand of the epilogue at the scale of its row
        t = mk(*s) * side * rs
        return t * row if row is not None else t

    b = None
    if "bias" in flags:
        b = mk(N) * side * rs
        if kind == "rows":
            b = b * d.pow2(-40, 40, N)
    mask = mask_like(M, K) if "mask" in flags else None
    if kind == "cancel" and mask is not None:
        mask[:, K // 2:] = mask[:, :K // 2]
    c.update(x=st(x), w=w, b=b, res=st(rowwise(M, N)) if ("res" in flags or "res-" in flags) else None,
             res_sign=-1.0 if "res-" in flags else 1.0, mask=mask, out_mask=mask_like(M, N) if "omask" in flags else None,
             addend=st(rowwise(M, N)) if "addend" in flags else None, relu_in="relu_in" in flags, relu_out="relu_out" in flags,
             gather=None)
    if "gather" in flags or "gather1" in flags:
        g_div, nsrc, rps = 4, 16, max(1, (M + 2) // 3)
        shapes = (M + rps - 1) // rps
        gk = mk(shapes * nsrc, N) * side * rs
        gq = mk((M + g_div - 1) // g_div, N) * side * rs if "gather" in flags else None
        gidx = torch.randint(0, nsrc, (M,), generator=d.g, device=d.gdev).int().to(d.dev)
        c["gather"] = (gq, g_div if gq is not None else 1, gk, gidx, rps, nsrc)
    return c


def take_rows(c, idx):
    """The forward case restricted to the rows ``idx`` (a long tensor): what a sampled comparison of a large case judges."""
    out = dict(c)
    for kk in ("x", "res", "mask", "out_mask", "addend"):
        if c.get(kk) is not None:
            out[kk] = c[kk][idx]
    if c.get("gather") is not None:
        out["gather"], out["gather_add"] = None, gather_terms(c, idx)
    out["M"] = int(idx.numel())
    return out


def gather_terms(c, rows=None):
    """(gq rows or None, gk rows) of the gathered addend gq[r / g_div] - gk[(r / rows_per_shape) * nsrc + gidx[r]], per row
    (gq None: the one-table form, whose gk rows are added)."""
    if c.get("gather_add") is not None:
        return c["gather_add"]
    gq, g_div, gk, gidx, rps, nsrc = c["gather"]
    r = torch.arange(c["M"], device=gk.device) if rows is None else rows
    kk = gk[(r // rps) * nsrc + gidx.long()[r]]
    return (None if gq is None else gq[r // g_div]), kk


def _pre(x, mask, relu):
    """The prologues on a tensor of any floating type: the decisions are taken on the values themselves."""
    if mask is not None:
        x = torch.where(mask > 0, x, torch.zeros_like(x))
    if relu:
        x = torch.where(x > 0, x, torch.zeros_like(x))
    return x


# ----------------------------------------------------------------------------------------------------------------------
# fp64 references and envelopes
# ----------------------------------------------------------------------------------------------------------------------
def _floor(a, bt, count):
    """2^-126 sum_k (|a_k| [b_k != 0] + |b_k| [a_k != 0]) + count 2^-149 for the products a @ bt (fp64 operands)."""
    return TINY * (a.abs() @ (bt != 0).double() + (a != 0).double() @ bt.abs()) + count * DENORM


def forward_reference(c, out_dtype=None, with_floor=True):
    """(ref, env): fp64 tensors [M, N] of one forward case.  ``out_dtype``: the storage type of the output (default: the case's
    activations' type).  ``with_floor=False`` leaves the floor term out (what the floor tests print)."""
    us = storage_unit(out_dtype if out_dtype is not None else c["dtype"])
    xp = _pre(_d(c["x"]), c["mask"], c["relu_in"])
    wt = _d(c["w"]).t()
    z = xp @ wt
    mag = xp.abs() @ wt.abs()
    if c["b"] is not None:
        z, mag = z + _d(c["b"]), mag + _d(c["b"]).abs()
    if c["res"] is not None:
        z, mag = z + c["res_sign"] * _d(c["res"]), mag + _d(c["res"]).abs()
    if c["relu_out"]:
        z = z.clamp_min(0.0)          # (|relu(a) - relu(b)| <= |a - b|: the envelope of the pre-activation holds)
    env = U32 * mag
    if with_floor:
        env = env + _floor(xp, wt, c["K"])
    if c["out_mask"] is not None:
        gate = (c["out_mask"] > 0).double()
        z, env = z * gate, env * gate
    if c["addend"] is not None:
        z, env = z + _d(c["addend"]), env + U32 * _d(c["addend"]).abs()
    if c.get("gather") is not None or c.get("gather_add") is not None:
        q, kk = gather_terms(c)          # (two tables: q - k; one table: it holds the difference and is added)
        z, env = (z - _d(kk) if q is not None else z + _d(kk)), env + U32 * _d(kk).abs()
        if q is not None:
            z, env = z + _d(q), env + U32 * _d(q).abs()
    return z, env + us * z.abs()


def wgrad_reference(c, with_floor=True):
    """(ref, env): dicts {"dw": [N,K], "db": [N]} of fp64 tensors of one weight-gradient case."""
    dyp = _pre(_d(c["dy"]), c["mask"], False)
    xp = _pre(_d(c["x"]), None, c["relu_x"])
    M = c["M"]
    ref = {"dw": dyp.t() @ xp, "db": dyp.sum(0)}
    env = {"dw": U32 * (dyp.abs().t() @ xp.abs()), "db": U32 * dyp.abs().sum(0) + M * DENORM}
    if with_floor:
        env["dw"] = env["dw"] + _floor(dyp.t(), xp, M)
    if c.get("acc_w") is not None:
        ref["dw"], env["dw"] = ref["dw"] + _d(c["acc_w"]), env["dw"] + U32 * _d(c["acc_w"]).abs()
        ref["db"], env["db"] = ref["db"] + _d(c["acc_b"]), env["db"] + U32 * _d(c["acc_b"]).abs()
    return ref, env


def predicate_tolerance(c, ref, out_dtype, count):
    """Tolerance of the predicates kind, per element: every operand is a whole number but the subnormals that passed a
    predicate, and an addend that carries one may move a rounding of the accumulator by an ulp: ``count`` addends times
    2 u times the magnitudes (2 count envelopes of the fp32 part), plus half an ulp of a bf16 output.  A wrong decision is an
    error of one at least; the callers assert that the tolerance stays under a half."""
    if c["op"] == "fwd":
        _, env = forward_reference(c, out_dtype=F32)
        env = env - U32 * ref.abs()
    else:
        env = wgrad_reference(c)[1]
    tol = {kk: 2.0 * count * v for kk, v in env.items()} if isinstance(env, dict) else 2.0 * count * env
    if out_dtype is BF:
        tol = tol + 2.0 ** -8 * ref.abs()
    return tol


def measure(got, ref, env):
    """E = max |got - ref| / env over the elements; an element with a zero envelope must be exact."""
    assert tuple(got.shape) == tuple(ref.shape), (tuple(got.shape), tuple(ref.shape))
    diff = (got.detach().double() - ref).abs()
    ratio = torch.where(diff == 0, torch.zeros_like(diff), diff / env)
    ratio = torch.nan_to_num(ratio, nan=float("inf"), posinf=float("inf"))
    return float(ratio.max()) if ratio.numel() else 0.0


# ----------------------------------------------------------------------------------------------------------------------
# emulations
# ----------------------------------------------------------------------------------------------------------------------
def split3(x):
    """x (fp32) -> its bf16 planes (h, m, l) as fp32 tensors: round to nearest, residuals exact."""
    h = x.to(BF).float()
    r = x - h
    m = r.to(BF).float()
    l = (r - m).to(BF).float()
    return h, m, l


def _operands(a, b, family):
    """The operand planes and plane pairs of a family, and its block length."""
    if family == "x3":
        return split3(a.float()), split3(b.float()), PLANES, 32
    return (a.float(),), (b.float(),), ((0, 0),), (4 if family == "f32" else 32)


def _accumulate(acc, ap, bp, pairs, blk, model, drop):
    """acc [.., R, C] (fp32) += sum over the last axis of ap[i] [.., R, L] and bp[j] [.., C, L], plane pair by plane pair."""
    L = ap[0].shape[-1]
    pairs = [p for n, p in enumerate(pairs) if n != drop]
    if model == "block":
        for k0 in range(0, L, blk):
            for i, j in pairs:
                part = ap[i][..., k0:k0 + blk].double() @ bp[j][..., k0:k0 + blk].double().transpose(-1, -2)
                acc = (acc.double() + part).float()
        return acc
    for k in range(L):
        for i, j in pairs:
            # one product, exact in fp64 (bf16 x bf16 fits fp32, fp32 x fp32 fits fp64), one rounding of the sum: an fma
            acc = (acc.double() + ap[i][..., k].double().unsqueeze(-1) * bp[j][..., k].double().unsqueeze(-2)).float()
    return acc


def emulate_forward(c, family, model="block", drop=None, out_dtype=None, neighbour=None):
    """One forward case as family ``family`` computes it: the accumulators start from the signed residual, walk the k blocks,
    then bias, ReLU, output mask, addend and gathered addend in fp32, one rounding each, and the store.
    ``neighbour`` "res" / "bias": the mutation that takes the residual of the next row / the bias of the next column."""
    out_dtype = out_dtype if out_dtype is not None else c["dtype"]
    xp = _pre(c["x"], c["mask"], c["relu_in"])
    M, N = c["M"], c["N"]
    acc = torch.zeros(M, N)
    res, b = c["res"], c["b"]
    if res is not None:
        res = torch.roll(res, -1, 0) if neighbour == "res" else res
        acc = c["res_sign"] * res.float()
    a, w, pairs, blk = _operands(xp, c["w"], family)
    acc = _accumulate(acc, a, w, pairs, blk, model, drop)
    if b is not None:
        acc = acc + (torch.roll(b, -1, 0) if neighbour == "bias" else b)
    if c["relu_out"]:
        acc = acc.clamp_min(0.0)
    if c["out_mask"] is not None:
        acc = torch.where(c["out_mask"] > 0, acc, torch.zeros_like(acc))
    if c["addend"] is not None:
        acc = acc + c["addend"].float()
    if c.get("gather") is not None:
        q, kk = gather_terms(c)
        acc = acc + ((q - kk) if q is not None else kk)
    return acc.to(out_dtype)


def wgrad_plan(M):
    """(workgroups, 32-row slabs per workgroup) of the emulated weight gradient: at least four slabs per workgroup, at most 256
    workgroups (the shape of wgrad_bf16x3.hip's plan on a 256-CU device)."""
    slabs = (M + 31) // 32
    grid = max(1, min(256, slabs // 4))
    per = (slabs + grid - 1) // grid
    return (slabs + per - 1) // per, per


def emulate_wgrad(c, family, model="block", drop=None):
    """One weight-gradient case: 32-row slabs accumulated per workgroup, the partials summed in workgroup order, the existing
    gradient added last.  Returns {"dw", "db"} in fp32."""
    dyp = _pre(c["dy"], c["mask"], False).float()
    xp = _pre(c["x"], None, c["relu_x"]).float()
    M, N, K = c["M"], c["N"], c["K"]
    G, per = wgrad_plan(M)
    pad = G * per * 32 - M          # (zero rows: adding exact zeros rounds nothing)
    grp = lambda t: torch.cat([t, torch.zeros(pad, t.shape[1])]).reshape(G, per * 32, -1).transpose(1, 2).contiguous()
    a, b, pairs, blk = _operands(grp(dyp), grp(xp), family)
    part = _accumulate(torch.zeros(G, N, K), a, b, pairs, blk if family != "x3" else 32, model, drop)
    pb = torch.zeros(G, N)
    dyg = grp(dyp)
    for r in range(per * 32):          # the bias gradient: plain fp32 sums of the rows
        pb = pb + dyg[:, :, r]
    dw, db = torch.zeros(N, K), torch.zeros(N)
    for g in range(G):
        dw, db = dw + part[g], db + pb[g]
    if c.get("acc_w") is not None:
        dw, db = c["acc_w"] + dw, c["acc_b"] + db
    return {"dw": dw, "db": db}


# ----------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_dense_forms_gpu.py (shared with tests/test_dense_ref_cpu.py, which proves for each of them that a
# lost product of the split and a neighbour's bias / residual lie outside the bound)
# ----------------------------------------------------------------------------------------------------------------------
# Row counts of the bf16x3 forward forms: "tile" = rows_per_workgroup - 5 (one workgroup tile with a ragged last row tile) and
# "grid" = num_cus * wgs_per_cu * grid_rows + 77, read from the device (some workgroups take a second tile).
X3_FORWARD = [
    # id, branch of launch_x3, (K, N), flags, traced variant <MT,NT,PRE,WV,XREG>xW, rows per workgroup, workgroups per CU,
    # nsdp_debug_set(6, .) value, rows per workgroup slot of the "grid" count
    ("resident-pre0", "resident weights, plain", (36, 40), ("bias", "res"), "linear_bf16x3<2,4,0,8,0>x1 wres", 256, 1, 0, 256),
    ("resident-pre2", "resident weights, ReLU", (36, 120), ("bias", "relu_in", "relu_out"), "linear_bf16x3<2,8,2,8,0>x1 wres", 256, 1, 0, 256),
    ("two-wg-pre0", "two 4-wave workgroups", (200, 120), ("bias",), "linear_bf16x3<2,8,0,4,0>x2", 128, 2, 0, 128),
    ("two-wg-pre2", "two 4-wave workgroups, ReLU", (256, 40), ("relu_in",), "linear_bf16x3<2,4,2,4,0>x2", 128, 2, 0, 128),
    ("nt13-xreg", "13 n tiles, register activations", (36, 200), ("bias", "res", "relu_out"), "linear_bf16x3<2,13,0,4,1>x2", 128, 2, 0, 128),
    ("nt13-xreg-pre2", "13 n tiles, register activations, ReLU", (200, 200), ("bias", "relu_in"), "linear_bf16x3<2,13,2,4,1>x2", 128, 2, 0, 128),
    # 16 n tiles: the launcher takes 2 row tiles per wave where that saves a round of the grid, 3 otherwise; a single tile is
    # always narrow, so the wide form at these row counts is selected by nsdp_debug_set(6, 4096), and the narrow form's second
    # round starts at 192 rows per compute unit (below, three row tiles win)
    ("nt16-wide", "16 n tiles, 3 row tiles", (256, 256), ("bias", "relu_in"), "linear_bf16x3<3,16,2,4,0>x1", 192, 1, 4096, 192),
    ("nt16-narrow", "16 n tiles, 2 row tiles", (36, 256), ("bias", "res"), "linear_bf16x3<2,16,0,4,0>x1", 128, 1, 0, 192),
    ("mask-nt8", "masked prologue, <= 8 n tiles", (200, 120), ("mask", "omask"), "linear_bf16x3<2,8,1,4,1>x2", 128, 2, 0, 128),
    ("mask-nt13", "masked prologue, 13 n tiles", (256, 200), ("mask", "bias"), "linear_bf16x3<3,13,1,4,0>x1", 192, 1, 0, 192),
    ("mask-nt16", "masked prologue, 16 n tiles", (36, 256), ("mask", "bias", "res", "omask"), "linear_bf16x3<2,16,1,4,0>x1", 128, 1, 0, 128),
]
# 13 n tiles above 2^19 rows: the 8-wave form; 2^19 + 77 is the smallest row count that reaches it (the one case above 200 000 rows)
X3_EIGHT_WAVE = ("nt13-8wave", "13 n tiles, 8 waves", ((1 << 19) + 77, 200, 200), ("bias", "relu_in"), "linear_bf16x3<2,13,2,8,0>x1")
# Epilogues, each at the smallest shape hip_linear routes to the kernel: "min" = hip_linear._X3_MIN_ROWS + 77 rows
X3_EPILOGUES = [
    # id, (M, K, N), flags, traced variant
    ("out-mask", ("min", 36, 40), ("bias", "omask"), "linear_bf16x3<2,4,0,8,0>x1 wres"),
    ("signed-residual", ("min", 36, 120), ("bias", "res-"), "linear_bf16x3<2,8,0,8,0>x1 wres"),
    ("addend-after-mask", ("min", 200, 120), ("mask", "omask", "addend"), "linear_bf16x3<2,8,1,4,1>x2"),
    ("gather", ("min", 36, 40), ("bias", "gather"), "linear_bf16x3<2,4,0,8,0>x1 wres gather"),
    ("gather-one-table", ("min", 36, 200), ("bias", "gather1"), "linear_bf16x3<2,13,0,4,1>x2 gather1"),
]
F32_FORWARD = [
    # (M, K, N), flags
    ((1, 4, 16), ("bias",)),
    ((37, 120, 120), ("bias", "relu_out")),
    ((129, 256, 256), ("bias", "res")),
    ((300, 128, 3), ("bias", "relu_in")),
]
WGRAD = [
    # id, family, (M, N, K), flags, prefix of the traced variant
    ("direct-33", "f32", (33, 40, 24), ("relu_x",), "linear_wgrad_direct<plain>"),
    ("direct-2047", "f32", (2047, 120, 256), ("mask", "relu_x"), "linear_wgrad_direct<mask>"),
    ("f32-rows", "f32", (2500, 120, 200), (), "linear_wgrad<"),
    ("x3-13x13", "x3", (2048, 200, 200), (), "wgrad_bf16x3<13,13,plain,notail>"),
    ("x3-mask-relu", "x3", (4099, 120, 128), ("mask", "relu_x"), "wgrad_bf16x3<8,8,mask,tail>"),
    ("x3-k-split", "x3", (2500, 256, 200), (), "wgrad_bf16x3<16,8,plain,tail>"),
    ("k4-33", "f32", (33, 16, 4), (), "linear_wgrad"),
    ("k4-5000", "f32", (5000, 120, 4), (), "linear_wgrad<k4,plain>"),
    ("bf16-37", "bf16", (37, 120, 120), (), "wgrad_bf16"),
    ("bf16-5131", "bf16", (5131, 200, 200), ("mask",), "wgrad_bf16"),
    ("bf16-4097", "bf16", (4097, 256, 256), ("relu_x",), "wgrad_bf16"),
]
BF16_FORWARD = [(37, 120, 120), (5131, 200, 200), (4097, 256, 256)]          # (M, K, N) of the pair hb.run / hb.wgrad
BF16_FLAGS = ("bias", "res", "relu_out")          # (the fp32-output form of the kernel takes no residual: it runs without)
CPU_ROWS = 96          # rows of a forward case the CPU file emulates (the rows of a dense layer are independent)


def case_seed(name, kind):
    return sum(ord(ch) for ch in name) * 8 + KINDS.index(kind)


def forward_cases():
    """(id, family, storage type, K, N, flags) of every bounded forward case of the GPU file."""
    out = [(c[0], "x3", F32, c[2][0], c[2][1], c[3]) for c in X3_FORWARD]
    out.append((X3_EIGHT_WAVE[0], "x3", F32, X3_EIGHT_WAVE[2][1], X3_EIGHT_WAVE[2][2], X3_EIGHT_WAVE[3]))
    out += [(c[0], "x3", F32, c[1][1], c[1][2], c[2]) for c in X3_EPILOGUES]
    out += [(f"f32-{m}x{k}x{n}", "f32", F32, k, n, fl) for (m, k, n), fl in F32_FORWARD]
    out += [(f"bf16-{m}x{k}x{n}", "bf16", BF, k, n, BF16_FLAGS) for m, k, n in BF16_FORWARD]
    return out
