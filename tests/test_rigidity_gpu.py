"""The local-rigidity training regulariser on the GPU (nsdp_amd/rigidity.py, include/nsdp_rigidity.h) against the fp64 yardstick
of tests/rigidity_ref.py, per element and in two steps, so that no case is ever left out:

  1. the residuals against fp64: |resid - r64| <= RESID_C * 2^-24 * (cur + rest) -- the bound scales with the two squared
     lengths, not with |r|, because r cancels;
  2. terms, loss and the gradient against the closed form evaluated in fp64 ON THE KERNEL'S OWN RESIDUALS:
     terms / loss within TERMS_C * 2^-24 of their value, the gradient per element within
     (GRAD_C0 + max(K - 1, depth(T))) * 2^-24 * sum |terms|, T the row's in-degree.

The constants are derived from the operation order documented in the header (rigidity_ref spells them out), not measured."""
import pytest
import torch

import rigidity_ref
from rigidity_ref import RESID_C, TERMS_C, U

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

DEGREES = [0, 1, 31, 32, 33, 0, 2, 1023, 1024, 1025, 5, 0, 64, 65, 1100, 3]


def _operands(B, n, K, seed, noise=0.3):
    g = torch.Generator().manual_seed(seed)
    S = torch.randn(B, n, 3, generator=g)
    P = S + noise * torch.randn(B, n, 3, generator=g)
    idx = torch.randint(0, n, (B, n, K), generator=g, dtype=torch.int64).int()
    return P, S, idx


def _run(P, S, idx, weight=1.0, scale=None):
    """local_rigidity_loss forward + backward on the GPU, and the residuals of forward_raw -> dict of CPU tensors."""
    from nsdp_amd import rigidity
    p, s, i = P.to(DEV).requires_grad_(True), S.to(DEV), idx.to(DEV)
    loss, terms = rigidity.local_rigidity_loss(p, s, weight=weight, idx=i, return_per_shape=True)
    (loss if scale is None else loss * scale).backward()
    raw = rigidity.forward_raw(p.detach(), s, i, weight)
    torch.cuda.synchronize()
    assert torch.equal(raw[0].reshape(()), loss.detach()) and torch.equal(raw[1], terms)
    return {"loss": loss.detach().cpu(), "terms": terms.cpu(), "dP": p.grad.cpu(), "resid": raw[2].cpu()}


def _check(P, S, idx, got, weight=1.0, g=1.0):
    K = idx.shape[2]
    # step 1: the residuals
    r64, cur, rest = rigidity_ref.resid64(P, S, idx)
    err, bound = (got["resid"].double() - r64).abs(), RESID_C * U * (cur + rest)
    print(f"resid: worst error / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all())
    # step 2: everything else, on the kernel's own residuals
    loss, terms = rigidity_ref.from_resid(got["resid"], weight)
    print(f"loss {float(got['loss'])!r} vs {float(loss)!r}")
    assert abs(float(got["loss"]) - float(loss)) <= TERMS_C * U * abs(float(loss))
    assert bool(((got["terms"].double() - terms).abs() <= TERMS_C * U * terms).all())
    grad, mass, lengths = rigidity_ref.closed_form(P, idx, got["resid"], weight, g)
    c = rigidity_ref.envelope_c(lengths, K)[:, :, None]
    err, bound = (got["dP"].double() - grad).abs(), c * U * mass
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"dP: worst error / bound {worst:.3f}, largest in-degree {int(lengths.max())}")
    assert bool((err <= bound).all()), worst
    assert bool((got["dP"][mass == 0] == 0).all())                         # zero rows are exactly zero
    return lengths


@pytest.mark.parametrize("K", [1, 7, 8, 32])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257])
@pytest.mark.parametrize("B", [1, 3])
def test_forward_and_backward_against_fp64(B, n, K):
    """Random indices in [0, n): any index tensor is a valid operand (n = 1: every entry names its own row)."""
    P, S, idx = _operands(B, n, K, 1000 * n + 10 * K + B)
    got = _run(P, S, idx)
    _check(P, S, idx, got)
    if n == 1:
        assert float(got["loss"]) == 0.0 and bool((got["dP"] == 0).all())


def test_more_rows_than_64_slices_of_256():
    """n = 16 641 rows: the per-shape term is summed by 64 slices of 261 rows (up to 16 384 rows a slice is 256 rows or fewer and
    a thread holds at most one), the last slice short."""
    P, S, idx = _operands(2, 16641, 2, 23)
    _check(P, S, idx, _run(P, S, idx))


def _designed_indices(degrees, K, seed, B=2):
    """idx [B, n, K] with n * K = sum(degrees) whose row i < len(degrees) is named exactly degrees[i] times (rows beyond: never),
    the names scattered over the positions."""
    g = torch.Generator().manual_seed(seed)
    E = int(sum(degrees))
    assert E % K == 0
    names = torch.repeat_interleave(torch.arange(len(degrees)), torch.tensor(degrees))
    idx = torch.stack([names[torch.randperm(E, generator=g)] for _ in range(B)]).reshape(B, E // K, K).int()
    return idx.contiguous()


@pytest.mark.parametrize("K", [1, 4])
def test_lists_of_every_form_and_at_every_switch(K):
    """Empty lists, one entry, and the in-degrees around the lane / wave (32) and wave / workgroup (1024) switches, in one
    launch: rows of every form in one wave, several workgroup-form rows in a workgroup.  K = 4 exercises e div K.  Two runs give
    the same bits.  Beyond the envelope, the order of additions is held to the bit: the gradient equals the fp32 rebuild of the
    documented order (rigidity_ref.ordered) on the kernel's own residuals."""
    idx = _designed_indices(DEGREES, K, 5 + K)
    B, n = idx.shape[0], idx.shape[1]
    assert n == sum(DEGREES) // K
    P, S, _ = _operands(B, n, 1, 17 + K)
    first = _run(P, S, idx)
    lengths = _check(P, S, idx, first)
    assert lengths[0, :16].tolist() == DEGREES and int(lengths[:, 16:].sum()) == 0
    want = rigidity_ref.ordered(P, idx, first["resid"])
    print(f"dP: {int((first['dP'] != want).sum())} elements differ from the documented order's bits")
    assert torch.equal(first["dP"], want)
    for lo, hi in ((0, rigidity_ref.LANE_MAX), (rigidity_ref.LANE_MAX + 1, rigidity_ref.WAVE_MAX), (rigidity_ref.WAVE_MAX + 1, 10 ** 9)):
        assert any(lo <= t <= hi for t in DEGREES)
    again = _run(P, S, idx)
    for key in first:
        assert torch.equal(first[key], again[key]), key


def test_one_hub_of_8200_entries():
    """Everything names row 0 (n = 2050, K = 4): one list of 8200 entries, the workgroup form; row 0 names itself four times."""
    P, S, _ = _operands(2, 2050, 1, 31)
    idx = torch.zeros(2, 2050, 4, dtype=torch.int32)
    first = _run(P, S, idx)
    lengths = _check(P, S, idx, first)
    assert int(lengths[0, 0]) == 8200 and bool((first["resid"][:, 0] == 0).all())
    again = _run(P, S, idx)
    for key in first:
        assert torch.equal(first[key], again[key]), key


def test_duplicate_hubs_through_neighbour_sets():
    """300 copies of one point and 200 random points: the lowest-index copies are every copy's nearest, so real data reaches
    the wave form; a copy that finds itself among its neighbours contributes exactly 0 there."""
    from nsdp_amd import rigidity
    g = torch.Generator().manual_seed(41)
    S = torch.randn(2, 500, 3, generator=g)
    S[:, :300] = S[:, :1]
    P = S + 0.2 * torch.randn(2, 500, 3, generator=g)
    idx = rigidity.neighbour_sets(S.to(DEV), 8).cpu()
    assert idx.dtype is torch.int32 and tuple(idx.shape) == (2, 500, 8)
    full = torch.cdist(S.double(), S.double())
    kth = torch.gather(full, 2, idx.long()).max(dim=2).values
    assert bool(((full <= kth[:, :, None]).sum(dim=2) >= 9).all())          # (the k nearest others: itself and 8 more lie within)
    own = torch.arange(500)[None, :, None]
    assert bool((idx[:, 9:300] != own[:, 9:300]).all()) and bool((idx[:, 300:] != own[:, 300:]).all())
    assert bool((idx[:, 1:9] == own[:, 1:9]).any(dim=2).all())              # copies 1 .. 8 find themselves in a later column
    got = _run(P, S, idx)
    lengths = _check(P, S, idx, got)
    assert rigidity_ref.LANE_MAX < int(lengths.max()) <= rigidity_ref.WAVE_MAX and int(lengths.max()) >= 290
    assert bool((got["resid"][idx == own] == 0).all())


def test_equal_clouds_give_exactly_zero():
    P, S, idx = _operands(3, 257, 8, 11)
    got = _run(S.clone(), S, idx)
    assert float(got["loss"]) == 0.0 and bool((got["terms"] == 0).all())
    assert bool((got["resid"] == 0).all()) and bool((got["dP"] == 0).all())


def test_self_entries_contribute_exactly_zero():
    P, S, idx = _operands(2, 130, 4, 13)
    own = torch.arange(130, dtype=torch.int32)[None, :, None].expand(2, 130, 4).contiguous()
    got = _run(P, S, own)
    assert float(got["loss"]) == 0.0 and bool((got["resid"] == 0).all()) and bool((got["dP"] == 0).all())
    mixed = idx.clone()
    mixed[:, :, 1] = own[:, :, 1]
    got, plain = _run(P, S, mixed), _run(P, S, idx)
    _check(P, S, mixed, got)
    assert bool((got["resid"][:, :, 1] == 0).all())
    for col in (0, 2, 3):
        assert torch.equal(got["resid"][:, :, col], plain["resid"][:, :, col])


def test_rigid_motions_give_zero_to_the_envelope():
    """An isometry of the source: a signed permutation of the axes and a translation, exact in fp32 on coordinates that are
    multiples of 2^-10 (every residual's exact value is 0, so |resid| itself is held to the envelope), and a general rotation
    rounded to fp32 (the exact residual of the rounded rows is not 0: the envelope around it)."""
    g = torch.Generator().manual_seed(19)
    S = torch.randint(-4096, 4096, (2, 257, 3), generator=g).float() / 1024.0
    idx = torch.randint(0, 257, (2, 257, 8), generator=g, dtype=torch.int64).int()
    R = torch.tensor([[0.0, -1.0, 0.0], [0.0, 0.0, 1.0], [-1.0, 0.0, 0.0]])
    assert abs(float(torch.linalg.det(R)) - 1.0) < 1e-6                      # (a rotation, not a reflection)
    P = S @ R.T + torch.tensor([0.5, -2.0, 1.0])
    assert torch.equal(P.double(), S.double() @ R.double().T + torch.tensor([0.5, -2.0, 1.0], dtype=torch.float64))
    r64, cur, rest = rigidity_ref.resid64(P, S, idx)
    assert bool((r64 == 0).all())
    got = _run(P, S, idx)
    assert bool((got["resid"].double().abs() <= RESID_C * U * (cur + rest)).all())
    _check(P, S, idx, got)
    q, _ = torch.linalg.qr(torch.randn(3, 3, dtype=torch.float64, generator=g))
    P = (S.double() @ q.T + torch.tensor([0.3, 0.7, -1.1], dtype=torch.float64)).float()
    r64, cur, rest = rigidity_ref.resid64(P, S, idx)
    got = _run(P, S, idx)
    assert bool((got["resid"].double().abs() <= RESID_C * U * (cur + rest) + r64.abs()).all())
    _check(P, S, idx, got)


def test_reproducible_bits():
    P, S, idx = _operands(3, 1000, 8, 43)
    first, again = _run(P, S, idx), _run(P, S, idx)
    for key in first:
        assert torch.equal(first[key], again[key]), key


def test_list_builds_give_the_same_bits():
    """n * K = 800 entries: the one-workgroup build (NSDP_INVERT_WIDE "1" and "0") and the many-workgroup build ("force") give
    the same bits.  Beyond 1024 entries the many-workgroup build is taken in every mode that has it; "0" refuses by name."""
    from nsdp_amd import _lib, hip_attention as ha
    P, S, idx = _operands(2, 100, 8, 51)
    with ha.invert_wide_mode("1"):
        assert not ha._use_wide(2, 800, 100)
        narrow = _run(P, S, idx)
    with ha.invert_wide_mode("force"):
        assert ha._use_wide(2, 800, 100)
        wide = _run(P, S, idx)
    with ha.invert_wide_mode("0"):
        old = _run(P, S, idx)
    for key in narrow:
        assert torch.equal(narrow[key], wide[key]) and torch.equal(narrow[key], old[key]), key
    _check(P, S, idx, narrow)
    P, S, idx = _operands(1, 257, 8, 52)
    base = _run(P, S, idx)
    with ha.invert_wide_mode("force"):
        assert torch.equal(_run(P, S, idx)["dP"], base["dP"])
    with ha.invert_wide_mode("0"), pytest.raises(_lib.NsdpHipError, match="local_rigidity_loss backward: NSDP_INVERT_WIDE=0"):
        _run(P, S, idx)


def test_upstream_gradient_is_read_from_the_device():
    """A loss scaled by a power of two scales the gradient exactly; the scale reaches the kernel as a device tensor."""
    P, S, idx = _operands(2, 255, 7, 71)
    base = _run(P, S, idx)
    for scale in (4.0, 0.125, -2.0):
        assert torch.equal(_run(P, S, idx, scale=scale)["dP"], base["dP"] * scale), scale
    _check(P, S, idx, _run(P, S, idx, scale=3.0), g=3.0)


def test_weight_scales_the_result():
    P, S, idx = _operands(3, 65, 8, 81)
    base = _run(P, S, idx)
    for w in (4.0, 0.125, -2.0):                                            # a power of two: exactly
        got = _run(P, S, idx, weight=w)
        assert torch.equal(got["loss"], base["loss"] * w) and torch.equal(got["dP"], base["dP"] * w), w
        assert torch.equal(got["terms"], base["terms"]) and torch.equal(got["resid"], base["resid"])      # (the terms carry no weight)
    _check(P, S, idx, _run(P, S, idx, weight=0.3), weight=0.3)


def test_a_term_is_a_function_of_its_own_shape_alone():
    P, S, idx = _operands(3, 257, 8, 91)
    together = _run(P, S, idx)
    for b in range(3):
        alone = _run(P[b:b + 1], S[b:b + 1], idx[b:b + 1])
        assert torch.equal(alone["terms"], together["terms"][b:b + 1]) and torch.equal(alone["resid"], together["resid"][b:b + 1])


def test_no_gradient_flows_to_the_source_or_the_indices():
    from nsdp_amd import rigidity
    P, S, idx = _operands(2, 65, 8, 95)
    p, s = P.to(DEV).requires_grad_(True), S.to(DEV).requires_grad_(True)
    rigidity.local_rigidity_loss(p, s, idx=idx.to(DEV)).backward()
    assert s.grad is None and p.grad is not None
    searched = rigidity.local_rigidity_loss(p, s, k=8)                      # (and the default path searches the source itself)
    assert torch.equal(searched.detach(), rigidity.local_rigidity_loss(p.detach(), s.detach(), idx=rigidity.neighbour_sets(s, 8)))
