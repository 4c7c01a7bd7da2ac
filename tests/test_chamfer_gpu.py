"""The Chamfer training loss on the GPU (nsdp_amd/chamfer.py, include/nsdp_chamfer.h) against the fp64 yardstick of
tests/chamfer_ref.py.

Bounds are derived, not measured:
  * loss: |L - L64| <= 16 * 2^-24 * L64 -- five roundings go into ((dx^2 + dy^2) + dz^2) of rounded differences, the double
    reduction adds one rounding to fp32, the scales add two; 16 leaves a factor 2 over that;
  * gradient, per element: |grad - exact| <= c * 2^-24 * sum |terms| with c = 6 + depth(T), T the length of the row's list:
    5 + depth first-order roundings from the operation order documented in the header (chamfer_ref.envelope_c spells them out),
    one unit for second-order terms and the yardstick.  "exact" is the closed form in fp64 on the kernel's OWN indices, which
    are first held to be minimisers in fp64 up to the rounding of an fp32 distance."""
import pytest
import torch

import chamfer_ref
from chamfer_ref import U

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

SIZES = [(1, 63), (63, 1), (64, 65), (65, 255), (257, 64), (255, 1000), (1000, 257), (1000, 63)]


def _clouds(B, n, m, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, n, 3, generator=g), torch.randn(B, m, 3, generator=g)


def _run(P, Q, w_pt=1.0, w_tp=1.0, target_grad=True, scale=None):
    """chamfer_loss forward + backward on the GPU -> dict of CPU tensors."""
    from nsdp_amd import chamfer
    p = P.to(DEV).requires_grad_(True)
    q = Q.to(DEV).requires_grad_(target_grad)
    loss, terms = chamfer.chamfer_loss(p, q, w_pt, w_tp, return_per_shape=True)
    (loss if scale is None else loss * scale).backward()
    torch.cuda.synchronize()
    return {"loss": loss.detach().cpu(), "terms": terms.cpu(), "dP": p.grad.cpu(), "dQ": None if q.grad is None else q.grad.cpu()}


def _indices(P, Q):
    from nsdp_amd import chamfer
    out = chamfer.forward_raw(P.to(DEV), Q.to(DEV))
    torch.cuda.synchronize()
    return [t.cpu() for t in out]


def _check_gradients(P, Q, got, idx_pt, idx_tp, w_pt=1.0, w_tp=1.0, g=1.0):
    chamfer_ref.assert_minimisers(P, Q, idx_pt, idx_tp)
    want = chamfer_ref.closed_form(P, Q, idx_pt, idx_tp, w_pt, w_tp, g)
    for name in ("dP", "dQ"):
        if got[name] is None:
            continue
        grad, mass, lengths = want[name]
        c = chamfer_ref.envelope_c(lengths)[:, :, None]
        err = (got[name].double() - grad).abs()
        bound = c * U * mass
        worst = float((err / bound.clamp_min(1e-300)).max())
        print(f"{name}: worst error / bound {worst:.3f}, longest list {int(lengths.max())}")
        assert bool((err <= bound).all()), (name, worst)
        assert bool((got[name][mass == 0] == 0).all()), name                 # zero rows are exactly zero


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n,m", SIZES)
def test_forward_and_backward_against_fp64(B, n, m):
    from nsdp_amd import pointnet2_utils
    P, Q = _clouds(B, n, m, 1000 * n + m + B)
    loss, terms, d_pt, i_pt, d_tp, i_tp = _indices(P, Q)
    # indices and distances: nn_dist2's, bit for bit, in both directions
    for query, source, d, i in ((P, Q, d_pt, i_pt), (Q, P, d_tp, i_tp)):
        d_want, i_want = pointnet2_utils.nn_dist2(query.to(DEV), source.to(DEV), True)
        assert torch.equal(d, d_want.cpu()) and torch.equal(i, i_want.cpu())
    got = _run(P, Q)
    assert torch.equal(got["loss"].reshape(1), loss) and torch.equal(got["terms"], terms)
    L64, terms64 = chamfer_ref.loss64(P, Q)
    print(f"loss {float(got['loss'])!r} vs {float(L64)!r}: error / bound {abs(float(got['loss']) - float(L64)) / (16 * U * float(L64)):.3f}")
    assert abs(float(got["loss"]) - float(L64)) <= 16 * U * float(L64)
    assert bool(((got["terms"].double() - terms64).abs() <= 16 * U * terms64).all())
    _check_gradients(P, Q, got, i_pt, i_tp)


@pytest.mark.parametrize("w_pt,w_tp", [(0.5, 2.0), (1.0, 0.0), (0.0, 1.0)])
def test_weights(w_pt, w_tp):
    P, Q = _clouds(3, 257, 65, 77)
    _, _, _, i_pt, _, i_tp = _indices(P, Q)
    got = _run(P, Q, w_pt, w_tp)
    L64, _ = chamfer_ref.loss64(P, Q, w_pt, w_tp)
    assert abs(float(got["loss"]) - float(L64)) <= 16 * U * float(L64)
    _check_gradients(P, Q, got, i_pt, i_tp, w_pt, w_tp)


def test_ties_go_to_the_smallest_index_on_a_lattice_and_among_duplicates():
    from nsdp_amd import pointnet2_utils
    axis = torch.arange(6.0)
    lattice = torch.stack(torch.meshgrid(axis, axis, axis, indexing="ij"), -1).reshape(1, 216, 3)
    centres = torch.stack(torch.meshgrid(axis[:5], axis[:5], axis[:5], indexing="ij"), -1).reshape(1, 125, 3) + 0.5
    g = torch.Generator().manual_seed(3)
    cloud = torch.randn(1, 40, 3, generator=g)
    dup = torch.cat([cloud, cloud[:, 5:25], cloud[:, :10]], dim=1)          # every row of 0 .. 24 appears twice
    for P, Q in ((centres, lattice), (lattice, centres), (cloud, dup), (dup, cloud)):
        loss, terms, d_pt, i_pt, d_tp, i_tp = _indices(P, Q)
        d64 = chamfer_ref.dist2_64(P, Q)
        ties = 0
        for d, i, dim in ((d_pt, i_pt, 2), (d_tp, i_tp, 1)):
            exact = d64.min(dim=dim).values
            assert torch.equal(d.double(), exact)                             # (half-integers and copies: the fp32 distance is exact)
            hits = d64 == exact.unsqueeze(dim)
            first = hits.int().argmax(dim=dim)                                # the smallest index among the minimisers
            assert torch.equal(i.long(), first)
            ties = max(ties, int(hits.sum(dim=dim).max()))
        assert ties >= 2                                                      # (there are ties in one direction at least)
        for query, source, d, i in ((P, Q, d_pt, i_pt), (Q, P, d_tp, i_tp)):
            d_want, i_want = pointnet2_utils.nn_dist2(query.to(DEV), source.to(DEV), True)
            assert torch.equal(d, d_want.cpu()) and torch.equal(i, i_want.cpu())
        _check_gradients(P, Q, _run(P, Q), i_pt, i_tp)


def test_equal_sets_give_exactly_zero():
    P, _ = _clouds(3, 257, 1, 11)
    got = _run(P, P.clone())
    assert float(got["loss"]) == 0.0 and bool((got["terms"] == 0).all())
    assert bool((got["dP"] == 0).all()) and bool((got["dQ"] == 0).all())


def test_zero_rows_with_empty_lists_are_exactly_zero():
    """Predictions 0 .. 36 ARE targets 0 .. 36, predictions 63 .. 99 are further copies of them: every copy's nearest target is
    at distance 0 and no target lists a later copy (the smallest index wins the tie), so rows 63 .. 99 have an empty list and a
    zero difference -- exactly zero, beside rows 37 .. 62 that are not."""
    P, Q = _clouds(2, 100, 63, 21)
    P[:, :37] = Q[:, :37]
    P[:, 37:63] = Q[:, 37:] + 0.01 * P[:, 37:63]
    P[:, 63:] = Q[:, :37]
    _, _, _, i_pt, _, i_tp = _indices(P, Q)
    assert bool((chamfer_ref.closed_form(P, Q, i_pt, i_tp)["dP"][2][:, 63:] == 0).all())
    got = _run(P, Q)
    assert bool((got["dP"][:, 63:] == 0).all()) and bool((got["dP"][:, :37] == 0).all()) and bool((got["dP"][:, 37:63] != 0).any())
    _check_gradients(P, Q, got, i_pt, i_tp)


def _designed_lists(lengths, seed, B=2):
    """Predictions far apart (10 units), every target within 1 unit of the prediction it is assigned to: the list of prediction
    i has exactly lengths[i] entries, scattered over the target rows."""
    g = torch.Generator().manual_seed(seed)
    n, m = len(lengths), int(sum(lengths))
    P = torch.zeros(B, n, 3)
    P[:, :, 0] = 10.0 * torch.arange(n)
    P[:, :, 1:] = torch.randn(B, n, 2, generator=g)
    owner = torch.repeat_interleave(torch.arange(n), torch.tensor(lengths))
    owners = torch.stack([owner[torch.randperm(m, generator=g)] for _ in range(B)])
    Q = torch.gather(P, 1, owners[:, :, None].expand(B, m, 3)) + (torch.rand(B, m, 3, generator=g) - 0.5)
    return P.contiguous(), Q.contiguous(), owners


@pytest.mark.parametrize("lengths", [[0, 1, 31, 32, 33, 0, 2, 1023, 1024, 1025, 5, 0, 64, 65, 1100, 3],
                                     [0] * 290 + [1030] + [1] * 6 + [40, 33, 1026]], ids=["switches", "second_workgroup"])
def test_lists_of_every_form_and_at_every_switch(lengths):
    """Empty lists, one entry, and the lengths around the lane / wave (32) and wave / workgroup (1024) switches, in one launch:
    several workgroup-form rows in a workgroup and rows of every form in one wave; then the same forms in a workgroup that is
    not the first of its shape.  Beyond the envelope, the order of additions is held to the bit: both gradients equal the fp32
    rebuild of the documented order (chamfer_ref.ordered) on the kernel's own indices."""
    P, Q, owners = _designed_lists(lengths, 5)
    _, _, _, i_pt, _, i_tp = _indices(P, Q)
    assert torch.equal(i_tp.long(), owners)
    for lo, hi in ((0, chamfer_ref.LANE_MAX), (chamfer_ref.LANE_MAX + 1, chamfer_ref.WAVE_MAX), (chamfer_ref.WAVE_MAX + 1, 10 ** 9)):
        assert any(lo <= t <= hi for t in lengths)
    first = _run(P, Q)
    assert torch.equal(chamfer_ref.closed_form(P, Q, i_pt, i_tp)["dP"][2][0], torch.tensor(lengths))
    _check_gradients(P, Q, first, i_pt, i_tp)
    want = chamfer_ref.ordered(P, Q, i_pt, i_tp)
    for name in ("dP", "dQ"):
        print(f"{name}: {int((first[name] != want[name]).sum())} elements differ from the documented order's bits")
        assert torch.equal(first[name], want[name]), name
    again = _run(P, Q)
    for key in first:
        assert torch.equal(first[key], again[key]), key


def test_collapsed_predictions_one_list_of_8200_entries():
    """All predictions equal (early training): every target's nearest prediction is row 0, one list holds all 8200 targets and the
    workgroup form sums it; two runs give the same bits."""
    _, Q = _clouds(2, 1, 8200, 31)
    P = torch.full((2, 300, 3), 0.25)
    _, _, _, i_pt, _, i_tp = _indices(P, Q)
    assert bool((i_tp == 0).all())
    first = _run(P, Q)
    _check_gradients(P, Q, first, i_pt, i_tp)
    again = _run(P, Q)
    for key in first:
        assert torch.equal(first[key], again[key]), key


def test_reproducible_bits():
    P, Q = _clouds(3, 1000, 257, 41)
    first, again = _run(P, Q), _run(P, Q)
    for key in first:
        assert torch.equal(first[key], again[key]), key


def test_list_builds_give_the_same_bits():
    """n = 8193 predictions (one more than the one-workgroup list build serves), m = 300, under NSDP_INVERT_WIDE at its default,
    "force" and "0": the modes that accept the size give the same bits, "0" refuses it by name.  A small case takes both builds
    (the one-workgroup entry under "1", the many-workgroup entry under "force") to the same bits as well."""
    from nsdp_amd import _lib, hip_attention as ha
    P, Q = _clouds(1, 8193, 300, 51)
    base = _run(P, Q, target_grad=False)
    _, _, _, i_pt, _, i_tp = _indices(P, Q)
    _check_gradients(P, Q, base, i_pt, i_tp)
    for mode in ("1", "force"):
        with ha.invert_wide_mode(mode):
            got = _run(P, Q, target_grad=False)
        assert torch.equal(got["dP"], base["dP"]) and torch.equal(got["loss"], base["loss"]), mode
    with ha.invert_wide_mode("0"), pytest.raises(_lib.NsdpHipError, match="NSDP_INVERT_WIDE=0"):
        _run(P, Q, target_grad=False)
    P, Q = _clouds(2, 300, 257, 52)
    with ha.invert_wide_mode("1"):
        assert not ha._use_wide(2, 257, 300)
        narrow = _run(P, Q)
    with ha.invert_wide_mode("force"):
        assert ha._use_wide(2, 257, 300)
        wide = _run(P, Q)
    with ha.invert_wide_mode("0"):
        old = _run(P, Q)
    for key in narrow:
        assert torch.equal(narrow[key], wide[key]) and torch.equal(narrow[key], old[key]), key


def test_target_gradient_only_when_asked_for(monkeypatch):
    from nsdp_amd import chamfer
    calls = []
    real = chamfer.backward_operand
    monkeypatch.setattr(chamfer, "backward_operand", lambda *a: calls.append(tuple(a[0].shape)) or real(*a))
    P, Q = _clouds(2, 65, 255, 61)
    got = _run(P, Q, target_grad=False)
    assert got["dQ"] is None and calls == [(2, 65, 3)]
    both = _run(P, Q, target_grad=True)
    assert calls[1:] == [(2, 65, 3), (2, 255, 3)] and torch.equal(both["dP"], got["dP"])
    _, _, _, i_pt, _, i_tp = _indices(P, Q)
    _check_gradients(P, Q, both, i_pt, i_tp)


def test_upstream_gradient_is_read_from_the_device():
    """A loss scaled by a power of two scales the gradient exactly; the scale reaches the kernel as a device tensor."""
    P, Q = _clouds(2, 255, 64, 71)
    base = _run(P, Q)
    for scale in (4.0, 0.125, -2.0):
        got = _run(P, Q, scale=scale)
        assert torch.equal(got["dP"], base["dP"] * scale) and torch.equal(got["dQ"], base["dQ"] * scale), scale
    _, _, _, i_pt, _, i_tp = _indices(P, Q)
    _check_gradients(P, Q, _run(P, Q, scale=3.0), i_pt, i_tp, g=3.0)
