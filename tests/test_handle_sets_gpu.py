"""The labelled-handle-set kernels (include/nsdp_handle_sets.h) against nsdp_amd.edit.reference_pose_dict's array expressions
evaluated ON THE SAME GPU with torch: separate multiplications and additions in the header's order, free points copied, the rows'
products by 0.0f / 1.0f literal.  Everything is compared as bit patterns (int32 views), NaN payloads and signed zeros included.

The packed entry: rows beyond the total keep their sentinel in every output, each shape's rows carry the bits of the rectangular
entry on that shape alone.  And the rule's drag restated as a handle set (label 1 = the moved region with a translation, label 2
= the other handle points, pinned) gives nsdp_handle_rows' bits."""
import numpy as np
import pytest
import torch

from nsdp_amd import edit, pointnet2_utils as pu
from nsdp_amd.edit import Motion, pack_motions, pack_params, reference_pose_dict

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SENTINEL = 12345.0          # what columns 0:3 and rows nobody owns hold before a call, and must hold after it
FLAG_SENTINEL = 77


def _bits(t):
    return t.contiguous().view(torch.int32)


def _labels(B, n, H, g):
    """(B, n) uint8 in which 0, every label 1..H and -- where H < 255 -- H + 1 and 255 all occur, as far as B * n points can
    hold them (a cloud of fewer points holds the first B * n of: 1, 0, H + 1, 255, 2, 3, ..., H); the rest are drawn from 0..255,
    half of them from 0..H so that handles stay frequent.  Returns the labels and the labels that must occur."""
    need = [1, 0] + ([H + 1, 255] if H < 255 else []) + list(range(2, H + 1))
    need = need[:B * n]
    flat = torch.where(torch.rand(B * n, generator=g) < 0.5, torch.randint(0, H + 1, (B * n,), generator=g),
                       torch.randint(0, 256, (B * n,), generator=g))
    where = torch.randperm(B * n, generator=g)[:len(need)]
    flat[where] = torch.tensor(need)
    return flat.to(torch.uint8).view(B, n), need


def _motions(T, B, H, g):
    """Random affine motions [T, B, H, 12] with an exact identity at handle 1 of pose 0 and a pure translation at the last handle
    of the last pose (both for every shape)."""
    m = (torch.rand(T, B, H, 12, generator=g) - 0.5) * 2.0
    m[0, :, 0] = torch.from_numpy(Motion.identity().matrix().reshape(12))
    if T * H > 1:
        m[T - 1, :, H - 1] = torch.from_numpy(Motion.translate((0.125, -0.3, 0.7)).matrix().reshape(12))
    return m


def _cloud(B, n, g):
    """Coordinates without zeros (0.25 <= |v| < 1.25), so that an identity motion hands the source's bits back."""
    return (torch.rand(B, n, 3, generator=g) + 0.25) * torch.where(torch.rand(B, n, 3, generator=g) < 0.5, -1.0, 1.0)


def _want(src, labels, H, motions=None, targets=None):
    """tgt [T, B, n, 3], columns 3:7 [T, B, n, 4], handle [B, n] uint8 by reference_pose_dict, pose by pose, on the GPU."""
    T = (motions if targets is None else targets).shape[0]
    tgt, cols, handle = [], [], None
    for t in range(T):
        dd = reference_pose_dict(src, None, labels, H, motions=None if motions is None else motions[t],
                                 targets=None if targets is None else targets[t])
        tgt.append(dd["verts_tgt"])
        cols.append(dd["surface_samples_inputs"][:, :, 3:7])
        assert torch.equal(_bits(dd["surface_samples_inputs"][:, :, 0:3]), _bits(src))
        handle = dd["cano_handle_sample_idx"].to(torch.uint8)
    return torch.stack(tgt), torch.stack(cols), handle


def _run(src, labels, motions=None, targets=None, with_tgt=True, with_handle=True):
    B, n = labels.shape
    T = (motions if targets is None else targets).shape[0]
    rows = torch.full((T, B, n, 7), SENTINEL, device=DEV)
    tgt = torch.full((T, B, n, 3), SENTINEL, device=DEV) if with_tgt else None
    ho = torch.full((B, n), FLAG_SENTINEL, dtype=torch.uint8, device=DEV) if with_handle else None
    out = pu.handle_set_rows(src, labels, rows, motions=motions, targets=targets, tgt=tgt, handle_out=ho)
    assert out is rows
    assert bool((rows[..., 0:3] == SENTINEL).all()), "columns 0:3 were written"
    return rows, tgt, ho


@pytest.mark.parametrize("H,T", [(1, 1), (3, 3), (255, 2)])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4097])
def test_rectangular_motions_equal_the_array_expressions(n, B, H, T):
    g = torch.Generator().manual_seed(1000 * n + 10 * B + H)
    labels, need = _labels(B, n, H, g)
    present = set(labels.unique().tolist())
    assert set(need) <= present, sorted(set(need) - present)
    if B * n >= H + 4:      # room for all of them: 0, 1..H and, below 255, H + 1 and 255
        assert {0, *range(1, H + 1)} <= present and (H == 255 or {H + 1, 255} <= present)
    src, labels, motions = _cloud(B, n, g).to(DEV), labels.to(DEV), _motions(T, B, H, g).to(DEV)
    rows, tgt, ho = _run(src, labels, motions=motions)
    want_tgt, want_cols, want_handle = _want(src, labels, H, motions=motions)
    assert torch.equal(ho, want_handle)
    assert torch.equal(_bits(tgt), _bits(want_tgt))
    assert torch.equal(_bits(rows[..., 3:7]), _bits(want_cols))
    # a free point's target is its source row, a point of the identity's handle too -- by their bits
    free = (want_handle == 0)
    assert torch.equal(_bits(tgt[0][free]), _bits(src[free]))
    one = labels == 1
    assert torch.equal(_bits(tgt[0][one]), _bits(src[one])) and bool(one.any())


@pytest.mark.parametrize("n,B,T", [(1, 1, 1), (65, 3, 2), (4097, 1, 3)])
def test_rectangular_targets_equal_the_array_expressions(n, B, T):
    g = torch.Generator().manual_seed(7 * n + B)
    labels, need = _labels(B, n, 3, g)
    assert set(need) <= set(labels.unique().tolist())
    src, labels = _cloud(B, n, g).to(DEV), labels.to(DEV)
    targets = (torch.rand(T, B, n, 3, generator=g) - 0.5).to(DEV)
    rows, tgt, ho = _run(src, labels, targets=targets)
    want_tgt, want_cols, want_handle = _want(src, labels, 0, targets=targets)
    assert torch.equal(ho, (labels != 0).to(torch.uint8)) and torch.equal(ho, want_handle)      # every non-zero label, 255 too
    assert torch.equal(_bits(tgt), _bits(want_tgt)) and torch.equal(_bits(rows[..., 3:7]), _bits(want_cols))
    assert torch.equal(_bits(tgt), _bits(torch.where((labels != 0)[None, :, :, None], targets, src[None])))


def test_nan_inf_and_negative_zero_come_out_as_the_array_expressions():
    g = torch.Generator().manual_seed(5)
    B, n, H, T = 2, 257, 3, 2
    labels, _ = _labels(B, n, H, g)
    src, motions = _cloud(B, n, g), _motions(T, B, H, g)
    targets = torch.rand(T, B, n, 3, generator=g) - 0.5
    special = torch.tensor([float("nan"), float("inf"), float("-inf"), -0.0, 0.0])
    for i in range(30):      # planted under every kind of label: free (0, 4, 255) and handles (1: the identity of pose 0; 2; 3)
        labels[i % B, i] = (0, 1, 2, 3, 4, 255)[i % 6]
        src[i % B, i, i % 3] = special[i % 5]
        targets[i % T, (i + 1) % B, i, (i + 1) % 3] = special[(i + 2) % 5]
    motions[0, 0, 1, 0], motions[0, 0, 1, 7] = float("nan"), float("inf")
    motions[1, 1, 2, 5], motions[1, 1, 2, 3], motions[1, 0, 0, 10] = float("-inf"), -0.0, -0.0
    src, labels, motions, targets = src.to(DEV), labels.to(DEV), motions.to(DEV), targets.to(DEV)
    for kw in (dict(motions=motions), dict(targets=targets)):
        rows, tgt, ho = _run(src, labels, **kw)
        want_tgt, want_cols, want_handle = _want(src, labels, H, **kw)
        assert bool(torch.isnan(want_tgt).any()) and bool(torch.isnan(want_cols).any())
        assert bool((_bits(want_cols[..., 0:3]) == -(1 << 31)).any()), "no -0.0 among the expected columns"
        assert torch.equal(ho, want_handle)
        assert torch.equal(_bits(tgt), _bits(want_tgt)), sorted(kw)
        assert torch.equal(_bits(rows[..., 3:7]), _bits(want_cols)), sorted(kw)


@pytest.mark.parametrize("form", ["motions", "targets"])
@pytest.mark.parametrize("with_tgt,with_handle", [(True, True), (True, False), (False, True), (False, False)])
def test_null_optional_outputs(form, with_tgt, with_handle):
    g = torch.Generator().manual_seed(11)
    B, n, H, T = 2, 300, 3, 2
    labels, _ = _labels(B, n, H, g)
    src, labels = _cloud(B, n, g).to(DEV), labels.to(DEV)
    kw = dict(motions=_motions(T, B, H, g).to(DEV)) if form == "motions" else dict(targets=(torch.rand(T, B, n, 3, generator=g) - 0.5).to(DEV))
    rows, tgt, ho = _run(src, labels, with_tgt=with_tgt, with_handle=with_handle, **kw)
    want_tgt, want_cols, want_handle = _want(src, labels, H, **kw)
    assert torch.equal(_bits(rows[..., 3:7]), _bits(want_cols))
    assert tgt is None or torch.equal(_bits(tgt), _bits(want_tgt))
    assert ho is None or torch.equal(ho, want_handle)


def test_wrapper_refusals():
    from nsdp_amd._lib import NsdpHipError
    src, lab = torch.zeros(2, 8, 3, device=DEV), torch.zeros(2, 8, dtype=torch.uint8, device=DEV)
    rows, mo = torch.zeros(1, 2, 8, 7, device=DEV), torch.zeros(1, 2, 3, 12, device=DEV)
    with pytest.raises(NsdpHipError, match="exactly one of motions and targets .got neither"):
        pu.handle_set_rows(src, lab, rows)
    with pytest.raises(NsdpHipError, match="exactly one of motions and targets .got both"):
        pu.handle_set_rows(src, lab, rows, motions=mo, targets=torch.zeros(1, 2, 8, 3, device=DEV))
    with pytest.raises(NsdpHipError, match=r"motions must be \(T, 2, H, 12\)"):
        pu.handle_set_rows(src, lab, rows, motions=mo[:, :1])
    with pytest.raises(NsdpHipError, match=r"targets must be \(T, 2, 8, 3\)"):
        pu.handle_set_rows(src, lab, rows, targets=torch.zeros(2, 8, 3, device=DEV))
    with pytest.raises(NsdpHipError, match=r"rows \(1,2,8,7\)"):
        pu.handle_set_rows(src, lab, rows[0], motions=mo)
    with pytest.raises(NsdpHipError, match="labels must be a contiguous uint8"):
        pu.handle_set_rows(src, lab.bool(), rows, motions=mo)
    with pytest.raises(NsdpHipError, match="labels must be a contiguous uint8"):
        pu.handle_set_rows(src, lab[:, :7], rows, motions=mo)
    with pytest.raises(NsdpHipError, match="motions must be torch.float32"):
        pu.handle_set_rows(src, lab, rows, motions=mo.double())
    with pytest.raises(NsdpHipError, match="contiguous"):
        pu.handle_set_rows(src, lab, rows, motions=torch.zeros(1, 2, 3, 24, device=DEV)[..., ::2])
    with pytest.raises(NsdpHipError, match="H=256"):
        pu.handle_set_rows(src, lab, rows, motions=torch.zeros(1, 2, 256, 12, device=DEV))
    offs = torch.tensor([0, 8, 16], dtype=torch.int32, device=DEV)
    with pytest.raises(NsdpHipError, match=r"motions must be \(2, H, 12\)"):
        pu.handle_set_rows_ragged(src.view(16, 3), offs, lab.view(16), rows.view(16, 7), motions=mo)
    with pytest.raises(NsdpHipError, match="got neither"):
        pu.handle_set_rows_ragged(src.view(16, 3), offs, lab.view(16), rows.view(16, 7))
    with pytest.raises(NsdpHipError, match=r"targets must be packed \(16, 3\)"):
        pu.handle_set_rows_ragged(src.view(16, 3), offs, lab.view(16), rows.view(16, 7), targets=torch.zeros(15, 3, device=DEV))


# ---------------------------------------------------------------------------------------------------- the packed entry
COUNTS = (3001, 0, 1, 255, 256, 257)
PAD = 41


@pytest.mark.parametrize("form", ["motions", "targets"])
def test_packed_rows_equal_the_rectangular_entry_shape_by_shape(form):
    g = torch.Generator().manual_seed(23)
    B, total, H = len(COUNTS), sum(COUNTS), 3
    cap = total + PAD
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(COUNTS)]), dtype=torch.int32, device=DEV)
    labels, _ = _labels(1, cap, H, g)
    src, labels = _cloud(1, cap, g)[0].to(DEV), labels[0].to(DEV)
    motions = _motions(1, B, H, g)[0].to(DEV)
    targets = (torch.rand(cap, 3, generator=g) - 0.5).to(DEV)
    kw = dict(motions=motions) if form == "motions" else dict(targets=targets)
    rows, tgt = torch.full((cap, 7), SENTINEL, device=DEV), torch.full((cap, 3), SENTINEL, device=DEV)
    ho = torch.full((cap,), FLAG_SENTINEL, dtype=torch.uint8, device=DEV)
    pu.handle_set_rows_ragged(src, offsets, labels, rows, tgt=tgt, handle_out=ho, **kw)
    assert bool((rows[:, 0:3] == SENTINEL).all()), "columns 0:3 were written"
    assert bool((rows[total:] == SENTINEL).all()) and bool((tgt[total:] == SENTINEL).all()) and bool((ho[total:] == FLAG_SENTINEL).all())
    lo = 0
    for b, nb in enumerate(COUNTS):
        if nb:
            one = dict(motions=motions[None, b:b + 1]) if form == "motions" else dict(targets=targets[None, None, lo:lo + nb])
            r1, t1, h1 = _run(src[None, lo:lo + nb].contiguous(), labels[None, lo:lo + nb].contiguous(), **one)
            assert torch.equal(_bits(rows[lo:lo + nb, 3:7]), _bits(r1[0, 0, :, 3:7])), b
            assert torch.equal(_bits(tgt[lo:lo + nb]), _bits(t1[0, 0])) and torch.equal(ho[lo:lo + nb], h1[0]), b
        lo += nb
    # the optional outputs may be null, and offsets that overrun the capacity are clamped: nothing behind cap - 1 exists to touch
    rows2 = torch.full((cap, 7), SENTINEL, device=DEV)
    pu.handle_set_rows_ragged(src, offsets, labels, rows2, **kw)
    assert torch.equal(_bits(rows2), _bits(rows))
    wild = offsets.clone()
    wild[-1] = cap + 100000
    rows3 = torch.full((cap, 7), SENTINEL, device=DEV)
    pu.handle_set_rows_ragged(src, wild, labels, rows3, **kw)
    assert torch.equal(_bits(rows3[:total]), _bits(rows[:total])) and bool((rows3[:, 0:3] == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------- the rule, restated
def test_a_rule_drag_restated_as_a_handle_set_gives_the_rule_kernels_bits():
    """Labels from the rule's move_out / handle_out (1 = moved, 2 = the other handle points), motions (translate d, identity):
    tgt, rows[..., 3:7] and handle_out equal nsdp_handle_rows' bits for the same drag.

    The coordinates hold no zeros.  The two spellings agree on every other finite value -- 1 * x is x, 0 * y is a zero of some
    sign and x + (that zero) is x; (x + 0) + d rounds as x + d * 1 does -- but not on a zero: 1 * (-0) + 0 * y is +0 where the
    rule's (-0) + d * 0 may be -0."""
    g = torch.Generator().manual_seed(31)
    B, n = 2, 4097
    src = _cloud(B, n, g)
    src = (src * 0.4).to(DEV)                                  # within the unit box, still without zeros
    assert bool((src != 0).all())
    d = [(-0.15, -0.2, 0.2), (0.1, 0.05, -0.3)]
    params = torch.from_numpy(pack_params(B, ["head", "frontleftfoot"], d, 0.1, False)).to(DEV)
    bounds = pu.handle_bounds(src)
    rule_rows, rule_tgt = torch.full((B, n, 7), SENTINEL, device=DEV), torch.empty(B, n, 3, device=DEV)
    rule_h, rule_m = torch.empty(B, n, dtype=torch.uint8, device=DEV), torch.empty(B, n, dtype=torch.uint8, device=DEV)
    pu.handle_rows(src, src, bounds, params, rule_rows, tgt=rule_tgt, handle_out=rule_h, move_out=rule_m)
    for b in range(B):
        assert 0 < int(rule_m[b].sum()) < int(rule_h[b].sum()) < n, b
    labels = torch.where(rule_m != 0, torch.full_like(rule_h, 1), rule_h * 2)
    motions = torch.from_numpy(pack_motions(B, 2, [[Motion.translate(np.float32(d[b])), Motion.identity()] for b in range(B)])).to(DEV)
    rows, tgt, ho = _run(src, labels, motions=motions[None])
    assert torch.equal(ho, rule_h)
    assert torch.equal(_bits(tgt[0]), _bits(rule_tgt))
    assert torch.equal(_bits(rows[0, :, :, 3:7]), _bits(rule_rows[:, :, 3:7]))
