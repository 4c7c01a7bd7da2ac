"""The user-handle kernels (include/nsdp_handles.h) against the rule written out in explicit-float32 numpy: every comparison is
exact equality of bits.  B = 3 with n in {1, 63, 64, 65, 257, 1025}; all six parts, cliptail on and off, another part and
translation per shape; points exactly ON each threshold (the comparisons are strict); -0.0 coordinates and negative coordinates
under a zero mask (the sign of zero); an empty region and an all-points region; explicit masks; columns 0:3 and the rows behind
the B shapes of a larger buffer untouched; and the bounds equal to min / max bit for bit, n = 1 and a shape whose extreme is its
last point included."""
import numpy as np
import pytest
import torch

from nsdp_amd import pointnet2_utils as pu
from nsdp_amd.edit import PARTS, pack_params

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F = np.float32
SIZES = (1, 63, 64, 65, 257, 1025)
SENTINEL = F(-7.25)


def bits(a):
    """The bit patterns, every NaN as one pattern: which NaN an invalid operation (inf * 0) makes differs between the host's and
    the GPU's arithmetic -- test_signed_zeros_and_nans... holds the NaN bits against the GPU's own array expressions."""
    a = np.ascontiguousarray(a, dtype=F)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


def rule(cano, src, lo, hi, part, cliptail, r, d):
    """dataset/utils.py: cano_handle_user_define for ONE shape, fp32 with one rounding per operation.
    cano, src [n, 3]; lo, hi [3]; -> handle [n] bool, move [n] bool, tgt [n, 3], cols [n, 4] = [tgt * handle | handle]."""
    r = F(r)
    x, y, z = cano[:, 0], cano[:, 1], cano[:, 2]
    head = y < F(lo[1] + r)
    tail = y > F(hi[1] - r)
    if cliptail:
        tail = tail & (z > -r)
    foot = z < F(lo[2] + r)
    handle = head | tail | foot
    left, right, front, behind = foot & (x > 0), foot & (x < 0), foot & (y < 0), foot & (y > 0)
    move = (head, tail, left & front, right & front, left & behind, right & behind)[part]
    m, h = move.astype(F)[:, None], handle.astype(F)[:, None]
    with np.errstate(invalid="ignore"):                  # (inf * 0 and nan * 0 are among the cases)
        tgt = (src + np.asarray(d, dtype=F)[None, :] * m).astype(F)
        return handle, move, tgt, np.concatenate([(tgt * h).astype(F), h], axis=1)


def cloud(B, n, seed):
    g = np.random.default_rng(seed)
    cano = g.uniform(-0.5, 0.5, (B, n, 3)).astype(F)
    src = g.uniform(-0.5, 0.5, (B, n, 3)).astype(F)
    return cano, src


def run_rows(cano, src, words, handle_mask=None, move_mask=None, extra_shapes=1, bounds=None):
    """The kernel on a [B + extra, n, 7] buffer filled with a sentinel; -> numpy rows (whole buffer), tgt, handle, move, bounds."""
    B, n, _ = src.shape
    tc = torch.from_numpy(cano).to(DEV)
    ts = tc if src is cano else torch.from_numpy(src).to(DEV)
    tb = pu.handle_bounds(tc) if bounds is None else torch.from_numpy(bounds).to(DEV)
    rows = torch.full((B + extra_shapes, n, 7), float(SENTINEL), device=DEV)
    tgt = torch.full((B, n, 3), float(SENTINEL), device=DEV)
    ho, mo = torch.full((B, n), 9, dtype=torch.uint8, device=DEV), torch.full((B, n), 9, dtype=torch.uint8, device=DEV)
    hm = None if handle_mask is None else torch.from_numpy(handle_mask).to(DEV)
    mm = None if move_mask is None else torch.from_numpy(move_mask).to(DEV)
    pu.handle_rows(tc, ts, tb, torch.from_numpy(words).to(DEV), rows[:B], hm, mm, tgt=tgt, handle_out=ho, move_out=mo)
    torch.cuda.synchronize()
    return rows.cpu().numpy(), tgt.cpu().numpy(), ho.cpu().numpy(), mo.cpu().numpy(), tb.cpu().numpy()


def check(cano, src, words, got, handle_mask=None, move_mask=None):
    rows, tgt, ho, mo, bounds = got
    B, n, _ = src.shape
    f = words.view(F)
    assert (bits(rows[:B, :, 0:3]) == bits(SENTINEL)).all(), "columns 0:3 were written"
    assert (bits(rows[B:]) == bits(SENTINEL)).all(), "rows behind the B shapes were written"
    for b in range(B):
        if handle_mask is None:
            handle, move, want_tgt, cols = rule(cano[b], src[b], bounds[b, 0:3], bounds[b, 3:6], int(words[b, 0]),
                                                bool(words[b, 1]), f[b, 2], f[b, 3:6])
        else:
            handle, move = handle_mask[b] != 0, move_mask[b] != 0
            m, h = move.astype(F)[:, None], handle.astype(F)[:, None]
            want_tgt = (src[b] + f[b, 3:6][None, :] * m).astype(F)
            cols = np.concatenate([(want_tgt * h).astype(F), h], axis=1)
        assert (ho[b] == handle.astype(np.uint8)).all(), (b, "handle")
        assert (mo[b] == move.astype(np.uint8)).all(), (b, "move")
        assert (bits(tgt[b]) == bits(want_tgt)).all(), (b, "tgt", np.argwhere(bits(tgt[b]) != bits(want_tgt))[:4].tolist())
        assert (bits(rows[b, :, 3:7]) == bits(cols)).all(), (b, "rows", np.argwhere(bits(rows[b, :, 3:7]) != bits(cols))[:4].tolist())


# ---------------------------------------------------------------------------------------------------- bounds
@pytest.mark.parametrize("n", SIZES + (4097, 9000))
def test_bounds_equal_min_max_bit_for_bit(n):
    B = 3
    cano, _ = cloud(B, n, 100 + n)
    cano[1] *= F(3.0)
    cano[2, -1] = (F(7.5), F(-8.5), F(9.5))            # the extreme of shape 2 is its LAST point, in all three columns
    if n > 1:
        cano[0, 0] = (F(-6.0), F(6.0), F(-6.5))        # ... and of shape 0 its first
    got = pu.handle_bounds(torch.from_numpy(cano).to(DEV)).cpu().numpy()
    want = np.concatenate([cano.min(axis=1), cano.max(axis=1)], axis=1)
    assert (bits(got) == bits(want)).all(), (got, want)


def test_bounds_order_signed_zeros():
    """-0.0 sorts below +0.0 (nsdp_handles.h): a column holding both as its extremes gets -0.0 as minimum, +0.0 as maximum."""
    cano = np.zeros((1, 130, 3), dtype=F)
    cano[0, 5::2, 0] = F(-0.0)
    cano[0, :, 1] = F(-0.0)
    got = pu.handle_bounds(torch.from_numpy(cano).to(DEV)).cpu().numpy()
    assert np.signbit(got[0, 0]) and not np.signbit(got[0, 3])
    assert np.signbit(got[0, 1]) and np.signbit(got[0, 4])
    assert not np.signbit(got[0, 2]) and not np.signbit(got[0, 5])
    assert (got == 0).all()


def test_bounds_workspace_and_out_arguments():
    cano, _ = cloud(2, 300, 5)
    t = torch.from_numpy(cano).to(DEV)
    ws = torch.empty(1 << 12, dtype=torch.int32, device=DEV)
    out = torch.empty(2, 6, device=DEV)
    assert pu.handle_bounds(t, workspace=ws, out=out) is out
    assert torch.equal(out, pu.handle_bounds(t))
    with pytest.raises(RuntimeError, match="workspace"):
        pu.handle_bounds(t, workspace=torch.empty(1, dtype=torch.int32, device=DEV))


# ---------------------------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("cliptail", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_rows_follow_the_rule_for_every_part(n, cliptail):
    """Two calls cover the six parts over B = 3 shapes, each shape with its own part and translation."""
    B = 3
    cano, src = cloud(B, n, 7 * n + cliptail)
    for parts in (PARTS[0:3], PARTS[3:6]):
        d = np.array([[-0.15, -0.2, -0.2], [0.15, 0.0, -0.0], [0.3, 0.25, -0.125]], dtype=F)
        words = pack_params(B, list(parts), d, 0.1, cliptail)
        check(cano, src, words, run_rows(cano, src, words))


def test_rows_take_the_rule_coordinates_from_cano_and_the_target_from_src():
    """cano == src (the reference: every frame of a pair is frame 0000) through ONE tensor passed twice."""
    B, n = 3, 257
    cano, _ = cloud(B, n, 11)
    words = pack_params(B, ["head", "tail", "frontleftfoot"], (0.1, 0.2, 0.3), 0.15, False)
    check(cano, cano, words, run_rows(cano, cano, words))


def test_points_exactly_on_the_thresholds_are_outside():
    """The comparisons are strict: a point whose coordinate EQUALS lo + r, hi - r or -r is no handle; one ulp inside is."""
    B, n, r = 3, 65, F(0.125)
    cano, src = cloud(B, n, 3)
    cano *= F(0.25)                                    # the bulk well inside the box
    lo, hi = np.array([-1.0, -1.0, -1.0], dtype=F), np.array([1.0, 1.0, 1.0], dtype=F)
    for b in range(B):
        cano[b, 0], cano[b, 1] = lo, hi                # the box's corners: y = lo.y -> head, z = lo.z -> foot; y = hi.y -> tail
        y_head, y_tail, z_foot = F(lo[1] + r), F(hi[1] - r), F(lo[2] + r)
        cano[b, 2] = (0.5, y_head, 0.0)                                        # ON the head threshold
        cano[b, 3] = (0.5, np.nextafter(y_head, F(-2)), 0.0)                   # one ulp inside
        cano[b, 4] = (0.5, y_tail, 0.0)                                        # ON the tail threshold
        cano[b, 5] = (0.5, np.nextafter(y_tail, F(2)), 0.0)
        cano[b, 6] = (0.5, 0.0, z_foot)                                        # ON the foot threshold
        cano[b, 7] = (0.5, 0.0, np.nextafter(z_foot, F(-2)))
        cano[b, 8] = (0.5, np.nextafter(y_tail, F(2)), -r)                     # tail, ON the cliptail threshold z = -r
        cano[b, 9] = (0.5, np.nextafter(y_tail, F(2)), np.nextafter(-r, F(1)))
        cano[b, 10] = (0.0, -0.5, np.nextafter(z_foot, F(-2)))                 # foot with x == 0: no left, no right foot
        cano[b, 11] = (0.5, 0.0, np.nextafter(z_foot, F(-2)))                  # foot with y == 0: no front, no behind foot
        cano[b, 12] = (-0.0, -0.5, np.nextafter(z_foot, F(-2)))                # x = -0.0 is not < 0
    for cliptail in (False, True):
        for parts in (PARTS[0:3], PARTS[3:6], ("tail", "tail", "head")):
            words = pack_params(B, list(parts), (0.5, -0.25, 0.125), r, cliptail)
            got = run_rows(cano, src, words)
            check(cano, src, words, got)
            handle = got[2][0]
            assert handle[0] == 1 and handle[1] == 1
            assert handle[2] == 0 and handle[3] == 1 and handle[4] == 0 and handle[6] == 0 and handle[7] == 1
            assert handle[5] == 1 and handle[8] == (0 if cliptail else 1) and handle[9] == 1
    words = pack_params(B, list(PARTS[2:5]), (0.5, -0.25, 0.125), r, False)
    move = run_rows(cano, src, words)[3]
    assert not move[:, 10:13].any()                    # x == 0, y == 0, x == -0.0: none of the four feet


def test_signed_zeros_and_nans_come_out_as_the_array_expressions():
    """-0.0 and negative source coordinates under a zero mask (x * 0 keeps the sign: -0.0), negative translations under a zero
    move (d * 0 = -0.0, and -0.0 + -0.0 = -0.0 while +0.0 + -0.0 = +0.0), NaN and infinite translations and sources."""
    B, n = 3, 64
    cano, src = cloud(B, n, 21)
    src[:, 0] = (-0.0, 0.0, -0.0)
    src[:, 1] = (-0.25, -0.0, 0.5)
    src[:, 2] = (np.nan, np.inf, -np.inf)
    src[:, 3] = (-0.0, -0.0, -0.0)
    cano[:, 0:4] = 0.0                                  # the four special rows sit in the middle of the box: no handle, no move
    cano[:, 4] = (0.4, -0.6, -0.6)                      # ... and two that are handle and move
    cano[:, 5] = (-0.4, -0.6, -0.6)
    src[:, 4] = (-0.0, 0.0, np.nan)
    src[:, 5] = (-0.0, -0.0, 1.0)
    d = np.array([[-0.15, -0.2, 0.2], [np.nan, np.inf, -0.0], [0.0, -0.0, -1.0]], dtype=F)
    words = pack_params(B, ["head", "frontleftfoot", "frontrightfoot"], d, 0.1, False)
    got = run_rows(cano, src, words)
    check(cano, src, words, got)
    rows, tgt = got[0], got[1]
    assert got[2][:, 0:4].sum() == 0 and got[3][:, 0:4].sum() == 0 and got[2][:, 4:6].all()
    # shape 0: d = (-0.15, -0.2, 0.2), m = 0 -> d * m = (-0, -0, +0); src row 0 = (-0, +0, -0) -> tgt = (-0, +0, +0)
    assert np.signbit(tgt[0, 0]).tolist() == [True, False, False]
    # ... times h = 0: the sign of the target stays, (-0, +0, +0); row 1 = (-0.25, -0, 0.5) -> (-0, -0, +0)
    assert np.signbit(rows[0, 0, 3:6]).tolist() == [True, False, False]
    assert np.signbit(rows[0, 1, 3:6]).tolist() == [True, True, False] and (rows[0, 1, 3:6] == 0).all()
    # row 2 = (nan, inf, -inf) under h = 0: nan * 0, inf * 0, -inf * 0 are all NaN
    assert np.isnan(rows[0, 2, 3:6]).all()
    # shape 1: d = (nan, inf, -0) under m = 0: nan * 0 = nan, inf * 0 = nan -> the target of an UNMOVED point is NaN, as src + d * m
    assert np.isnan(tgt[1, 0, 0:2]).all() and np.signbit(tgt[1, 0, 2])
    # the same on the GPU as torch's array expressions, NaN payloads included: equal as integers
    ts, td = torch.from_numpy(src).to(DEV), torch.from_numpy(d).to(DEV)[:, None, :]
    m = torch.from_numpy(got[3]).to(DEV)[:, :, None].float()
    h = torch.from_numpy(got[2]).to(DEV)[:, :, None].float()
    want_tgt = ts + td * m
    want_cols = torch.cat([want_tgt * h, h], dim=-1)
    assert torch.equal(torch.from_numpy(tgt).to(DEV).view(torch.int32), want_tgt.view(torch.int32))
    assert torch.equal(torch.from_numpy(rows[:B, :, 3:7].copy()).to(DEV).view(torch.int32), want_cols.view(torch.int32))


def test_an_empty_and_an_all_points_region():
    B, n = 3, 257
    cano, src = cloud(B, n, 31)
    words = pack_params(B, ["head", "tail", "behindleftfoot"], (0.1, -0.1, 0.2), [0.0, 2.0, 0.0], False)
    got = run_rows(cano, src, words)
    check(cano, src, words, got)
    assert got[2][0].sum() == 0 and got[3][0].sum() == 0               # r = 0: y < lo.y for no point
    assert got[2][1].all() and got[3][1].all()                          # r = 2: every point is head, tail and foot
    assert got[2][2].sum() == 0 and got[3][2].sum() == 0


def test_a_part_outside_the_table_moves_nothing():
    B, n = 3, 64
    cano, src = cloud(B, n, 41)
    words = pack_params(B, "head", (0.1, 0.2, 0.3), 0.1, False)
    words[:, 0] = (6, -1, 1 << 30)
    got = run_rows(cano, src, words)
    assert got[3].sum() == 0 and got[2].sum() > 0


@pytest.mark.parametrize("n", (1, 65, 1025))
def test_explicit_masks_replace_the_rule(n):
    B = 3
    cano, src = cloud(B, n, 51 + n)
    g = np.random.default_rng(n)
    hm = (g.uniform(size=(B, n)) < 0.5).astype(np.uint8) * np.uint8(3)      # (any non-zero byte counts)
    mm = (g.uniform(size=(B, n)) < 0.3).astype(np.uint8)
    hm[1], mm[1] = 0, 1                                                     # an empty handle whose every point moves
    hm[2], mm[2] = 1, 0
    words = pack_params(B, "head", [(0.1, 0.2, 0.3), (-0.1, -0.2, -0.3), (0.0, -0.0, 5.0)], 0.1, True)
    got = run_rows(cano, src, words, hm, mm)
    check(cano, src, words, got, hm, mm)
    # the mask form reads neither cano nor bounds: bool masks, both None
    rows = torch.full((B, n, 7), float(SENTINEL), device=DEV)
    pu.handle_rows(None, torch.from_numpy(src).to(DEV), None, torch.from_numpy(words).to(DEV), rows,
                   torch.from_numpy(hm != 0).to(DEV), torch.from_numpy(mm != 0).to(DEV))
    assert (bits(rows.cpu().numpy()) == bits(got[0][:B])).all()
    with pytest.raises(RuntimeError, match="go together"):
        pu.handle_rows(None, torch.from_numpy(src).to(DEV), None, torch.from_numpy(words).to(DEV), rows,
                       torch.from_numpy(hm).to(DEV), None)


def test_optional_outputs_may_be_left_out():
    B, n = 3, 63
    cano, src = cloud(B, n, 61)
    words = pack_params(B, "tail", (0.1, 0.2, 0.3), 0.1, False)
    full = run_rows(cano, src, words, extra_shapes=0)
    tc, ts = torch.from_numpy(cano).to(DEV), torch.from_numpy(src).to(DEV)
    rows = torch.full((B, n, 7), float(SENTINEL), device=DEV)
    assert pu.handle_rows(tc, ts, pu.handle_bounds(tc), torch.from_numpy(words).to(DEV), rows) is rows
    assert (bits(rows.cpu().numpy()) == bits(full[0])).all()
