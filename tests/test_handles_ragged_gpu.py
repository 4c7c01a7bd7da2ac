"""The packed user-handle kernels (include/nsdp_handles_ragged.h) against the rectangular ones (include/nsdp_handles.h) on each
shape alone at B = 1: every comparison is exact equality of bits.  Shape counts (1, 255, 256, 257, 4096, 4097, 0, 700) in a
buffer of total + 300 rows: the one-row shape, the wave and workgroup edges of the rows kernel, the partial-group edge of the
bounds kernel (4096 rows per partial workgroup), an empty shape in the middle, and padding behind the last shape.  The rule
with another part, translation, partial_range and cliptail per shape, and the mask form; rows at or beyond the total and
columns 0:3 keep a sentinel; -0.0, +0.0, an infinity and a NaN in one cloud; a larger n_max; capture + replay."""
import numpy as np
import pytest
import torch

from nsdp_amd import pointnet2_utils as pu
from nsdp_amd.edit import PARTS, pack_params
from nsdp_amd.ragged import offsets_of

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
COUNTS = (1, 255, 256, 257, 4096, 4097, 0, 700)
PAD = 300
SENTINEL = -7.25


def i32(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def case():
    """The packed operands, the per-shape drags and -- computed once, by the rectangular entries on each shape alone -- what
    every output must hold."""
    B, total = len(COUNTS), sum(COUNTS)
    cap = total + PAD
    g = torch.Generator().manual_seed(2024)
    cano = (torch.rand(cap, 3, generator=g) - 0.5).to(DEV)
    src = (torch.rand(cap, 3, generator=g) - 0.5).to(DEV)
    hm = (torch.rand(cap, generator=g) < 0.5).to(torch.uint8).mul_(3).to(DEV)      # (any non-zero byte counts)
    mm = (torch.rand(cap, generator=g) < 0.3).to(DEV)                              # (bool: one byte as well)
    parts = [PARTS[b % len(PARTS)] for b in range(B)]
    d = np.array([[-0.15, -0.2, -0.2], [0.15, 0.0, -0.0], [0.3, 0.25, -0.125], [-0.15, 0.15, -0.15], [0.15, -0.2, 0.2],
                  [-0.15, -0.2, 0.2], [1.0, 2.0, 3.0], [0.05, 0.1, -0.1]], dtype=np.float32)
    r = [0.1, 0.2, 0.15, 0.1, 0.05, 0.1, 0.1, 0.3]
    clip = [False, True, False, True, False, True, False, True]
    words = pack_params(B, parts, d, r, clip)
    offsets = offsets_of(COUNTS, DEV)
    starts = np.concatenate([[0], np.cumsum(COUNTS)])
    want = []
    for b, n in enumerate(COUNTS):
        if n == 0:
            want.append(None)
            continue
        lo, hi = int(starts[b]), int(starts[b + 1])
        c1, s1 = cano[lo:hi].unsqueeze(0).contiguous(), src[lo:hi].unsqueeze(0).contiguous()
        w1 = torch.from_numpy(words[b:b + 1].copy()).to(DEV)
        bounds = pu.handle_bounds(c1)
        out = {"bounds": bounds}
        for form, masks in (("rule", (None, None)), ("masks", (hm[lo:hi].unsqueeze(0).contiguous(), mm[lo:hi].unsqueeze(0).contiguous()))):
            rows = torch.full((1, n, 7), SENTINEL, device=DEV)
            tgt = torch.empty((1, n, 3), device=DEV)
            ho, mo = torch.empty((1, n), dtype=torch.uint8, device=DEV), torch.empty((1, n), dtype=torch.uint8, device=DEV)
            pu.handle_rows(c1, s1, bounds, w1, rows, *masks, tgt=tgt, handle_out=ho, move_out=mo)
            out[form] = (rows[0], tgt[0], ho[0], mo[0])
        want.append(out)
    return dict(B=B, total=total, cap=cap, cano=cano, src=src, hm=hm, mm=mm, words=torch.from_numpy(words).to(DEV),
                offsets=offsets, starts=starts, want=want)


def run_rows(c, masks, bounds=None):
    cap = c["cap"]
    rows = torch.full((cap, 7), SENTINEL, device=DEV)
    tgt = torch.full((cap, 3), SENTINEL, device=DEV)
    ho, mo = torch.full((cap,), 9, dtype=torch.uint8, device=DEV), torch.full((cap,), 9, dtype=torch.uint8, device=DEV)
    bounds = pu.handle_bounds_ragged(c["cano"], c["offsets"], max(COUNTS)) if bounds is None else bounds
    hm, mm = (c["hm"], c["mm"]) if masks else (None, None)
    assert pu.handle_rows_ragged(c["cano"], c["src"], c["offsets"], bounds, c["words"], rows, hm, mm, tgt=tgt, handle_out=ho,
                                 move_out=mo) is rows
    return rows, tgt, ho, mo


def check_rows(c, got, form):
    rows, tgt, ho, mo = got
    total, sent = c["total"], i32(torch.full((1,), SENTINEL, device=DEV))
    assert bool((i32(rows[:, 0:3]) == sent).all()), "columns 0:3 were written"
    assert bool((i32(rows[total:]) == sent).all()) and bool((i32(tgt[total:]) == sent).all()), "padding rows were written"
    assert bool((ho[total:] == 9).all()) and bool((mo[total:] == 9).all()), "padding flags were written"
    for b, n in enumerate(COUNTS):
        if n == 0:
            continue
        lo, hi = int(c["starts"][b]), int(c["starts"][b + 1])
        wrows, wtgt, wh, wm = c["want"][b][form]
        assert torch.equal(ho[lo:hi], wh) and torch.equal(mo[lo:hi], wm), (b, form, "flags")
        assert torch.equal(i32(tgt[lo:hi]), i32(wtgt)), (b, form, "tgt")
        assert torch.equal(i32(rows[lo:hi, 3:7]), i32(wrows[:, 3:7])), (b, form, "rows")
        if n >= 255 and form == "rule":      # (no comparison of nothing with nothing)
            assert 0 < int(wh.sum()) < n, (b, "handle")


def test_bounds_equal_the_rectangular_entry_on_each_shape_alone(case):
    got = pu.handle_bounds_ragged(case["cano"], case["offsets"], max(COUNTS))
    assert got.shape == (case["B"], 6)
    for b, n in enumerate(COUNTS):
        if n:
            assert torch.equal(i32(got[b]), i32(case["want"][b]["bounds"][0])), b
    # the empty shape: the reductions' identities, as the header names them
    empty = COUNTS.index(0)
    assert i32(got[empty]).tolist() == [0x7FFFFFFF] * 3 + [-1] * 3
    # a larger n_max than needed (another grid, other partials): the same bits
    for n_max in (max(COUNTS) + 1, 3 * 4096 + 5, 1 << 20):
        assert torch.equal(i32(pu.handle_bounds_ragged(case["cano"], case["offsets"], n_max)), i32(got)), n_max
    # workspace / out arguments
    ws, out = torch.empty(1 << 12, dtype=torch.int32, device=DEV), torch.empty(case["B"], 6, device=DEV)
    assert pu.handle_bounds_ragged(case["cano"], case["offsets"], max(COUNTS), workspace=ws, out=out) is out
    assert torch.equal(i32(out), i32(got))
    with pytest.raises(RuntimeError, match="workspace"):
        pu.handle_bounds_ragged(case["cano"], case["offsets"], max(COUNTS), workspace=torch.empty(1, dtype=torch.int32, device=DEV))


@pytest.mark.parametrize("form", ["rule", "masks"])
def test_rows_equal_the_rectangular_entry_on_each_shape_alone(case, form):
    check_rows(case, run_rows(case, form == "masks"), form)


def test_the_mask_form_reads_neither_cano_nor_bounds(case):
    c = case
    rows = torch.full((c["cap"], 7), SENTINEL, device=DEV)
    pu.handle_rows_ragged(None, c["src"], c["offsets"], None, c["words"], rows, c["hm"], c["mm"])
    assert torch.equal(i32(rows), i32(run_rows(c, True)[0]))
    with pytest.raises(RuntimeError, match="go together"):
        pu.handle_rows_ragged(None, c["src"], c["offsets"], None, c["words"], rows, c["hm"], None)


def test_signed_zeros_an_infinity_and_a_nan(case):
    """One cloud of three shapes holds -0.0, +0.0, an infinity and a NaN among its coordinates: the packed entries give the bits
    the rectangular ones give on each shape alone (the NaN becomes the bound it touches, the zeros keep their signs)."""
    counts = (130, 65, 257)
    total = sum(counts)
    g = torch.Generator().manual_seed(7)
    cano = torch.rand(total, 3, generator=g) - 0.5
    src = torch.rand(total, 3, generator=g) - 0.5
    cano[0:130, 0] = 0.0
    cano[5:130:2, 0] = -0.0                                # shape 0: x holds both zeros as its extremes
    cano[0:130, 1] = -0.0
    cano[140, 2] = float("inf")                            # shape 1: an infinity and a NaN
    cano[150, 1] = float("nan")
    cano[200, 0] = float("-inf")                           # shape 2
    cano[210, 2] = -float("nan")
    src[3] = torch.tensor([-0.0, 0.0, -0.0])
    src[141] = torch.tensor([float("nan"), float("inf"), -float("inf")])
    src[220] = torch.tensor([-0.0, -0.0, -0.0])
    cano, src = cano.to(DEV), src.to(DEV)
    words_np = pack_params(3, ["head", "frontleftfoot", "tail"], [(-0.15, -0.2, 0.2), (float("nan"), float("inf"), -0.0),
                                                                  (0.0, -0.0, -1.0)], 0.1, [False, False, True])
    words = torch.from_numpy(words_np).to(DEV)
    offsets = offsets_of(counts, DEV)
    bounds = pu.handle_bounds_ragged(cano, offsets, max(counts))
    rows = torch.full((total, 7), SENTINEL, device=DEV)
    tgt = torch.empty((total, 3), device=DEV)
    ho = torch.empty((total,), dtype=torch.uint8, device=DEV)
    pu.handle_rows_ragged(cano, src, offsets, bounds, words, rows, tgt=tgt, handle_out=ho)
    lo = 0
    for b, n in enumerate(counts):
        c1, s1 = cano[lo:lo + n].unsqueeze(0).contiguous(), src[lo:lo + n].unsqueeze(0).contiguous()
        b1 = pu.handle_bounds(c1)
        assert torch.equal(i32(bounds[b]), i32(b1[0])), b
        r1, t1, h1 = torch.full((1, n, 7), SENTINEL, device=DEV), torch.empty((1, n, 3), device=DEV), torch.empty((1, n), dtype=torch.uint8, device=DEV)
        pu.handle_rows(c1, s1, b1, words[b:b + 1].contiguous(), r1, tgt=t1, handle_out=h1)
        assert torch.equal(i32(rows[lo:lo + n]), i32(r1[0])) and torch.equal(i32(tgt[lo:lo + n]), i32(t1[0])), b
        assert torch.equal(ho[lo:lo + n], h1[0]), b
        lo += n
    bb = bounds.cpu()
    assert np.signbit(bb[0, 0].item()) and not np.signbit(bb[0, 3].item()) and bb[0, 0] == 0 and bb[0, 3] == 0
    assert np.signbit(bb[0, 1].item()) and np.signbit(bb[0, 4].item())
    assert torch.isinf(bb[1, 5]) and torch.isnan(bb[1, 4]) and torch.isinf(bb[2, 0]) and torch.isnan(bb[2, 2])


def test_capture_and_replay_equal_the_eager_call(case):
    c = case
    eager_bounds = pu.handle_bounds_ragged(c["cano"], c["offsets"], max(COUNTS))
    eager = run_rows(c, False, eager_bounds)
    cap = c["cap"]
    ws = torch.empty(c["B"] * 2 * 6, dtype=torch.int32, device=DEV)
    bounds = torch.zeros(c["B"], 6, device=DEV)
    rows = torch.full((cap, 7), SENTINEL, device=DEV)
    tgt = torch.full((cap, 3), SENTINEL, device=DEV)
    ho, mo = torch.full((cap,), 9, dtype=torch.uint8, device=DEV), torch.full((cap,), 9, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pu.handle_bounds_ragged(c["cano"], c["offsets"], max(COUNTS), workspace=ws, out=bounds)
        pu.handle_rows_ragged(c["cano"], c["src"], c["offsets"], bounds, c["words"], rows, tgt=tgt, handle_out=ho, move_out=mo)
    assert bool((bounds == 0).all()), "a capture records the kernels, it does not run them"
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(i32(bounds), i32(eager_bounds))
    for got, want in zip((rows, tgt, ho, mo), eager):
        assert torch.equal(got.view(torch.uint8), want.view(torch.uint8))
    check_rows(c, (rows, tgt, ho, mo), "rule")
