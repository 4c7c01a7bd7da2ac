"""CPU: the boundary of the labelled-handle-set entries -- include/nsdp_handle_sets.h declares the two entries and the built
library exports them at ABI version 17, beside nsdp_handles.h and nsdp_handles_ragged.h, which keep their own; handle_sets.hip is
built without contraction; every bad argument comes back as a status with a message before anything is launched, sizes judged
before pointers -- and the host side of nsdp_amd.edit: Motion composes in float64 and rounds once, pack_motions' shapes and
refusals, reference_pose_dict's identity, the command line."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from nsdp_amd import _lib, build as nsdp_build, edit
from nsdp_amd.edit import Motion, pack_motions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nsdp_handle_sets.h")
ENTRY_POINTS = ["nsdp_handle_set_rows", "nsdp_handle_set_rows_ragged"]
ULP = float(np.finfo(np.float32).eps)      # the spacing of float32 at 1


@pytest.fixture(scope="module")
def so():
    if not os.path.exists(_lib.SO_PATH):
        nsdp_build.build()
    lib = ctypes.CDLL(_lib.SO_PATH)
    lib.nsdp_last_error.restype = ctypes.c_char_p
    return lib


def test_header_declares_and_library_exports_the_entries(so):
    with open(HEADER) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(nsdp_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(ENTRY_POINTS)
    for name in ENTRY_POINTS:
        assert hasattr(so, name), name
    assert so.nsdp_abi_version() >= 17
    assert not set(ENTRY_POINTS) & set(_lib.declared_symbols())          # (nsdp_hip.h keeps its own table of entries)
    for other in ("nsdp_handles.h", "nsdp_handles_ragged.h"):             # (and so do the two rule headers)
        assert "nsdp_handle_set_rows" not in open(os.path.join(ROOT, "include", other)).read()
    assert nsdp_build.HANDLE_SETS_HEADER == HEADER and "HANDLE_SETS_HEADER" in open(nsdp_build.__file__).read().split("def _deps_mtime")[1]
    assert nsdp_build.PER_FILE["handle_sets.hip"] == nsdp_build.EXACT
    assert "handle_sets.hip" in nsdp_build.sources()
    assert os.path.basename(HEADER) in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_bad_arguments_return_status(so):
    one = ctypes.c_void_p(16)      # (a non-null pointer the library must not touch before it has checked everything)
    odd = ctypes.c_void_p(18)
    fn = so.nsdp_handle_set_rows
    # (src, labels, motions, targets, B, n, H, T, rows, tgt, handle_out, stream)
    ok = dict(src=one, labels=one, motions=one, targets=None, B=1, n=8, H=3, T=1, rows=one, tgt=one, ho=one)

    def rows(**kw):
        a = dict(ok, **kw)
        return fn(a["src"], a["labels"], a["motions"], a["targets"], a["B"], a["n"], a["H"], a["T"], a["rows"], a["tgt"], a["ho"], None)

    assert rows(B=0) == -1 and b"batch 0" in so.nsdp_last_error()
    assert rows(B=65536) == -1 and b"batch 65536" in so.nsdp_last_error()
    assert rows(n=0) == -1 and b"n=0" in so.nsdp_last_error()
    assert rows(n=(1 << 20) + 1) == -1 and b"n=1048577" in so.nsdp_last_error()
    assert rows(T=0) == -1 and b"T=0" in so.nsdp_last_error()
    assert rows(T=-2) == -1 and b"T=-2" in so.nsdp_last_error()
    assert rows(T=256, B=256) == -1 and b"T*B=65536" in so.nsdp_last_error()
    assert rows(T=65535, B=65535) == -1 and b"T*B=4294836225" in so.nsdp_last_error()      # (the product is formed in 64 bits)
    assert rows(H=0) == -1 and b"H=0" in so.nsdp_last_error()
    assert rows(H=256) == -1 and b"H=256" in so.nsdp_last_error()
    assert rows(targets=one) == -1 and b"exactly one of motions and targets (got both)" in so.nsdp_last_error()
    assert rows(motions=None) == -1 and b"exactly one of motions and targets (got neither)" in so.nsdp_last_error()
    for missing in ("src", "labels", "rows"):
        assert rows(**{missing: None}) == -1 and b"null" in so.nsdp_last_error(), missing
    for which in ("src", "motions", "rows", "tgt"):
        assert rows(**{which: odd}) == -1 and b"aligned" in so.nsdp_last_error(), which
    assert rows(motions=None, targets=odd, H=0) == -1 and b"aligned" in so.nsdp_last_error()
    assert rows(motions=None, targets=one, H=0, rows=None) == -1 and b"null" in so.nsdp_last_error()      # (H is not read with targets)
    # sizes are judged before pointers
    assert fn(None, None, None, None, 1, 0, 3, 1, None, None, None, None) == -1 and b"n=0" in so.nsdp_last_error()
    assert fn(None, None, None, None, 1, 8, 3, 0, None, None, None, None) == -1 and b"T=0" in so.nsdp_last_error()

    fn = so.nsdp_handle_set_rows_ragged
    # (src, offsets, labels, motions, targets, B, cap, H, rows, tgt, handle_out, stream)
    ok = dict(src=one, offsets=one, labels=one, motions=one, targets=None, B=1, cap=8, H=3, rows=one, tgt=one, ho=one)

    def packed(**kw):
        a = dict(ok, **kw)
        return fn(a["src"], a["offsets"], a["labels"], a["motions"], a["targets"], a["B"], a["cap"], a["H"], a["rows"], a["tgt"],
                  a["ho"], None)

    assert packed(B=0) == -1 and b"batch 0" in so.nsdp_last_error()
    assert packed(B=65536) == -1 and b"batch 65536" in so.nsdp_last_error()
    assert packed(cap=0) == -1 and b"cap=0" in so.nsdp_last_error()
    assert packed(cap=-7) == -1 and b"cap=-7" in so.nsdp_last_error()
    assert packed(H=0) == -1 and b"H=0" in so.nsdp_last_error()
    assert packed(H=256) == -1 and b"H=256" in so.nsdp_last_error()
    assert packed(targets=one) == -1 and b"got both" in so.nsdp_last_error()
    assert packed(motions=None) == -1 and b"got neither" in so.nsdp_last_error()
    for missing in ("src", "offsets", "labels", "rows"):
        assert packed(**{missing: None}) == -1 and b"null" in so.nsdp_last_error(), missing
    for which in ("src", "offsets", "motions", "rows", "tgt"):
        assert packed(**{which: odd}) == -1 and b"aligned" in so.nsdp_last_error(), which
    assert packed(motions=None, targets=odd, H=0) == -1 and b"aligned" in so.nsdp_last_error()
    assert fn(None, None, None, None, None, 1, 0, 3, None, None, None, None) == -1 and b"cap=0" in so.nsdp_last_error()


def test_wrappers_refuse_cpu_tensors_and_inconsistent_shapes():
    from nsdp_amd import pointnet2_utils as pu
    src, lab, rows = torch.zeros(1, 8, 3), torch.zeros(1, 8, dtype=torch.uint8), torch.zeros(1, 1, 8, 7)
    with pytest.raises(_lib.NsdpHipError, match="GPU tensor"):
        pu.handle_set_rows(src, lab, rows, motions=torch.zeros(1, 1, 2, 12))
    with pytest.raises(_lib.NsdpHipError, match="GPU tensor"):
        pu.handle_set_rows_ragged(src[0], torch.tensor([0, 8], dtype=torch.int32), lab[0], rows[0, 0], motions=torch.zeros(1, 2, 12))


# ---------------------------------------------------------------------------------------------------- Motion
def _apply32(m, p):
    """The float32 matrix of a motion applied to a point, in float64 (the arithmetic adds nothing to the matrix's one rounding)."""
    a = m.matrix().astype(np.float64)
    return a[:, :3] @ np.asarray(p, dtype=np.float64) + a[:, 3]


def test_motion_identity_is_exactly_the_identity():
    want = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], dtype=np.float32)
    got = Motion.identity().matrix()
    assert got.dtype == np.float32 and got.shape == (3, 4) and got.tobytes() == want.tobytes()
    assert Motion.identity().then(Motion.identity()).matrix().tobytes() == want.tobytes()
    assert Motion.rotate((0, 0, 1), 0.0).matrix().tobytes() == want.tobytes()
    assert Motion.translate((0.25, -1.0, 3.0)).matrix().tolist() == [[1, 0, 0, 0.25], [0, 1, 0, -1.0], [0, 0, 1, 3.0]]
    assert Motion.affine(np.diag([2.0, 3.0, 4.0]), (1, 2, 3)).matrix().tolist() == [[2, 0, 0, 1], [0, 3, 0, 2], [0, 0, 4, 3]]


@pytest.mark.parametrize("axis,vec,want", [((0, 0, 1), (1, 0, 0), (0, 1, 0)), ((0, 0, 2.5), (0, 1, 0), (-1, 0, 0)),
                                           ((1, 0, 0), (0, 1, 0), (0, 0, 1)), ((0, 1, 0), (0, 0, 1), (1, 0, 0))])
def test_rotate_90_of_a_unit_vector(axis, vec, want):
    got = _apply32(Motion.rotate(axis, 90.0), vec)
    assert np.abs(got - np.asarray(want, dtype=np.float64)).max() <= ULP, got      # 1 ulp of the unit length
    back = _apply32(Motion.rotate(axis, -90.0), want)
    assert np.abs(back - np.asarray(vec, dtype=np.float64)).max() <= ULP, back


def test_rotate_a_general_angle():
    got = _apply32(Motion.rotate((0, 0, 1), 30.0), (1, 0, 0))
    assert np.abs(got - np.array([np.sqrt(3) / 2, 0.5, 0.0])).max() <= ULP
    got = _apply32(Motion.rotate((1, 1, 1), 120.0), (1, 0, 0))      # a third of a turn about the diagonal: x -> y
    assert np.abs(got - np.array([0.0, 1.0, 0.0])).max() <= ULP
    with pytest.raises(ValueError, match="axis"):
        Motion.rotate((0, 0, 0), 10.0)


def test_then_is_associative_on_a_fixed_case():
    a = Motion.rotate((1, 2, 3), 37.0, pivot=(0.1, -0.2, 0.3))
    b = Motion.translate((0.5, -0.25, 0.125))
    c = Motion.affine([[1.1, 0.2, 0.0], [0.0, 0.9, -0.1], [0.3, 0.0, 1.0]], (0.01, 0.02, -0.03))
    left, right = a.then(b).then(c).matrix(), a.then(b.then(c)).matrix()
    scale = np.abs(left).max()
    assert np.abs(left.astype(np.float64) - right.astype(np.float64)).max() <= float(np.spacing(np.float32(scale)))      # 1 ulp of the largest entry
    # and `then` means: the first motion first
    p = np.array([0.3, -0.4, 0.5])
    assert np.allclose(_apply32(a.then(b), p), _apply32(b, _apply32(a, p)), rtol=0, atol=4 * ULP)
    assert not np.allclose(_apply32(a.then(b), p), _apply32(a, _apply32(b, p)), rtol=0, atol=1e-3)


@pytest.mark.parametrize("pivot", [(0.25, -0.5, 0.125), (3.0, 4.0, 12.0), (-1e-3, 2e-3, 5e-4), (100.0, -250.0, 75.0)])
def test_the_pivot_stays_fixed(pivot):
    c = np.asarray(pivot, dtype=np.float64)
    for axis, deg in (((0, 0, 1), 20.0), ((1, -2, 0.5), 123.0), ((0, 1, 0), 90.0), ((1, 1, 0), -45.0)):
        moved = _apply32(Motion.rotate(axis, deg, pivot=pivot), c)
        assert np.linalg.norm(moved - c) <= 4 * float(np.spacing(np.float32(np.linalg.norm(c)))), (axis, deg, moved - c)      # 4 ulp of |c|


# ---------------------------------------------------------------------------------------------------- pack_motions
def test_pack_motions_shapes():
    r, t, i = Motion.rotate((0, 0, 1), 20.0, pivot=(0.1, 0.2, 0.3)), Motion.translate((1, 2, 3)), Motion.identity()
    one = pack_motions(2, 3, [r, t, i])                                   # one list, broadcast over the shapes
    assert one.shape == (2, 3, 12) and one.dtype == np.float32 and one.flags["C_CONTIGUOUS"]
    assert np.array_equal(one[0], one[1]) and np.array_equal(one[0, 0], r.matrix().reshape(12))
    assert one[0, 1].tolist() == [1, 0, 0, 1, 0, 1, 0, 2, 0, 0, 1, 3] and one[0, 2].tolist() == [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
    per = pack_motions(2, 3, [[r, t, i], [i, i, t]])                      # a list per shape
    assert np.array_equal(per[0], one[0]) and np.array_equal(per[1, 2], one[0, 1]) and np.array_equal(per[1, 0], one[0, 2])
    assert np.array_equal(pack_motions(2, 3, per), per)                    # an array that already has the shape
    assert np.array_equal(pack_motions(2, 3, per.reshape(2, 3, 3, 4)), per)
    assert np.array_equal(pack_motions(2, 3, torch.from_numpy(per)), per)
    assert np.array_equal(pack_motions(2, 3, per[0]), np.stack([per[0], per[0]]))
    mixed = pack_motions(1, 2, [np.arange(12.0), np.arange(12.0).reshape(3, 4) + 1])      # 12 numbers in either shape
    assert mixed[0, 0].tolist() == list(range(12)) and mixed[0, 1].tolist() == list(range(1, 13))
    assert pack_motions(3, 3, [[i, i, i], [t, t, t], [r, r, r]])[1, 0].tolist() == one[0, 1].tolist()      # B == H: lists are shapes


def test_pack_motions_refusals():
    i = Motion.identity()
    with pytest.raises(ValueError, match="neither 3 motions .* nor 2 lists"):
        pack_motions(2, 3, [i, i])
    with pytest.raises(ValueError, match="shape 1 has 2 motions for 3 handles"):
        pack_motions(2, 3, [[i, i, i], [i, i]])
    with pytest.raises(ValueError, match="no 3 x 4 motion"):
        pack_motions(2, 3, [[i, i, i], [i, i, np.zeros(5)]])
    with pytest.raises(ValueError, match=r"must be \[2, 3, 12\]"):
        pack_motions(2, 3, np.zeros((3, 2, 12), dtype=np.float32))
    with pytest.raises(ValueError, match="a list of 3 motions"):
        pack_motions(2, 3, i)
    with pytest.raises(ValueError, match="3 x 4 matrix"):
        Motion(np.zeros((4, 4)))


# ---------------------------------------------------------------------------------------------------- the torch reference
def test_reference_pose_dict_with_identities_returns_the_source_bits():
    g = torch.Generator().manual_seed(4)
    # coordinates without zeros: 1 * (-0) + 0 * y is +0, the one pattern an identity MOTION does not hand back
    verts = (torch.rand(2, 97, 3, generator=g) + 0.25) * torch.where(torch.rand(2, 97, 3, generator=g) < 0.5, -1.0, 1.0)
    surface = (torch.rand(2, 64, 3, generator=g) + 0.25) * torch.where(torch.rand(2, 64, 3, generator=g) < 0.5, -1.0, 1.0)
    labels = torch.randint(0, 6, (2, 64), generator=g).to(torch.uint8)      # 0..5 with H = 3: 4 and 5 are free points
    vlabels = torch.randint(0, 6, (2, 97), generator=g).to(torch.uint8)
    dd = edit.reference_pose_dict(verts, surface, labels, 3, motions=[Motion.identity()] * 3, vert_labels=vlabels)
    handle = (labels >= 1) & (labels <= 3)
    assert torch.equal(dd["cano_handle_sample_idx"], handle) and torch.equal(dd["cano_handle_vert_idx"], (vlabels >= 1) & (vlabels <= 3))
    assert torch.equal(dd["verts_tgt"].view(torch.int32), verts.view(torch.int32))
    inputs = dd["surface_samples_inputs"]
    assert inputs.shape == (2, 64, 7) and torch.equal(inputs[:, :, 0:3], surface) and torch.equal(inputs[:, :, 6], handle.float())
    assert torch.equal(inputs[:, :, 3:6], surface * handle[:, :, None].float())
    # the cloud is the vertex set: one set of labels serves both; no vertex labels with a separate cloud: no vertex targets
    same = edit.reference_pose_dict(verts, None, vlabels, 3, motions=[Motion.identity()] * 3)
    assert torch.equal(same["verts_tgt"], verts) and same["cano_handle_vert_idx"] is same["cano_handle_sample_idx"]
    assert edit.reference_pose_dict(verts, surface, labels, 3, motions=[Motion.identity()] * 3)["verts_tgt"] is None
    # targets: copied at every non-zero label, the source elsewhere
    tg = torch.rand(2, 64, 3, generator=g)
    dd = edit.reference_pose_dict(verts, surface, labels, 3, targets=tg)
    assert torch.equal(dd["cano_handle_sample_idx"], labels != 0)
    assert torch.equal(dd["surface_samples_inputs"][:, :, 3:6], tg * (labels != 0)[:, :, None].float())
    # a translation moves exactly the labelled points, by separate roundings
    d = np.float32(0.1), np.float32(-0.2), np.float32(0.3)
    dd = edit.reference_pose_dict(verts, None, vlabels, 1, motions=[Motion.translate(d)])
    one = (vlabels == 1)[:, :, None]
    assert torch.equal(dd["verts_tgt"], torch.where(one, ((verts * 1.0 + 0.0) + 0.0) + torch.tensor(d), verts))
    with pytest.raises(ValueError, match="exactly one of motions and targets"):
        edit.reference_pose_dict(verts, None, vlabels, 3)


# ---------------------------------------------------------------------------------------------------- the command line
def test_cli_flags_parse():
    ap = edit.build_parser()
    a = ap.parse_args(["cfg.yaml"])
    assert (a.handles, a.rotate_deg, a.axis, a.track) == (None, 0.0, "0,0,1", None) and edit.handles_from_args(a) == (None, None)
    a = ap.parse_args(["cfg.yaml", "--handles", "head,frontleftfoot", "--rotate-deg", "20", "--axis", "0,1,0", "--track", "4"])
    assert edit.handles_from_args(a) == (["head", "frontleftfoot"], (0.0, 1.0, 0.0)) and a.track == 4 and a.rotate_deg == 20.0
    for bad in (["--handles", "nose"], ["--handles", "head,head"], ["--handles", "head", "--axis", "0,0,0"],
                ["--handles", "head", "--axis", "1,2"], ["--handles", "head", "--track", "0"], ["--track", "3"],
                ["--rotate-deg", "5"]):
        with pytest.raises(SystemExit):
            edit.handles_from_args(ap.parse_args(["cfg.yaml"] + bad))
