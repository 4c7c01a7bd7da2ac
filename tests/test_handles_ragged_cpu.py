"""CPU: the boundary of the packed user-handle entries and of the packed editing session -- include/nsdp_handles_ragged.h
declares the three entries and the built library exports them at ABI version 16, outside nsdp_hip.h's table and beside
nsdp_handles.h, which keeps its own three; handles_ragged.hip is built without contraction; bad arguments come back as a status
with a message before anything is touched, sizes judged before pointers; the wrappers refuse CPU tensors; the new command-line
flags parse; and RaggedEditSession names each refusal that needs no GPU."""
import ctypes
import os
import re

import pytest
import torch

from helpers import build_product, model_cfg
from nsdp_amd import _lib, build as nsdp_build, edit
from nsdp_amd.ragged import RaggedPoints

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nsdp_handles_ragged.h")
ENTRY_POINTS = ["nsdp_handle_bounds_ragged", "nsdp_handle_bounds_ragged_workspace_bytes", "nsdp_handle_rows_ragged"]


@pytest.fixture(scope="module")
def so():
    if not os.path.exists(_lib.SO_PATH):
        nsdp_build.build()
    lib = ctypes.CDLL(_lib.SO_PATH)
    lib.nsdp_last_error.restype = ctypes.c_char_p
    lib.nsdp_handle_bounds_ragged_workspace_bytes.restype = ctypes.c_size_t
    return lib


def test_header_declares_and_library_exports_the_entries(so):
    with open(HEADER) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(nsdp_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(ENTRY_POINTS)
    for name in ENTRY_POINTS:
        assert hasattr(so, name), name
    assert so.nsdp_abi_version() >= 16
    assert not set(ENTRY_POINTS) & set(_lib.declared_symbols())          # (nsdp_hip.h keeps its own table of entries)
    assert os.path.basename(HEADER) in open(nsdp_build.__file__).read()
    assert nsdp_build.HANDLES_RAGGED_HEADER == HEADER
    assert nsdp_build.PER_FILE["handles_ragged.hip"] == nsdp_build.EXACT
    assert "handles_ragged.hip" in nsdp_build.sources()
    # the identities of a shape without rows are named in the header
    full = open(HEADER).read()
    assert "NSDP_HANDLE_BOUNDS_EMPTY_MIN_BITS 0x7fffffffu" in full and "NSDP_HANDLE_BOUNDS_EMPTY_MAX_BITS 0xffffffffu" in full


def test_workspace_bytes_refuses_what_the_entry_refuses(so):
    ws = so.nsdp_handle_bounds_ragged_workspace_bytes      # (B, cap, n_max)
    assert ws(0, 100, 10) == 0 and ws(65536, 100, 10) == 0 and ws(-1, 100, 10) == 0
    assert ws(1, 0, 10) == 0 and ws(1, -3, 10) == 0
    assert ws(1, 100, 0) == 0 and ws(1, 100, -5) == 0 and ws(1, 100, (1 << 20) + 1) == 0
    assert ws(1, 1, 1) > 0 and ws(65535, 1, 1) > 0 and ws(1, 1, 1 << 20) > 0 and ws(1, (1 << 31) - 1, 1) > 0
    assert ws(1, 1, 1) % 4 == 0 and ws(3, 5000, 1025) % 4 == 0
    sizes = [ws(2, 1 << 21, n) for n in (1, 63, 4096, 4097, 100000, 1 << 20)]
    assert sizes == sorted(sizes) and sizes[0] < sizes[-1]                # monotone in n_max
    assert ws(1, 10, 4096) == 6 * 4 and ws(1, 10, 4097) == 2 * 6 * 4       # ceil(n_max / 4096) partials of six words per shape
    assert ws(1, 10, 1 << 20) == 256 * 6 * 4
    assert ws(65535, 10, 1 << 20) == 65535 * ws(1, 10, 1 << 20)
    assert ws(2, 10, 4096) == ws(2, 1 << 30, 4096)                         # (cap sizes nothing)


def test_bad_arguments_return_status(so):
    one = ctypes.c_void_p(16)      # (a non-null pointer the library must not touch before it has checked everything)
    odd = ctypes.c_void_p(18)
    fn = so.nsdp_handle_bounds_ragged
    ok = dict(cano=one, offsets=one, B=1, cap=8, n_max=8, ws=one, bounds=one)

    def bounds(**kw):
        a = dict(ok, **kw)
        return fn(a["cano"], a["offsets"], a["B"], a["cap"], a["n_max"], a["ws"], a["bounds"], None)

    assert bounds(B=0) == -1 and b"batch" in so.nsdp_last_error()
    assert bounds(B=65536) == -1 and b"batch" in so.nsdp_last_error()
    assert bounds(cap=0) == -1 and b"cap=0" in so.nsdp_last_error()
    assert bounds(n_max=0) == -1 and b"n_max=0" in so.nsdp_last_error()
    assert bounds(n_max=(1 << 20) + 1) == -1 and b"n_max=1048577" in so.nsdp_last_error()
    for missing in ("cano", "offsets", "ws", "bounds"):
        assert bounds(**{missing: None}) == -1 and b"null" in so.nsdp_last_error(), missing
    for which in ("cano", "offsets", "ws", "bounds"):
        assert bounds(**{which: odd}) == -1 and b"aligned" in so.nsdp_last_error(), which
    # sizes are judged before pointers
    assert fn(None, None, 1, 8, 0, None, None, None) == -1 and b"n_max=0" in so.nsdp_last_error()
    assert fn(None, None, 0, 8, 8, None, None, None) == -1 and b"batch" in so.nsdp_last_error()

    fn = so.nsdp_handle_rows_ragged
    # (cano, src, offsets, bounds, params, handle_mask, move_mask, B, cap, rows, tgt, handle_out, move_out, stream)
    ok = dict(cano=one, src=one, offsets=one, bounds=one, params=one, hm=None, mm=None, B=1, cap=4, rows=one, tgt=one, ho=one,
              mo=one)

    def rows(**kw):
        a = dict(ok, **kw)
        return fn(a["cano"], a["src"], a["offsets"], a["bounds"], a["params"], a["hm"], a["mm"], a["B"], a["cap"], a["rows"],
                  a["tgt"], a["ho"], a["mo"], None)

    assert rows(B=0) == -1 and b"batch" in so.nsdp_last_error()
    assert rows(B=65536) == -1 and b"batch" in so.nsdp_last_error()
    assert rows(cap=0) == -1 and b"cap=0" in so.nsdp_last_error()
    assert rows(cap=-7) == -1 and b"cap=-7" in so.nsdp_last_error()
    for missing in ("src", "offsets", "params", "rows"):
        assert rows(**{missing: None}) == -1 and b"null" in so.nsdp_last_error(), missing
    for missing in ("cano", "bounds"):                                   # (the rule reads them; the mask form does not)
        assert rows(**{missing: None}) == -1 and b"null" in so.nsdp_last_error(), missing
    assert rows(hm=one) == -1 and b"go together" in so.nsdp_last_error()
    assert rows(mm=one) == -1 and b"go together" in so.nsdp_last_error()
    for which in ("cano", "src", "offsets", "bounds", "params", "rows", "tgt"):
        assert rows(**{which: odd}) == -1 and b"aligned" in so.nsdp_last_error(), which
    assert fn(None, None, None, None, None, None, None, 1, 0, None, None, None, None, None) == -1 and b"cap=0" in so.nsdp_last_error()


def test_wrappers_refuse_cpu_tensors():
    from nsdp_amd import pointnet2_utils as pu
    x, offs = torch.zeros(8, 3), torch.tensor([0, 8], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        pu.handle_bounds_ragged(x, offs, 8)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        pu.handle_rows_ragged(x, x, offs, torch.zeros(1, 6), torch.zeros(1, 8, dtype=torch.int32), torch.zeros(8, 7))


# ---------------------------------------------------------------------------------------------------- the command line
def test_cli_flags_parse():
    ap = edit.build_parser()
    a = ap.parse_args(["cfg.yaml"])
    assert a.vertex_counts is None and a.surface_counts is None and edit.counts_from_args(a) == (None, None)
    assert (a.vertices, a.surface, a.batch, a.drags, a.graph) == (25000, None, None, 10, False)      # (the defaults stay)
    a = ap.parse_args(["cfg.yaml", "--vertex-counts", "300,257,640", "--graph"])
    assert edit.counts_from_args(a) == ([300, 257, 640], None) and a.graph
    a = ap.parse_args(["cfg.yaml", "--vertex-counts", "300,257", "--surface-counts", "256,300"])
    assert edit.counts_from_args(a) == ([300, 257], [256, 300])
    a = ap.parse_args(["cfg.yaml", "--vertex-counts", "300,257", "--surface", "256"])
    assert edit.counts_from_args(a) == ([300, 257], None) and a.surface == 256
    for bad in (["--vertex-counts", "300,x"], ["--vertex-counts", "300,0"], ["--surface-counts", "5"],
                ["--vertex-counts", "300,257", "--surface-counts", "256"],
                ["--vertex-counts", "300", "--surface-counts", "256", "--surface", "9"]):
        with pytest.raises(SystemExit):
            edit.counts_from_args(ap.parse_args(["cfg.yaml"] + bad))


# ---------------------------------------------------------------------------------------------------- refusals without a GPU
@pytest.fixture(scope="module")
def flow():
    model, _, _ = build_product(model_cfg("arbitrary", [64, 16, 8]), 5, "cpu")
    return model.eval()


def test_edit_session_names_the_packed_class(flow):
    ragged = RaggedPoints.from_list([torch.zeros(5, 3), torch.zeros(7, 3)])
    with torch.no_grad(), pytest.raises(ValueError, match="ragged inputs: verts_src.*RaggedEditSession"):
        edit.EditSession(flow, ragged)


def test_session_refusals_that_need_no_gpu(flow):
    from nsdp_amd import precision
    S = edit.RaggedEditSession
    verts = RaggedPoints.from_list([torch.zeros(70, 3), torch.zeros(64, 3)])
    with torch.no_grad():
        with pytest.raises(ValueError, match="RaggedEditSession refused: CPU tensors: verts_src"):
            S(flow, verts)
        with pytest.raises(ValueError, match="verts_src must be a RaggedPoints"):
            S(flow, torch.zeros(2, 64, 3))
        flow.train()
        try:
            with pytest.raises(ValueError, match="training mode"):
                S(flow, verts)
        finally:
            flow.eval()
        flow.model_deform.encoder.train()                                   # (one sub-module is enough)
        try:
            with pytest.raises(ValueError, match="training mode"):
                S(flow, verts)
        finally:
            flow.eval()
        with precision.storage(torch.bfloat16):
            with pytest.raises(ValueError, match="bf16 storage"):
                S(flow, _Cuda(verts))
        with pytest.raises(ValueError, match="FlowArbitrary or a Deformation_Networks"):
            S(torch.nn.Linear(3, 3).eval(), verts)
        with pytest.raises(ValueError, match="does not read the handle columns"):
            S(flow.model_canonicalize, _Cuda(verts))
        # what needs only the host's counts and shapes: operands that claim to be on the GPU
        gv = _Cuda(verts)
        with pytest.raises(ValueError, match="an empty shape: shape 1 of verts_src"):
            S(flow, _Cuda(RaggedPoints.from_list([torch.zeros(70, 3), torch.zeros(0, 3)])))
        with pytest.raises(ValueError, match="shape 1 of the cloud has 15 points, fewer than the 16 points the first level samples"):
            S(flow, _Cuda(RaggedPoints.from_list([torch.zeros(70, 3), torch.zeros(15, 3)])))
        with pytest.raises(ValueError, match="shape 0 of the cloud has 12 points, fewer than"):
            S(flow, gv, surface=_Cuda(RaggedPoints.from_list([torch.zeros(12, 3), torch.zeros(64, 3)])))
        with pytest.raises(ValueError, match="cano .* is not over the same layout as verts_src"):
            S(flow, gv, cano=_Cuda(RaggedPoints.from_list([torch.zeros(64, 3), torch.zeros(70, 3)])))
        with pytest.raises(ValueError, match="cano must be a RaggedPoints"):
            S(flow, gv, cano=_CudaTensor(torch.zeros(2, 64, 3)))
        with pytest.raises(ValueError, match="surface_cano goes with a surface"):
            S(flow, gv, surface_cano=gv)
        with pytest.raises(ValueError, match="surface_cano is not over the same layout"):
            S(flow, gv, surface=gv, surface_cano=_CudaTensor(torch.zeros(2, 64, 3)))
        with pytest.raises(ValueError, match="surface holds 3 shapes, verts_src 2"):
            S(flow, gv, surface=_CudaTensor(torch.zeros(3, 64, 3)))
        with pytest.raises(ValueError, match="surface holds 1 shapes, verts_src 2"):
            S(flow, gv, surface=_Cuda(RaggedPoints.from_list([torch.zeros(64, 3)])))
        with pytest.raises(ValueError, match=r"float32 \[B, S, 3\]"):
            S(flow, gv, surface=_CudaTensor(torch.zeros(2, 64, 4)))
    with torch.enable_grad():
        with pytest.raises(ValueError, match="autograd is enabled"):
            S(flow, verts)


def test_session_refuses_pairs_without_geometry():
    """The PointNet++ encoder / interpolation decoder pair (tests/test_alternates.py) searches inside its forward pass."""
    from nsdp_amd.model import build_model
    cfg = {"model": {"type": "forward", "use_normals": False, "encoder": "pointnet++", "decoder": "interp",
                     "encoder_kwargs": {"npoints_per_layer": [256, 64, 16], "nneighbor": 16, "d_transformer": 256,
                                        "nfinal_transformers": 3},
                     "decoder_kwargs": {"dim_inp": 256, "dim": 200, "hidden_dim": 128, "out_dim": 3}}}
    model = build_model(cfg, device="cpu")[0].eval()
    verts = _Cuda(RaggedPoints.from_list([torch.zeros(300, 3), torch.zeros(280, 3)]))
    with torch.no_grad(), pytest.raises(ValueError, match=r"has no geometry\(\)"):
        edit.RaggedEditSession(model, verts)


class _Cuda(RaggedPoints):
    """A packed set on the CPU that answers ``is_cuda`` with True: what the refusals decided on the host alone see of a GPU set
    (ragged_refusal reads counts, shapes and dtypes; it launches nothing and returns before anything would)."""

    def __init__(self, r):
        super().__init__(r.packed, r.offsets, r.counts)

    @property
    def is_cuda(self):
        return True


class _CudaTensor(torch.Tensor):
    """The same for a rectangular tensor."""

    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t)

    @property
    def is_cuda(self):
        return True
