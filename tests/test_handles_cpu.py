"""CPU: the boundary of the user-handle entries and of the editing session -- include/nsdp_handles.h declares the three entries
and the built library exports them at ABI version 15, outside nsdp_hip.h's table; bad arguments come back as a status with a
message before anything is touched; HandleSpec.from_config follows the reference's if / elif priority and reads its YAML data
blocks (tests/golden/userhandle_configs.json: the `data` settings of config/tosca/*.yaml and config/dogrec/*.yaml); the command
line parses; and the session names each refusal that needs no GPU."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from helpers import build_product, model_cfg
from nsdp_amd import _lib, build as nsdp_build, edit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nsdp_handles.h")
ENTRY_POINTS = ["nsdp_handle_bounds", "nsdp_handle_bounds_workspace_bytes", "nsdp_handle_rows"]
GOLDEN = os.path.join(ROOT, "tests", "golden", "userhandle_configs.json")


@pytest.fixture(scope="module")
def so():
    if not os.path.exists(_lib.SO_PATH):
        nsdp_build.build()
    lib = ctypes.CDLL(_lib.SO_PATH)
    lib.nsdp_last_error.restype = ctypes.c_char_p
    lib.nsdp_handle_bounds_workspace_bytes.restype = ctypes.c_size_t
    return lib


def test_header_declares_and_library_exports_the_entries(so):
    with open(HEADER) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(nsdp_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(ENTRY_POINTS)
    for name in ENTRY_POINTS:
        assert hasattr(so, name), name
    assert so.nsdp_abi_version() >= 15
    assert not set(ENTRY_POINTS) & set(_lib.declared_symbols())          # (nsdp_hip.h keeps its own table of entries)
    assert os.path.basename(HEADER) in open(nsdp_build.__file__).read()
    assert nsdp_build.HANDLES_HEADER == HEADER
    assert nsdp_build.PER_FILE["handles.hip"] == nsdp_build.EXACT


def test_header_constants_mirror_the_python_side():
    from nsdp_amd import pointnet2_utils as pu
    text = open(HEADER).read()
    for i, part in enumerate(edit.PARTS):
        assert re.search(rf"NSDP_HANDLE_{part.upper()} = {i}\b", text), part
    assert pu.HANDLE_PARTS == edit.PARTS
    assert f"NSDP_HANDLE_PARAM_WORDS = {pu.HANDLE_PARAM_WORDS}" in text
    source = open(os.path.join(ROOT, "nsdp_amd", "csrc", "handles_rule.h")).read()      # (the limit of both layouts)
    assert "kMaxPoints = 1 << 20;" in source and pu.HANDLE_MAX_POINTS == 1 << 20


def test_workspace_bytes_refuses_what_the_entry_refuses(so):
    ws = so.nsdp_handle_bounds_workspace_bytes
    assert ws(0, 100) == 0 and ws(65536, 100) == 0 and ws(-1, 100) == 0
    assert ws(1, 0) == 0 and ws(1, -5) == 0 and ws(1, (1 << 20) + 1) == 0
    assert ws(1, 1) > 0 and ws(65535, 1) > 0 and ws(1, 1 << 20) > 0
    assert ws(1, 1) % 4 == 0 and ws(3, 1025) % 4 == 0
    sizes = [ws(2, n) for n in (1, 63, 4096, 4097, 100000, 1 << 20)]
    assert sizes == sorted(sizes) and sizes[0] < sizes[-1]
    assert ws(1, 1 << 20) == 256 * 6 * 4                                 # 256 workgroups' partials of six words
    assert ws(65535, 1 << 20) == 65535 * ws(1, 1 << 20)


def test_bad_arguments_return_status(so):
    one = ctypes.c_void_p(16)      # (a non-null pointer the library must not touch before it has checked everything)
    odd = ctypes.c_void_p(18)
    fn = so.nsdp_handle_bounds
    # (cano, B, n, workspace, bounds, stream)
    assert fn(one, 0, 4, one, one, None) == -1 and b"batch" in so.nsdp_last_error()
    assert fn(one, 65536, 4, one, one, None) == -1 and b"batch" in so.nsdp_last_error()
    assert fn(one, 1, 0, one, one, None) == -1 and b"n=0" in so.nsdp_last_error()
    assert fn(one, 1, (1 << 20) + 1, one, one, None) == -1 and b"n=1048577" in so.nsdp_last_error()
    assert fn(None, 1, 4, one, one, None) == -1 and b"null" in so.nsdp_last_error()
    assert fn(one, 1, 4, None, one, None) == -1 and b"null" in so.nsdp_last_error()
    assert fn(one, 1, 4, one, None, None) == -1 and b"null" in so.nsdp_last_error()
    assert fn(odd, 1, 4, one, one, None) == -1 and b"aligned" in so.nsdp_last_error()
    assert fn(one, 1, 4, odd, one, None) == -1 and b"aligned" in so.nsdp_last_error()
    assert fn(one, 1, 4, one, odd, None) == -1 and b"aligned" in so.nsdp_last_error()
    fn = so.nsdp_handle_rows
    # (cano, src, bounds, params, handle_mask, move_mask, B, n, rows, tgt, handle_out, move_out, stream)
    ok = dict(cano=one, src=one, bounds=one, params=one, hm=None, mm=None, B=1, n=4, rows=one, tgt=one, ho=one, mo=one)

    def call(**kw):
        a = dict(ok, **kw)
        return fn(a["cano"], a["src"], a["bounds"], a["params"], a["hm"], a["mm"], a["B"], a["n"], a["rows"], a["tgt"], a["ho"],
                  a["mo"], None)

    assert call(B=0) == -1 and b"batch" in so.nsdp_last_error()
    assert call(B=65536) == -1 and b"batch" in so.nsdp_last_error()
    assert call(n=0) == -1 and b"n=0" in so.nsdp_last_error()
    assert call(n=(1 << 20) + 1) == -1 and b"n=1048577" in so.nsdp_last_error()
    for missing in ("src", "params", "rows"):
        assert call(**{missing: None}) == -1 and b"null" in so.nsdp_last_error(), missing
    for missing in ("cano", "bounds"):                                   # (the rule reads them; the mask form does not)
        assert call(**{missing: None}) == -1 and b"null" in so.nsdp_last_error(), missing
    assert call(hm=one) == -1 and b"go together" in so.nsdp_last_error()
    assert call(mm=one) == -1 and b"go together" in so.nsdp_last_error()
    for which in ("cano", "src", "bounds", "params", "rows", "tgt"):
        assert call(**{which: odd}) == -1 and b"aligned" in so.nsdp_last_error(), which
    # sizes are judged before pointers: a refused size with every pointer null names the size
    assert fn(None, None, None, None, None, None, 1, 0, None, None, None, None, None) == -1 and b"n=0" in so.nsdp_last_error()


def test_wrappers_refuse_cpu_tensors():
    from nsdp_amd import pointnet2_utils as pu
    x = torch.zeros(1, 8, 3)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        pu.handle_bounds(x)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        pu.handle_rows(x, x, torch.zeros(1, 6), torch.zeros(1, 8, dtype=torch.int32), torch.zeros(1, 8, 7))


# ---------------------------------------------------------------------------------------------------- HandleSpec
def _data(**flags):
    uh = {"cliptail": False, **{p: False for p in edit.PARTS}, "xtrans": 0.1, "ytrans": -0.2, "ztrans": 0.3}
    uh.update(flags)
    return {"partial_range": 0.1, "userhandle": uh}


def test_from_config_follows_the_reference_priority():
    for i, part in enumerate(edit.PARTS):
        assert edit.HandleSpec.from_config(_data(**{part: True})).part == part
        later = {p: True for p in edit.PARTS[i:]}                        # every later flag set as well: the first one wins
        assert edit.HandleSpec.from_config(_data(**later)).part == part
    spec = edit.HandleSpec.from_config(_data(tail=True, cliptail=True))
    assert spec == edit.HandleSpec("tail", (0.1, -0.2, 0.3), 0.1, True)
    d = _data(head=True)
    d["partial_range"] = 0.25
    assert edit.HandleSpec.from_config(d).partial_range == 0.25


def test_from_config_without_a_part_is_a_value_error():
    with pytest.raises(ValueError, match="none of"):
        edit.HandleSpec.from_config(_data())
    with pytest.raises(ValueError, match="userhandle"):
        edit.HandleSpec.from_config({"partial_range": 0.1})
    with pytest.raises(ValueError, match="part must be one of"):
        edit.HandleSpec("nose", (0, 0, 0))


def test_from_config_reads_the_reference_data_blocks():
    with open(GOLDEN) as f:
        blocks = json.load(f)
    assert sorted(blocks) == sorted(f"{d}/{p}" for d in ("tosca", "dogrec") for p in ("head", "tail", "frontleftfoot", "behindrightfoot"))
    want = {"head": (-0.15, -0.20, -0.20), "tail": (-0.15, 0.15, -0.15), "frontleftfoot": (0.15, -0.20, 0.20),
            "behindrightfoot": (-0.15, -0.20, 0.20)}
    for name, data in blocks.items():
        spec = edit.HandleSpec.from_config(data)
        part = name.split("/")[1]
        assert spec.part == part and spec.translation == want[part], name
        assert spec.partial_range == 0.1 and spec.cliptail is False


def test_pack_params_layout():
    w = edit.pack_params(2, ["tail", "behindrightfoot"], [(0.5, -0.0, 1.5), (2.0, 3.0, 4.0)], 0.1, [True, False])
    assert w.dtype == np.int32 and w.shape == (2, 8)
    assert w[:, 0].tolist() == [1, 5] and w[:, 1].tolist() == [1, 0] and not w[:, 6:].any()
    f = w.view(np.float32)
    assert f[0, 2] == np.float32(0.1) and f[:, 3:6].tolist() == [[0.5, -0.0, 1.5], [2.0, 3.0, 4.0]]
    assert np.signbit(f[0, 4])                                            # (the sign of a zero translation travels)
    assert edit.pack_params(3, "head", (1, 2, 3), 0.2, False)[:, 0].tolist() == [0, 0, 0]
    for bad in (dict(part="nose"), dict(part=["head"]), dict(part=6), dict(translation=(1, 2))):
        args = dict(part="head", translation=(0, 0, 0))
        args.update(bad)
        with pytest.raises(ValueError):
            edit.pack_params(2, args["part"], args["translation"], 0.1, False)


# ---------------------------------------------------------------------------------------------------- the command line
def test_cli_argument_parsing():
    ap = edit.build_parser()
    a = ap.parse_args(["cfg.yaml"])
    assert (a.config_file, a.vertices, a.surface, a.batch, a.part, a.translate, a.drags, a.graph, a.weight_file, a.out) == \
        ("cfg.yaml", 25000, None, None, None, None, 10, False, None, None)
    a = ap.parse_args(["cfg.yaml", "--vertices", "5000", "--surface", "2048", "--batch", "2", "--part", "tail", "--translate",
                       "0.1,-0.2,0.3", "--drags", "4", "--graph", "--weight_file", "w.pt", "--out", "o"])
    assert (a.vertices, a.surface, a.batch, a.part, a.translate, a.drags, a.graph, a.weight_file, a.out) == \
        (5000, 2048, 2, "tail", "0.1,-0.2,0.3", 4, True, "w.pt", "o")
    with pytest.raises(SystemExit):
        ap.parse_args(["cfg.yaml", "--part", "nose"])
    # the drag of the command line: the flags over the config's data.userhandle, head.yaml's drag without either
    cfg = {"data": _data(frontrightfoot=True, cliptail=True)}
    assert edit.spec_from_args(ap.parse_args(["c"]), cfg) == edit.HandleSpec("frontrightfoot", (0.1, -0.2, 0.3), 0.1, True)
    assert edit.spec_from_args(a, cfg) == edit.HandleSpec("tail", (0.1, -0.2, 0.3), 0.1, True)
    assert edit.spec_from_args(ap.parse_args(["c"]), {"model": {}}) == edit.HandleSpec("head", (-0.15, -0.2, -0.2), 0.1, False)
    with pytest.raises(SystemExit):
        edit.spec_from_args(ap.parse_args(["c", "--translate", "1,2"]), cfg)


# ---------------------------------------------------------------------------------------------------- refusals without a GPU
@pytest.fixture(scope="module")
def flow():
    model, _, _ = build_product(model_cfg("arbitrary", [64, 16, 8]), 5, "cpu")
    return model.eval()


def test_session_refusals_that_need_no_gpu(flow):
    from nsdp_amd import precision
    from nsdp_amd.ragged import RaggedPoints
    verts = torch.zeros(1, 64, 3)
    with torch.no_grad():
        with pytest.raises(ValueError, match="CPU tensors"):
            edit.EditSession(flow, verts)
        with pytest.raises(ValueError, match="CPU tensors: verts_src"):
            edit.EditSession(flow, verts, surface=torch.zeros(1, 32, 3))
        flow.train()
        try:
            with pytest.raises(ValueError, match="training mode"):
                edit.EditSession(flow, verts)
        finally:
            flow.eval()
        flow.model_deform.encoder.train()                                   # (one sub-module is enough)
        try:
            with pytest.raises(ValueError, match="training mode"):
                edit.EditSession(flow, verts)
        finally:
            flow.eval()
        ragged = RaggedPoints.from_list([torch.zeros(5, 3), torch.zeros(7, 3)])
        with pytest.raises(ValueError, match="ragged inputs: verts_src"):
            edit.EditSession(flow, ragged)
        with pytest.raises(ValueError, match="ragged inputs: surface"):
            edit.EditSession(flow, verts, surface=ragged)
        with precision.storage(torch.bfloat16):
            with pytest.raises(ValueError, match="bf16 storage"):
                edit.EditSession(flow, verts)
        with pytest.raises(ValueError, match="FlowArbitrary or a Deformation_Networks"):
            edit.EditSession(torch.nn.Linear(3, 3).eval(), verts)
        with pytest.raises(ValueError, match="does not read the handle columns"):
            edit.EditSession(flow.model_canonicalize, verts)
        with pytest.raises(ValueError, match=r"float32 \[B, n, 3\]"):
            edit.EditSession(flow, torch.zeros(1, 64, 4))
    with torch.enable_grad():
        with pytest.raises(ValueError, match="autograd is enabled"):
            edit.EditSession(flow, verts)


def test_session_refuses_pairs_without_geometry():
    """The PointNet++ encoder / interpolation decoder pair (tests/test_alternates.py) searches inside its forward pass."""
    from nsdp_amd.model import build_model
    cfg = {"model": {"type": "forward", "use_normals": False, "encoder": "pointnet++", "decoder": "interp",
                     "encoder_kwargs": {"npoints_per_layer": [256, 64, 16], "nneighbor": 16, "d_transformer": 256,
                                        "nfinal_transformers": 3},
                     "decoder_kwargs": {"dim_inp": 256, "dim": 200, "hidden_dim": 128, "out_dim": 3}}}
    model = build_model(cfg, device="cpu")[0].eval()
    with torch.no_grad(), pytest.raises(ValueError, match=r"has no geometry\(\)"):
        edit.EditSession(model, torch.zeros(1, 64, 3))
