"""The deformation gradient (hip_decoder.decoder_jacobian, include/nsdp_jacobian.h) against the ways to get it without the
kernel, in one process on one GPU.

    python tools/bench_jacobian.py [--reps 7] [--shapes 4x100000,8x8192] [--out profiles/decoder_jacobian.txt]

For every shape B x NQ one JSON line for the DECODER alone (procedural weights, 100 anchors per shape, the neighbour search
included in every partner -- it is part of the call) and one for the full dense-inference STEP (forward model, 2048 surface
samples, ``test_on_batch_with_cano``).  ms per call: median and min-max over interleaved repetitions (forward, jacobian,
six forwards, autograd, forward, ...) of HIP-event windows of several calls, after one untimed call of each:

    forward_ms     hip_decoder.decoder_forward: the plain fused forward (no Jacobian);
    jacobian_ms    hip_decoder.decoder_jacobian: value and Jacobian, one launch;
    six_forward_ms six decoder_forward calls at q +- h e_j: what central differences cost (their result is not usable: a step
                   fp32 can resolve straddles ReLU kinks);
    autograd_ms    three backward passes through the layered training path (torch.autograd.grad of out[..., i].sum()), where
                   its [B, NQ, 8, 200] tensors fit in memory and the path differentiates with respect to the queries; else null
                   with the reason in ``autograd_note``;
    step_ms / step_jacobian_ms   the full step without and with ``jacobian=True``.

The lines are also written to ``--out``.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nsdp_amd import hip_decoder, synth                              # noqa: E402
from nsdp_amd.config import default_config                          # noqa: E402

SHAPES = ((4, 100000), (8, 8192))
ANCHORS, N_SURF = 100, 2048
AUTOGRAD_MAX_BYTES = 64 << 30      # ten [B, NQ, 8, 200] fp32 tensors must fit beside everything else
H = 1e-3


def _window(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def _stats(ts):
    return round(statistics.median(ts), 4), round(min(ts), 4), round(max(ts), 4)


def _interleaved(partners, reps, inner):
    for fn in partners.values():
        fn()                                                             # (the untimed call of each)
    torch.cuda.synchronize()
    times = {k: [] for k in partners}
    for _ in range(reps):
        for k, fn in partners.items():
            times[k].append(_window(fn, inner))
    return {k: _stats(v) for k, v in times.items()}


def _decoder_case(dev, B, NQ, reps):
    from nsdp_amd.model import build_model
    cfg = default_config("forward")
    model, _, _, _ = build_model(cfg, device="cpu")
    dec = model.decoder
    state = synth.procedural_state_dict(dec.state_dict(), 11)
    dec.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    dec = dec.to(dev).eval()
    C = dec.ct1.w_qs.in_features
    t = lambda name, shape, lo=-0.5, hi=0.5: torch.from_numpy(np.ascontiguousarray(synth.uniform(5, name, shape, lo, hi), dtype=np.float32)).to(dev)
    q = t("xyz_q", (B, NQ, 3))
    enc = {"z": 0.5 * torch.from_numpy(np.ascontiguousarray(synth.normal(5, "z", (B, C)), dtype=np.float32)).to(dev),
           "anchors": t("anchors", (B, ANCHORS, 3)),
           "anchor_feats": 0.5 * torch.from_numpy(np.ascontiguousarray(synth.normal(5, "feats", (B, ANCHORS, C)), dtype=np.float32)).to(dev)}
    shifted = [q + s * H * torch.eye(3, device=dev)[j] for j in range(3) for s in (1.0, -1.0)]

    def forward():
        with torch.no_grad():
            return hip_decoder.decoder_forward(dec, q, enc)

    def jacobian():
        with torch.no_grad():
            return hip_decoder.decoder_jacobian(dec, q, enc)

    def six_forward():
        with torch.no_grad():
            return [hip_decoder.decoder_forward(dec, s, enc) for s in shifted]

    def autograd():
        with torch.enable_grad():
            x = q.detach().clone().requires_grad_(True)
            out = dec(x, enc)
            return [torch.autograd.grad(out[..., i].sum(), x, retain_graph=i < 2)[0] for i in range(3)]

    partners = {"forward": forward, "jacobian": jacobian, "six_forward": six_forward}
    note = None
    need = 10 * B * NQ * 8 * 200 * 4
    if need > AUTOGRAD_MAX_BYTES:
        note = f"ten [B, NQ, 8, 200] fp32 tensors = {need / 2**30:.1f} GiB: not attempted"
    else:
        try:
            rows = autograd()
            if any(r is None for r in rows):
                raise RuntimeError("no gradient with respect to the queries")
            partners["autograd"] = autograd
            del rows
        except Exception as e:                                           # (recorded, not hidden: the line says why there is no figure)
            note = f"{type(e).__name__}: {str(e).splitlines()[0][:160]}"
            torch.cuda.empty_cache()
    out, jac = jacobian()
    equal = bool(torch.equal(out, forward()))
    inner = 3 if B * NQ >= 200000 else 10
    st = _interleaved(partners, reps, inner)
    rec = {"case": "decoder", "B": B, "NQ": NQ, "anchors": ANCHORS, "calls_per_window": inner, "reps": reps,
           "out_equal_to_forward": equal, "jacobian_finite": bool(torch.isfinite(jac).all())}
    for k in ("forward", "jacobian", "six_forward", "autograd"):
        rec[k + "_ms"], rec[k + "_min"], rec[k + "_max"] = st.get(k, (None, None, None))
    rec["autograd_note"] = note
    rec["jacobian_over_forward"] = round(rec["jacobian_ms"] / rec["forward_ms"], 2)
    rec["six_forward_over_jacobian"] = round(rec["six_forward_ms"] / rec["jacobian_ms"], 2)
    if rec["autograd_ms"] is not None:
        rec["autograd_over_jacobian"] = round(rec["autograd_ms"] / rec["jacobian_ms"], 2)
    return rec


def _step_case(dev, B, NQ, reps):
    from nsdp_amd.model import build_model
    from nsdp_amd.model.deformation_networks import test_on_batch_with_cano
    cfg = default_config("forward")
    levels = cfg["model"]["encoder_kwargs"]["npoints_per_layer"]
    cfg["model"]["encoder_kwargs"]["npoints_per_layer"] = [min(int(p), N_SURF) for p in levels]
    model, _, _, _ = build_model(cfg, device="cpu")
    state = synth.procedural_state_dict(model.state_dict(), 2048)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    model = model.to(dev).eval()
    data = synth.make_batch(1000, B, N_SURF, NQ)
    dd = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in data.items()}
    dd["surface_samples_src"] = dd["surface_samples_inputs"][:, :, 0:3].contiguous()
    dd["verts_src"] = dd.pop("space_samples_src")
    dd.pop("space_samples_tgt")
    plain, withj = dict(dd), dict(dd)
    partners = {"step": lambda: test_on_batch_with_cano(model, plain, cfg),
                "step_jacobian": lambda: test_on_batch_with_cano(model, withj, cfg, jacobian=True)}
    inner = 3 if B * NQ >= 200000 else 10
    st = _interleaved(partners, reps, inner)
    from nsdp_amd import deformation_gradient as dg
    det = dg.determinant(withj["verts_tgt_jacobian"])
    rec = {"case": "step", "B": B, "NQ": NQ, "surface": N_SURF, "calls_per_window": inner, "reps": reps,
           "verts_equal_to_plain": bool(torch.equal(plain["verts_tgt_pred"], withj["verts_tgt_pred"])),
           "fold_overs": dg.fold_overs(withj["verts_tgt_jacobian"]).tolist(), "det_median": float(det.median())}
    for k in ("step", "step_jacobian"):
        rec[k + "_ms"], rec[k + "_min"], rec[k + "_max"] = st[k]
    rec["step_jacobian_over_step"] = round(rec["step_jacobian_ms"] / rec["step_ms"], 2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default=",".join(f"{b}x{n}" for b, n in SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decoder_jacobian.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    shapes = [tuple(int(x) for x in s.split("x")) for s in args.shapes.split(",")]
    lines = [json.dumps({"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip})]
    print(lines[0], flush=True)
    for B, NQ in shapes:
        for case in (_decoder_case, _step_case):
            lines.append(json.dumps(case(dev, B, NQ, args.reps)))
            print(lines[-1], flush=True)
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
