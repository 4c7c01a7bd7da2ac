"""Builds libnsdp_hip.so (hand-written HIP for gfx950) in-tree with hipcc.  No torch extension
machinery, no hipify: plain `hipcc --offload-arch=gfx950` per translation unit, then one shared link.

    python -m nsdp_amd.build [--force]
"""
from __future__ import annotations

import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
OBJDIR = os.path.join(LIBDIR, "obj")
SO = os.path.join(LIBDIR, "libnsdp_hip.so")
HEADER = os.path.join(os.path.dirname(HERE), "include", "nsdp_hip.h")
EVAL_HEADER = os.path.join(os.path.dirname(HERE), "include", "nsdp_eval.h")
SAMPLING_HEADER = os.path.join(os.path.dirname(HERE), "include", "nsdp_sampling.h")
SEARCH_HEADER = os.path.join(os.path.dirname(HERE), "include", "nsdp_search.h")
SCATTER_HEADER = os.path.join(os.path.dirname(HERE), "include", "nsdp_scatter.h")
HANDLES_HEADER = os.path.join(os.path.dirname(HERE), "include", "nsdp_handles.h")
HANDLES_RAGGED_HEADER = os.path.join(os.path.dirname(HERE), "include", "nsdp_handles_ragged.h")
HANDLE_SETS_HEADER = os.path.join(os.path.dirname(HERE), "include", "nsdp_handle_sets.h")
CHAMFER_HEADER = os.path.join(os.path.dirname(HERE), "include", "nsdp_chamfer.h")
JACOBIAN_HEADER = os.path.join(os.path.dirname(HERE), "include", "nsdp_jacobian.h")
RIGIDITY_HEADER = os.path.join(os.path.dirname(HERE), "include", "nsdp_rigidity.h")
SURFACE_HEADER = os.path.join(os.path.dirname(HERE), "include", "nsdp_surface.h")
BATCH_HEADER = os.path.join(os.path.dirname(HERE), "include", "nsdp_batch.h")
MESHBATCH_HEADER = os.path.join(os.path.dirname(HERE), "include", "nsdp_meshbatch.h")
MESHWHOLE_HEADER = os.path.join(os.path.dirname(HERE), "include", "nsdp_meshwhole.h")
OPTIM_HEADER = os.path.join(os.path.dirname(HERE), "include", "nsdp_optim.h")
MESHNORMALS_HEADER = os.path.join(os.path.dirname(HERE), "include", "nsdp_meshnormals.h")
SELFINTERSECT_HEADER = os.path.join(os.path.dirname(HERE), "include", "nsdp_selfintersect.h")
RAYCAST_HEADER = os.path.join(os.path.dirname(HERE), "include", "nsdp_raycast.h")
GEODESIC_HEADER = os.path.join(os.path.dirname(HERE), "include", "nsdp_geodesic.h")
RASTER_HEADER = os.path.join(os.path.dirname(HERE), "include", "nsdp_raster.h")

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# -munsafe-fp-atomics: fp32 atomicAdd lowers to the hardware global_atomic_add_f32 instead of a CAS loop
# (all buffers are ordinary coarse-grained device allocations)
COMMON = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function",
          "-munsafe-fp-atomics"]
# geometry kernels must keep one rounding per fp32 op (bit-exact distances): contraction off
EXACT = ["-ffp-contract=off"]
FAST = ["-ffp-contract=fast"]
PER_FILE = {
    "fps.hip": EXACT,
    "fps_cluster.hip": EXACT,                   # (the keys of fps.hip: the same distance bits)
    "knn.hip": EXACT,
    "knn_grid.hip": EXACT,                      # (the distances of knn.hip: the same bits)
    "invert_wide.hip": EXACT,                   # (integer work only)
    "handles.hip": EXACT,                       # (the handle rule and src + d * m: one rounding per operation)
    "handles_ragged.hip": EXACT,                # (handles.hip's arithmetic over packed rows: the same bits)
    "handle_sets.hip": EXACT,                   # (motions as literal products and sums: one rounding per operation)
    "eval_metric.hip": EXACT,                   # (nn_dist2 must give nsdp_knn's distance bits)
    "chamfer.hip": EXACT,                       # (the gradient's documented operation order: one rounding per operation)
    "rigidity.hip": EXACT,                      # (squared lengths with nsdp_knn's bits; the gradient's documented operation order)
    "surface_distance.hip": EXACT,              # (the point-to-triangle distance's documented operation order)
    "batch_assemble.hip": EXACT,                # (src + level * noise and the handle rule: one rounding per operation)
    "mesh_sample.hip": EXACT,                   # (the sampling rule of nsdp_meshbatch.h: one rounding per operation, exact sqrt and /)
    "mesh_whole.hip": EXACT,                    # (the handle rule and the input row of batch_rows.h: mesh_sample.hip's bits)
    "mesh_normals.hip": EXACT,                  # (the rule of nsdp_meshnormals.h: one rounding per operation, exact sqrt and /)
    "self_intersect.hip": EXACT,                # (the rule of nsdp_selfintersect.h: the signs of determinants, one rounding per operation)
    "ray_cast.hip": EXACT,                      # (the rule of nsdp_raycast.h: fp32 shear, exact fp64 edge signs, one rounding per operation)
    "geodesic.hip": EXACT,                      # (the rule of nsdp_geodesic.h: edge lengths and path sums, one rounding per operation, exact sqrt)
    "rasterize.hip": EXACT,                     # (the rule of nsdp_raster.h: fp32 corners, exact integer edge signs in fp64, one rounding per operation)
    "pointnet2_ops.hip": EXACT,
    # torch's single-tensor Adam rounds once per operation: no fused multiply-adds in the optimizer kernel (nor in the
    # gradient-norm kernels of nsdp_optim.h, which live beside it and share its chunk loop)
    "adam.hip": EXACT,
    # -O3 turns the uniform base pointers of this file's hand-placed `global_load ... s[base]` asm operands into
    # VGPR copies (rejected by the assembler); -O2 keeps them scalar
    "wgrad_bf16x3.hip": FAST + ["-O2", "-fno-slp-vectorize"],
    # packed fp32 VALU (v_pk_add_f32 / v_pk_mul_f32, what the SLP vectorizer makes of the activation split's adjacent scalar
    # subtractions) costs more issue time beside MFMAs than the two scalar operations it replaces (MI355X_MICROARCH.md): without
    # it the forward / dX GEMMs run 0.5-3 % faster alone and the B = 32 step 0.26 ms (three interleaved rounds), bit-identical
    "gemm_bf16x3.hip": FAST + ["-fno-slp-vectorize"],
    "gemm_bf16x3_g16.hip": FAST + ["-fno-slp-vectorize"],      # (the same kernel template, x3_kernel.h: its G16-layout instantiations)
}


def sources():
    return sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))


def _deps_mtime():
    # (this file too: the compiler flags live here)
    hs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")] + [HEADER, EVAL_HEADER, SAMPLING_HEADER, SEARCH_HEADER, SCATTER_HEADER, HANDLES_HEADER, HANDLES_RAGGED_HEADER, HANDLE_SETS_HEADER, CHAMFER_HEADER, JACOBIAN_HEADER, RIGIDITY_HEADER, SURFACE_HEADER, BATCH_HEADER, MESHBATCH_HEADER, MESHWHOLE_HEADER, OPTIM_HEADER, MESHNORMALS_HEADER, SELFINTERSECT_HEADER, RAYCAST_HEADER, GEODESIC_HEADER, RASTER_HEADER, os.path.abspath(__file__)]
    return max(os.path.getmtime(h) for h in hs)


def _compile(src, force):
    obj = os.path.join(OBJDIR, src[:-4] + ".o")
    path = os.path.join(CSRC, src)
    if (not force and os.path.exists(obj)
            and os.path.getmtime(obj) >= max(os.path.getmtime(path), _deps_mtime())):
        return obj, False
    cmd = [HIPCC] + COMMON + PER_FILE.get(src, FAST) + ["-c", path, "-o", obj]
    subprocess.check_call(cmd)
    return obj, True


def build(force: bool = False, verbose: bool = False) -> str:
    os.makedirs(OBJDIR, exist_ok=True)
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        results = list(ex.map(lambda s: _compile(s, force), sources()))
    objs = [o for o, _ in results]
    if force or any(c for _, c in results) or not os.path.exists(SO):
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", SO] + objs)
        if verbose:
            print("linked", SO)
    return SO


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
