"""GPU: nsdp_mesh_rasterize (include/nsdp_raster.h) against tests/raster_ref.py, byte for byte, at the smallest shapes where
the kernels can go wrong -- images of one pixel, of one partial tile, of partial tiles in both directions and of several tiles;
meshes on both sides of a block of 64 faces and of the 256-box vote of a tile; a face larger than the image, one wholly off
screen, a degenerate one, one with a corner behind the camera plane (dropped and counted); a mesh without faces; several images
of several meshes in a shuffled image_shape; both flags; bary and count NULL and non-NULL; capacities beyond the last offsets --
then the three Python layouts against each other, the reordered plan against the given order, and the cross-check with the ray
cast: on a grid-aligned closed mesh under an orthographic camera the number of covering faces IS the number of crossings of the
pixel's ray, ties included."""
import numpy as np
import pytest
import torch

import ray_cast_ref as rr
import raster_ref as ra

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
f32 = np.float32


def _scene(F, H, W, seed):
    """Three meshes packed with padding rows, four images in a shuffled image_shape -> the operands of the entry (numpy)."""
    rng = np.random.default_rng(seed)
    V = max(4, F // 2 + 3)
    v0 = rng.uniform(-1, 1, (V, 3)).astype(f32)
    f0 = rng.integers(0, V, (F, 3))
    extra_v = f32([[-50, -50, 0.5], [50, -50, 0.5], [0, 60, 0.75],          # larger than every image
                   [30, 30, 0], [31, 30, 0], [30, 31, 0],                   # wholly off screen
                   [0, 0, -10]])                                            # behind the camera plane of the pinholes (W = -7)
    extra_f = np.array([[V, V + 1, V + 2], [V + 3, V + 4, V + 5], [0, 0, 1], [V + 6, 0, 1]])
    if F == 1:
        v0[:3] = f32([[-0.9, -0.8, 0.1], [0.8, -0.7, -0.2], [0.1, 0.9, 0.3]])
        f0[0] = (0, 1, 2)
    vc, fc = ra.cube()
    meshes = [(np.concatenate([v0, extra_v]), np.concatenate([f0, extra_f])), (vc * f32(0.5), fc),
              (rng.uniform(-1, 1, (4, 3)).astype(f32), np.zeros((0, 3), np.int64))]
    focal = 0.8 * max(min(H, W), 2)
    cams = np.stack([ra.ortho(8, W / 2, H / 2, 4),                          # the cube, its corners on or between centres
                     ra.pinhole(focal, W / 2, H / 2, 3),                    # the mesh without faces
                     ra.pinhole(focal, W / 2 + 0.25, H / 2 - 0.125, 3),     # the random mesh
                     ra.pinhole(2 * focal, W / 2, H / 2, 2.5)])             # the cube again, closer
    shape = np.array([1, 2, 0, 1], np.int32)
    pad = 5
    verts = np.concatenate([m[0] for m in meshes] + [np.full((pad, 3), np.nan, f32)])
    faces = np.concatenate([m[1] for m in meshes] + [np.full((pad, 3), -1)]).astype(np.int32)
    voff = np.cumsum([0] + [len(m[0]) for m in meshes]).astype(np.int32)
    foff = np.cumsum([0] + [len(m[1]) for m in meshes]).astype(np.int32)
    return verts, voff, faces, foff, cams.reshape(-1, 16), shape


def _call(scene, H, W, flags, with_bary, with_count):
    from nsdp_amd import rasterize as rz
    verts, voff, faces, foff, cams, shape = [torch.tensor(a).to(DEV) for a in scene]
    return rz.mesh_rasterize(verts, voff, faces, foff, cams, shape, H, W, with_bary, with_count, flags)


def _same_bytes(got, want, with_bary, with_count):
    depth, face, bary, count, dropped = got
    assert np.array_equal(depth.cpu().numpy().view(np.uint32), want["depth"].view(np.uint32))
    assert np.array_equal(face.cpu().numpy(), want["face"])
    assert np.array_equal(dropped.cpu().numpy(), want["dropped"])
    assert (bary is None) == (not with_bary) and (count is None) == (not with_count)
    if with_bary:
        assert np.array_equal(bary.cpu().numpy().view(np.uint32), want["bary"].view(np.uint32))
    if with_count:
        assert np.array_equal(count.cpu().numpy(), want["count"])


SHAPES = [(1, 1, 1), (8, 8, 63), (33, 17, 65), (64, 48, 129), (17, 33, 1), (8, 8, 129), (33, 17, 64 * 256 + 1)]


@pytest.mark.parametrize("H,W,F", SHAPES)
def test_every_output_equals_the_emulation(H, W, F):
    scene = _scene(F, H, W, 7 * F + H)
    for flags, with_bary, with_count in ((0, True, True), (ra.FRONT_ONLY, False, False), (ra.FRONT_ONLY, True, False), (0, False, True)):
        want = ra.rasterize(scene[0], scene[1], scene[2], scene[3], scene[4], scene[5], H, W, flags)
        if flags == 0:
            assert want["dropped"].tolist() == [0, 0, 1, 0] and (want["face"][1] == -1).all()
            if H * W > 1:
                assert (want["count"][2] > 0).sum() >= H * W // 2 and (want["face"][0] >= 0).any()      # the large face covers
        _same_bytes(_call(scene, H, W, flags, with_bary, with_count), want, with_bary, with_count)


def test_two_runs_give_equal_bytes():
    scene = _scene(129, 64, 48, 5)
    a, b = _call(scene, 64, 48, 0, True, True), _call(scene, 64, 48, 0, True, True)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_limits_and_layouts_are_refused_by_name():
    from nsdp_amd import rasterize as rz
    v, f = ra.cube()
    tv, tf = torch.tensor(v).to(DEV), torch.tensor(f).to(DEV)
    plan = rz.RasterPlan(tf, tv)
    cam = torch.tensor(ra.ortho(8, 16.5, 16.5, 4)).to(DEV).reshape(1, 4, 4)
    for args, word in (((tv.cpu(), plan, cam, 8, 8), "CPU tensors"), ((tv.bfloat16(), plan, cam, 8, 8), "dtype"),
                       ((tv, plan, cam, 0, 8), "limits"), ((tv, plan, cam, 8, 4097), "limits"), ((tv, plan, cam.reshape(4, 4), 8, 8), "shape"),
                       ((tv, plan, cam.expand(3, 1, 4, 4), 8, 8), "shape"), ((tv, object(), cam, 8, 8), "RasterPlan"),
                       ((tv[:5], plan, cam, 8, 8), "topology")):
        with pytest.raises(rz.RasterError, match=word):
            rz.rasterize(*args)
    with pytest.raises(rz.RasterError, match="limits"):
        rz.rasterize(tv, plan, cam.expand(128, 4, 4), 4096, 4096)           # 2^31 pixels


def _noisy_sphere(seed):
    v, f = ra.uv_sphere()
    rng = np.random.default_rng(seed)
    return (v + rng.normal(0, 0.01, v.shape)).astype(f32), f


def test_three_layouts_and_the_reordered_plan_agree():
    """Two poses of one topology as shared faces, as faces of their own and as packed meshes; each through the Morton-ordered
    plan and through the given order: equal bytes in the caller's numbering (the emulation finds no two covering faces with equal
    depth bits at a pixel of this scene, so the order of the visit cannot show)."""
    from nsdp_amd import rasterize as rz
    from nsdp_amd.ragged import RaggedPoints
    H, W = 48, 64
    (va, f), (vb, _) = _noisy_sphere(1), _noisy_sphere(2)
    cams = [rz.Camera.look_at((2.5, 1.5, -3), (0, 0, 0), (0, 1, 0), 35, W, H), rz.Camera.orthographic((0, 3, 0.5), (0, 0, 0), (0, 0, 1), 2.5, W, H)]
    want = [[ra.image(v, f, c.matrix, H, W) for c in cams] for v in (va, vb)]
    for per_pose in want:
        for r in per_pose:
            hit = r["face"] >= 0
            assert hit.sum() > H * W // 6 and (r["second"][hit] != r["depth"][hit]).all() and r["dropped"] == 0
    tf = torch.tensor(f).to(DEV)
    poses = torch.tensor(np.stack([va, vb])).to(DEV)                       # [2, V, 3]
    packed = RaggedPoints.from_list([poses[0], poses[1]])
    layouts = {"shared": (tf, poses), "batched": (tf.unsqueeze(0).expand(2, -1, -1).contiguous(), poses),
               "ragged": (RaggedPoints.from_list([tf, tf]), packed)}
    for name, (faces, verts) in layouts.items():
        for reorder in (True, False):
            plan = rz.RasterPlan(faces, verts, reorder=reorder)
            got = rz.rasterize(verts, plan, cams, H, W, count=True)
            assert tuple(got.depth.shape) == (2, 2, H, W) and tuple(got.bary.shape) == (2, 2, H, W, 3) and tuple(got.dropped.shape) == (2, 2)
            for p in range(2):
                for k in range(2):
                    r = want[p][k]
                    assert np.array_equal(got.depth[p, k].cpu().numpy().view(np.uint32), r["depth"].view(np.uint32)), (name, reorder, p, k)
                    assert np.array_equal(got.face[p, k].cpu().numpy(), r["face"]) and np.array_equal(got.count[p, k].cpu().numpy(), r["count"])
                    assert np.array_equal(got.bary[p, k].cpu().numpy().view(np.uint32), r["bary"].view(np.uint32))
                    assert np.array_equal(got.hit[p, k].cpu().numpy(), r["face"] >= 0) and int(got.dropped[p, k]) == 0
    # views of their own per mesh: [2, K, 4, 4]
    own = torch.tensor(np.stack([[cams[0].matrix, cams[1].matrix], [cams[1].matrix, cams[0].matrix]])).to(DEV)
    got = rz.rasterize(poses, rz.RasterPlan(tf, poses), own, H, W, return_bary=False)
    assert got.bary is None and got.count is None
    assert np.array_equal(got.face[1, 0].cpu().numpy(), want[1][1]["face"]) and np.array_equal(got.face[1, 1].cpu().numpy(), want[1][0]["face"])


def test_interpolate_and_shade():
    from nsdp_amd import rasterize as rz
    from nsdp_amd.mesh_normals import vertex_normals
    H, W = 40, 40
    v, f = ra.uv_sphere()
    tv, tf = torch.tensor(v).to(DEV), torch.tensor(f).to(DEV)
    plan = rz.RasterPlan(tf, tv)
    cam = rz.Camera.fit(tv, (0.3, -0.2, 1.0), W, H)
    r = rz.rasterize(tv, plan, cam, H, W)
    hit = r.hit[0]
    assert int(hit.sum()) > H * W // 6 and int(r.dropped[0]) == 0 and not bool(hit[0, 0])      # the margin is free
    # interpolating the positions gives points of the sphere's surface at the pixel's depth along the view
    pos = rz.interpolate(r, plan, tv)[0]
    assert tuple(pos.shape) == (H, W, 3) and bool((pos[~hit] == 0).all())
    radius = pos[hit].norm(dim=-1)
    assert float(radius.max()) <= 1 + 1e-5 and float(radius.min()) > 0.9
    m = torch.tensor(cam.matrix).to(DEV)
    z = pos[hit] @ m[2, :3] + m[2, 3]
    assert float((z - r.depth[0][hit]).abs().max()) < 1e-5
    rgb = rz.shade(r, tv, plan, colors=rz.error_colors(tv[:, 2].abs(), vmax=1.0), background=(7, 8, 9))
    assert rgb.dtype == torch.uint8 and tuple(rgb.shape) == (1, H, W, 3)
    assert rgb[0][~hit].unique(dim=0).tolist() == [[7, 8, 9]] and int(rgb[0][hit].float().std()) > 5
    grey = rz.shade(r, tv, plan, normals=vertex_normals(tv, plan.topology))
    centre = grey[0, H // 2, W // 2].tolist()
    assert centre[0] == centre[1] == centre[2] and centre[0] > 240 and int(grey[0][hit].min()) >= 63      # facing the light; 0.25 ambient


def test_cross_check_with_the_ray_cast():
    """An orthographic camera whose screen axes are +x and +y of the world, 16 pixels per unit, a closed mesh on the 1/4096 grid:
    snapping is exact and so is the ray cast's shear for d = (0, 0, 1), the two symbolic displacements are the same -- so the
    number of covering faces equals the crossings of the pixel's ray at every pixel, ties included."""
    from nsdp_amd import ray_cast, rasterize as rz
    v, f, M, H, W = ra.cross_check_case()
    want = ra.image(v, f, M, H, W)
    o, d = ra.cross_check_rays(M, H, W)
    tv, tf = torch.tensor(v).to(DEV), torch.tensor(f).to(DEV)
    plan = rz.RasterPlan(tf, tv)
    assert plan.open_edges == 0
    r = rz.rasterize(tv, plan, torch.tensor(M).to(DEV).reshape(1, 4, 4), H, W, count=True)
    hits = ray_cast.cast_rays(torch.tensor(o).to(DEV), torch.tensor(d).to(DEV), tv, plan, count=True)
    count, cross = r.count[0].cpu().numpy(), hits.crossings.cpu().numpy().reshape(H, W)
    assert np.array_equal(count, want["count"]) and want["ties"] > 1000
    assert np.array_equal(count, cross) and np.isin(count, (0, 2)).all() and (count == 2).sum() > 700
    hit = r.hit[0].cpu().numpy()
    assert np.array_equal(hit, hits.hit.cpu().numpy().reshape(H, W))
    depth, t = r.depth[0].cpu().numpy().astype(np.float64), hits.t.cpu().numpy().reshape(H, W).astype(np.float64)
    zmax = float(np.abs(v[:, 2].astype(np.float64) + 2).max())
    bound = 2.0 ** -24 * (np.abs(depth) + np.abs(t)) * (1 + 2.0 ** -20) + (float(ra.D_ABS) + float(rr.T_ABS)) * zmax
    print("largest |depth - t| / bound", float((np.abs(depth - t)[hit] / bound[hit]).max()))
    assert (np.abs(depth - t)[hit] <= bound[hit]).all()
    clear = hit & (np.abs(want["second"].astype(np.float64) - want["depth"]) > 2.0 ** -20 * np.abs(want["depth"]))
    assert (hit & ~clear).sum() <= 0.02 * hit.sum()
    assert np.array_equal(r.face[0].cpu().numpy()[clear], hits.face.cpu().numpy().reshape(H, W)[clear])
