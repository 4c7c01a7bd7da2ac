"""GPU: what nsdp_amd/ray_cast.py builds on the cast -- ``contains`` (the parity of the crossings) against the emulation on the
same points and against the analytic answer on a cube and a sphere for points farther from the surface than the stated
envelope; ``volume_iou``: integer counts equal to the emulation's on the same samples, and 1/3 for two unit cubes offset by
(1/2, 0, 0) within four binomial standard deviations for the N used."""
import math

import numpy as np
import pytest
import torch

import ray_cast_ref as rr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
f32 = np.float32
UP = np.array([0, 0, 1], f32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _inside_ref(p, v, f):
    return rr.cast(p, np.tile(UP, (len(p), 1)), v, f)[3] % 2 == 1


def _envelope(p, v):
    """The stated envelope of ``contains``: 6 * 2^-24 of the largest coordinate difference R between the points and the
    corners, on x and on y of the sheared frame (a lateral distance of at most sqrt(2) of it: doubled here)."""
    R = float(np.abs(p[:, None, :] - v[None, :, :]).max())
    return 2 * rr.SHEAR_XY * 2.0 ** -24 * R


@pytest.mark.parametrize("cull", [True, False])
def test_contains_on_a_cube(cull):
    from nsdp_amd import ray_cast as rc
    v, f = rr.cube()
    rng = np.random.default_rng(4)
    p = rng.uniform(-1.5, 1.5, (3000, 3)).astype(f32)
    near = rng.uniform(-0.9, 0.9, (400, 3)).astype(f32)                       # just inside and just outside every face
    axis, side = rng.integers(0, 3, 400), rng.choice([-1.0, 1.0], 400)
    near[np.arange(400), axis] = (side * (1 + np.where(np.arange(400) % 2, 1e-4, -1e-4))).astype(f32)
    p = np.concatenate([p, near, f32([[0, 0, 0], [0.5, 0.5, -3], [0.25, -0.5, 3]])])      # (below: two crossings; above: none)
    plan = rc.RayCastPlan(_dev(f), _dev(v))
    assert plan.open_edges == 0
    got = rc.contains(_dev(p), _dev(v), plan, cull=cull).cpu().numpy()
    assert got.dtype == np.bool_ and np.array_equal(got, _inside_ref(p, v, f))
    dist = np.abs(np.abs(p).max(axis=1) - 1)                                  # the distance to the surface along the nearest axis
    clear = dist > _envelope(p, v)
    assert clear.sum() >= len(p) - 5 and clear[3000:3400].all()
    assert np.array_equal(got[clear], (np.abs(p).max(axis=1) < 1)[clear])
    assert got[3000:3400:2].all() and not got[3001:3400:2].any() and got[-3] and not got[-2] and not got[-1]
    # another direction gives the same answer on the clear points
    other = rc.contains(_dev(p), _dev(v), plan, direction=(0.3, -1.0, 0.2), cull=cull).cpu().numpy()
    assert np.array_equal(other[clear], got[clear])


def test_contains_on_a_sphere():
    from nsdp_amd import ray_cast as rc
    v, f = rr.sphere()
    tri = v[f].astype(np.float64)
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    r_in = float(np.min(np.abs((n * tri[:, 0]).sum(1)) / np.linalg.norm(n, axis=1)))      # the inscribed radius of the polyhedron
    assert 0.99 < r_in < 1
    rng = np.random.default_rng(8)
    p = rng.uniform(-1.2, 1.2, (4000, 3)).astype(f32)
    plan = rc.RayCastPlan(_dev(f), _dev(v))
    got = rc.contains(_dev(p), _dev(v), plan).cpu().numpy()
    assert np.array_equal(got, _inside_ref(p, v, f))
    r, env = np.linalg.norm(p.astype(np.float64), axis=1), _envelope(p, v)
    assert got[r < r_in - env].all() and not got[r > 1 + env].any() and (r < r_in - env).sum() > 1000 and (r > 1 + env).sum() > 1000


def test_contains_layouts():
    from nsdp_amd import ray_cast as rc
    from nsdp_amd.ragged import RaggedPoints
    v, f = rr.cube()
    rng = np.random.default_rng(5)
    p = rng.uniform(-1.5, 1.5, (2, 500, 3)).astype(f32)
    v2 = np.stack([v, v * f32(0.5)])
    plan = rc.RayCastPlan(_dev(f), _dev(v2))
    got = rc.contains(_dev(p), _dev(v2), plan).cpu().numpy()
    assert np.array_equal(got[0], _inside_ref(p[0], v2[0], f)) and np.array_equal(got[1], _inside_ref(p[1], v2[1], f))
    vs, fs = rr.uv_sphere()
    rv = RaggedPoints.from_list([_dev(v), _dev(vs)])
    rplan = rc.RayCastPlan(RaggedPoints.from_list([_dev(f), _dev(fs)]), rv)
    rp = RaggedPoints.from_list([_dev(p[0][:100]), _dev(p[1])], capacity=700)
    rgot = rc.contains(rp, rv, rplan)
    assert isinstance(rgot, RaggedPoints) and rgot.packed.dtype == torch.bool
    assert np.array_equal(rgot.packed[:100, 0].cpu().numpy(), _inside_ref(p[0][:100], v, f))
    assert np.array_equal(rgot.packed[100:600, 0].cpu().numpy(), _inside_ref(p[1], vs, fs))


N = 20000


def test_volume_iou_of_two_offset_unit_cubes():
    from nsdp_amd import ray_cast as rc
    v, f = rr.cube(0.0, 1.0)
    va, vb = v, (v + f32([0.5, 0, 0])).astype(f32)
    plan = rc.RayCastPlan(_dev(f), _dev(va))
    g = torch.Generator(device=DEV)
    g.manual_seed(17)
    pts = rc.iou_samples(_dev(va), _dev(vb), plan, N, generator=g)
    g.manual_seed(17)
    iou, a, b, both = rc.volume_iou(_dev(va), _dev(vb), plan, N, generator=g)
    assert a.dtype == torch.int64 and both.dtype == torch.int64 and iou.dtype == torch.float64 and iou.shape == ()
    p = pts.cpu().numpy()
    assert p.shape == (N, 3) and p.min() >= 0 and p[:, 0].max() <= 1.5 and p[:, 1:].max() <= 1
    ia, ib = _inside_ref(p, va, f), _inside_ref(p, vb, f)
    assert (int(a), int(b), int(both)) == (int(ia.sum()), int(ib.sum()), int((ia & ib).sum()))      # the emulation's counts, exactly
    assert float(iou) == int(both) / (int(a) + int(b) - int(both))
    bound = 4 * math.sqrt((1 / 3) * (2 / 3) / N)                              # four binomial standard deviations for N samples
    print("iou", float(iou), "bound", bound, "counts", int(a), int(b), int(both))
    assert abs(float(iou) - 1 / 3) <= bound


def test_volume_iou_layouts_and_an_empty_union():
    from nsdp_amd import ray_cast as rc
    from nsdp_amd.ragged import RaggedPoints
    v, f = rr.cube(0.0, 1.0)
    shift = (v + f32([0.5, 0, 0])).astype(f32)
    # faces of their own, B = 2: the pair above, and a mesh against itself (IoU 1)
    plan = rc.RayCastPlan(_dev(np.stack([f, f])), _dev(np.stack([v, v])))
    g = torch.Generator(device=DEV)
    g.manual_seed(3)
    iou, a, b, both = rc.volume_iou(_dev(np.stack([v, v])), _dev(np.stack([shift, v])), plan, 4000, generator=g)
    assert iou.shape == (2,) and abs(float(iou[0]) - 1 / 3) <= 4 * math.sqrt(2 / 9 / 4000) and float(iou[1]) == 1.0
    assert int(a[1]) == int(b[1]) == int(both[1]) > 3900
    # packed: a cube pair and a sphere against a copy of itself collapsed to a point (nothing inside it: the union is the sphere)
    vs, fs = rr.uv_sphere()
    ra = RaggedPoints.from_list([_dev(v), _dev(vs)])
    rb = RaggedPoints.from_list([_dev(shift), _dev(vs * f32(0))])
    rplan = rc.RayCastPlan(RaggedPoints.from_list([_dev(f), _dev(fs)]), ra)
    g.manual_seed(3)
    pts = rc.iou_samples(ra, rb, rplan, 3000, generator=g)
    g.manual_seed(3)
    iou, a, b, both = rc.volume_iou(ra, rb, rplan, 3000, generator=g)
    p = pts.packed.cpu().numpy()
    ia, ib = _inside_ref(p[:3000], v, f), _inside_ref(p[:3000], shift, f)
    assert (int(a[0]), int(b[0]), int(both[0])) == (int(ia.sum()), int(ib.sum()), int((ia & ib).sum()))
    assert int(a[1]) == int(_inside_ref(p[3000:], vs, fs).sum()) > 1000 and int(b[1]) == 0 and float(iou[1]) == 0.0
    # both poses collapsed: no sample is inside either, the union is empty and the IoU is 0 by definition
    zero = RaggedPoints.from_list([_dev(v * f32(0)), _dev(vs * f32(0))])
    iou, a, b, both = rc.volume_iou(zero, zero, rplan, 100, generator=g)
    assert iou.tolist() == [0.0, 0.0] and int(a.sum()) == 0
