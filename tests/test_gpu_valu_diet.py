"""Bit-exactness of the shortened shading: the per-triangle unit normals
computed at scene upload (prep_unit_normals) and rnd_dir's sqrt-free
acceptance test, on scenes that also pin the exact phase's division (tiny and
huge determinants).

Every image is compared with the CPU oracle as uint32 views (no tolerance).
mt_exact and shade are shared by all kernels, so each scene runs the automatic
brute-force kernel, the scalar kernel (variant 136) and the BVH traversal.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, RAYS = 64, 36, 4
SCALAR = 136


def _same_bits(gpu, ref, what):
    a = np.ascontiguousarray(gpu[..., :3], dtype=np.float32).view(np.uint32)
    b = np.ascontiguousarray(ref[..., :3], dtype=np.float32).view(np.uint32)
    bad = (a != b).any(-1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} pixels differ in their bits"


def _oracle(oraclemod, sd, u, mode):
    acc, _, segs, _ = oraclemod.render(sd.triangles(), sd.materials(), u, np.arange(u.height, dtype=np.int32), 0, 1,
                                       mode, nodes=sd.nodes() if mode == "bvh" else None)
    return acc, segs


_refs = {}


def _ref(oraclemod, key, sd, u, mode):
    """One oracle image per (scene, traversal), shared by the tests and left unchanged."""
    if (key, mode) not in _refs:
        acc, segs = _oracle(oraclemod, sd, u, mode)
        acc.setflags(write=False)
        _refs[(key, mode)] = (acc, segs)
    return _refs[(key, mode)]


def _render(rt2mod, sd, u, how):
    scene = rt2mod.Scene(sd, 0)
    if how == "bvh":
        scene.set_traversal("bvh")
    elif how == "scalar":
        scene.set_variant(SCALAR)
    img = scene.render_host(u, 0, 1)
    return img, scene.stats(reset=True).segments


@pytest.mark.parametrize("how", ["auto", "scalar", "bvh"])
@pytest.mark.parametrize("cfg", ["B", "K"])
def test_configs_bit_identical(rt2mod, oraclemod, config_scene, cfg, how):
    sd, spec = config_scene(cfg)
    u = rt2mod.offline_uniforms(W, H, spec.bounces, RAYS, sd.num_triangles)
    mode = "bvh" if how == "bvh" else "brute"
    ref, segs = _ref(oraclemod, cfg, sd, u, mode)
    img, gsegs = _render(rt2mod, sd, u, how)
    _same_bits(img, ref, f"config {cfg} {how}")
    assert gsegs == segs


def _quad(sd, p, eu, ev, mtl):
    """Two triangles spanning p + s*eu + t*ev; normal eu x ev (the side that is hit)."""
    p, eu, ev = (np.asarray(x, np.float64) for x in (p, eu, ev))
    sd.add_triangle(tuple(p), tuple(p + eu), tuple(p + ev), mtl)
    sd.add_triangle(tuple(p + eu), tuple(p + eu + ev), tuple(p + ev), mtl)


TINY = [1e-4, 1e-3, 1e-2, 1e-1, 1.0]


def scale_spread_scene(rt2mod):
    """A box around the default camera ((0, 5, 10), looking down -z) whose 21
    triangles have edges from 1e-4 to 1e3: a 1000-unit floor, a mirror back
    wall, a two-faced glass pane in front of the left wall, a light ceiling,
    and five triangles of edge s = 1e-4 .. 1 placed 10 s in front of the camera
    (each about 12 pixels wide), one per material kind, so the stored normals
    of |n| = 1e-8 .. 1e6 are all read by shade."""
    M = rt2mod.Material
    sd = rt2mod.SceneData()
    white = sd.add_material(M.diffuse((0.9, 0.9, 0.9)))
    green = sd.add_material(M.diffuse((0.1, 0.9, 0.1)))
    red = sd.add_material(M.diffuse((0.9, 0.1, 0.1)))
    light = sd.add_material(M.light((1, 1, 1), 6.0))
    mirror = sd.add_material(M.specular((1, 1, 1), (1, 1, 1), 1.0, 1.0))
    glass = sd.add_material(M.glass((0.9, 0.95, 1.0), 1.5))
    checker = sd.add_material(M.checker(3.0))
    metal = sd.add_material(M.specular((0.8, 0.6, 0.3), (1, 1, 1), 0.7, 0.4))
    _quad(sd, (-500, 0, -500), (0, 0, 1000), (1000, 0, 0), checker)   # floor, n = +y
    _quad(sd, (-6, 0, -8), (12, 0, 0), (0, 10, 0), mirror)           # back wall, n = +z
    _quad(sd, (-5, 0, -8), (0, 10, 0), (0, 0, 20), glass)            # glass pane: entry face, n = +x
    _quad(sd, (-5.5, 0, -8), (0, 10, 0), (0, 0, 20), glass)          # ... exit face (met from inside), n = +x
    _quad(sd, (-6, 0, -8), (0, 10, 0), (0, 0, 20), red)              # left wall, n = +x
    _quad(sd, (6, 0, -8), (0, 0, 20), (0, 10, 0), green)             # right wall, n = -x
    _quad(sd, (-6, 10, -8), (12, 0, 0), (0, 0, 20), light)           # ceiling, n = -y
    _quad(sd, (-6, 0, 12), (0, 10, 0), (12, 0, 0), white)            # behind the camera, n = -z
    cam = np.float64([0, 5, 10])
    for i, (s, mtl) in enumerate(zip(TINY, (white, metal, glass, checker, mirror))):
        dist = 10.0 * s
        a = cam + dist * np.float64([-0.2 + 0.1 * i - 0.05, (-0.1 if i % 2 else 0.02), -1.0])
        sd.add_triangle(tuple(a), tuple(a + [s, 0, 0]), tuple(a + [0, s, 0]), mtl)  # n = +z, faces the camera
    sd.build_bvh()
    return sd


@pytest.fixture(scope="module")
def spread(rt2mod):
    sd = scale_spread_scene(rt2mod)
    assert sd.num_triangles == 21
    return sd, rt2mod.offline_uniforms(W, H, 8, RAYS, sd.num_triangles)


def test_scale_spread_scene_spans_the_scales(rt2mod, spread):
    sd, _ = spread
    t = sd.triangles()
    a, b, c = (t[k][:, :3].astype(np.float64) for k in "abc")
    e = np.concatenate([np.linalg.norm(b - a, axis=1), np.linalg.norm(c - a, axis=1)])
    assert e.min() <= 1.0001e-4 and e.max() >= 1e3
    n = np.linalg.norm(np.cross(b - a, c - a), axis=1)
    assert n.min() >= 0.99e-8 and n.max() >= 1e6  # every det of a facing hit stays above mt_exact's 1e-10


@pytest.mark.parametrize("how", ["auto", "scalar", "bvh"])
def test_scale_spread_bit_identical(rt2mod, oraclemod, spread, how):
    sd, u = spread
    mode = "bvh" if how == "bvh" else "brute"
    ref, segs = _ref(oraclemod, "spread", sd, u, mode)
    img, gsegs = _render(rt2mod, sd, u, how)
    _same_bits(img, ref, f"scale spread {how}")
    assert gsegs == segs
    # each tiny triangle is in the picture: without it the oracle's image differs
    if how == "auto":
        for k in range(16, 21):
            sd0 = rt2mod.SceneData()
            sd0.add_triangles(np.delete(sd.triangles(), k))
            acc0, _, _, _ = oraclemod.render(sd0.triangles(), sd.materials(), u, np.arange(H, dtype=np.int32), 0, 1,
                                             "brute")
            assert (acc0[..., :3] != ref[..., :3]).any(), f"triangle {k} is never hit"


@pytest.mark.parametrize("how", ["auto", "scalar"])
def test_det_above_2_100(rt2mod, oraclemod, how):
    """One triangle with vertices near 2^60 in the plane z = -5: |n| = 2^122, so
    every det of a hit is above 2^100, where only the full IEEE division
    sequence is right (and the scene is outside the matrix filter's range): the
    unit normal's |n|^2 overflows.  Same bits as the oracle."""
    M = rt2mod.Material
    sd = rt2mod.SceneData()
    grey = sd.add_material(M.diffuse((0.7, 0.7, 0.7)))
    light = sd.add_material(M.light((1, 1, 1), 5.0))
    B = float(2 ** 60)
    sd.add_triangle((-B, -B, -5.0), (B, -B, -5.0), (0.0, B, -5.0), grey)
    _quad(sd, (-4, 9, -4), (8, 0, 0), (0, 0, 12), light)  # n = -y, above the camera
    t = sd.triangles()[0]
    e0 = (t["b"][:3] - t["a"][:3]).astype(np.float64)
    e1 = (t["c"][:3] - t["a"][:3]).astype(np.float64)
    assert abs(np.cross(e0, e1)[2]) * 0.9 > 2.0 ** 100  # det = -d.n with d.z <= -0.9 through the image
    u = rt2mod.offline_uniforms(W, H, 8, RAYS, sd.num_triangles)
    ref, segs = _ref(oraclemod, "huge", sd, u, "brute")
    assert (ref[..., :3] != ref[0, 0, :3]).any()  # not a constant image
    img, gsegs = _render(rt2mod, sd, u, how)
    _same_bits(img, ref, f"det > 2^100, {how}")
    assert gsegs == segs
