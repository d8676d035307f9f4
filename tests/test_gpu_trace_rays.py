"""Ray queries (rt2_trace_rays / rt2_trace_rays_host) against the sequential
scan of the oracle's rayTriangleIntersect: dst compared by bits, tri exactly.

The rays, scenes and the reference are those of tests/trace_rays_lib.py;
tests/test_trace_rays_cpu.py asserts on the oracle alone what they are built
to give (hits and misses in every case, no exact ties in the soups, ties in
the tie scene), so a pass here is not vacuous.

Every brute-force case runs on both paths: "auto" (RT2_TRACE_AUTO: the matrix
kernel trace_rays_k5r, whatever the ray count) and "scalar" (RT2_TRACE_SCALAR:
trace_rays_scalar); every query asserts which kernel ran.
"""
import numpy as np
import pytest

import closest_hit_scenes as S
import trace_rays_lib as T

pytestmark = pytest.mark.gpu

PATHS = ("auto", "scalar")
F32 = np.float32

_scenes = {}
_nodes = {}  # (scene, triangles) -> the node array of its BVH scene


def _scene(rt2mod, kind, n, bvh=False):
    """(scene, triangles as uploaded), made once per (scene, traversal)."""
    key = (kind, n, bvh)
    if key not in _scenes:
        tris, mats = T.scene_tris(kind, n), S.code_materials(n)
        if bvh:
            sd = S.scene_data(tris, mats)
            scene = rt2mod.Scene(sd)
            scene.set_traversal("bvh")
            up = sd.triangles()
            up.setflags(write=False)
            _nodes[(kind, n)] = sd.nodes()
        else:
            scene, up = rt2mod.Scene(triangles=tris, materials=mats), tris
        _scenes[key] = (scene, up)
    return _scenes[key]


def _expected_kernel(rt2mod, scene, path, n_rays):
    """The kernel a brute-force query must have run on (Scene.last_kernel)."""
    if path == "scalar":
        return rt2mod.QUERY_SCALAR
    return rt2mod.QUERY_RES if scene.n_tris <= 38 * 32 else rt2mod.QUERY_RES_L2


def _trace(rt2mod, scene, path, o, d, tmax=None):
    got = scene.trace_rays(o, d, tmax, rt2mod.TRACE_SCALAR if path == "scalar" else rt2mod.TRACE_AUTO)
    assert scene.last_kernel() == _expected_kernel(rt2mod, scene, path, len(got[0])), path
    return got


def _same(got, dst, tri, what):
    gd, gt = got
    assert gd.dtype == F32 and gt.dtype == np.int32 and len(gd) == len(dst) == len(gt)
    bad = (gd.view(np.uint32) != np.asarray(dst, F32).view(np.uint32)) | (gt != tri)
    if bad.any():
        lines = [f"ray {i}: GPU ({gd[i]!r}, {gt[i]}), reference ({dst[i]!r}, {tri[i]})" for i in np.flatnonzero(bad)[:6]]
        raise AssertionError(f"{what}: {int(bad.sum())} of {len(bad)} rays differ\n" + "\n".join(lines))


def _soup1217(oraclemod):
    """The 1,025 rays of the 1,217-triangle soup with their reference; the
    smaller cases are prefixes."""
    o, d = T.scene_rays("soup", 1217, 1025)
    dst, tri, _ = T.scene_ref(oraclemod, "soup", 1217, 1025)
    return o, d, dst, tri


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("n", T.SOUP_SIZES)
def test_triangle_counts(rt2mod, oraclemod, n, path):
    """1; the group edge 32 / 33; all resident 1,216 and the first group from
    L2 1,217; the renders' launcher boundary 8,192 / 8,193, which means
    nothing here."""
    if n == 1217:
        o, d, dst, tri = (a[:193] for a in _soup1217(oraclemod))
    else:
        nr = T.n_rays_for(n)
        o, d = T.scene_rays("soup", n, nr)
        dst, tri, _ = T.scene_ref(oraclemod, "soup", n, nr)
    scene, _ = _scene(rt2mod, "soup", n)
    _same(_trace(rt2mod, scene, path, o, d), dst, tri, f"soup {n} {path}")


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("k", T.RAY_COUNTS)
def test_ray_counts(rt2mod, oraclemod, k, path):
    """upper = false (<= 32 live rays), both 32-ray blocks, a ragged last
    chunk, a second workgroup (1,025)."""
    o, d, dst, tri = (a[:k] for a in _soup1217(oraclemod))
    scene, _ = _scene(rt2mod, "soup", 1217)
    _same(_trace(rt2mod, scene, path, o, d), dst, tri, f"{k} rays {path}")


@pytest.mark.parametrize("path", PATHS)
def test_more_than_one_pass_of_the_grid(rt2mod, oraclemod, path):
    """300,001 rays repeating a 257-ray pattern: 4,688 chunks for at most
    4,096 waves; every output equals its pattern entry's."""
    n, m = 300_001, 257
    o, d, dst, tri = (a[:m] for a in _soup1217(oraclemod))
    idx = np.arange(n) % m
    scene, _ = _scene(rt2mod, "soup", 1217)
    _same(_trace(rt2mod, scene, path, o[idx], d[idx]), dst[idx], tri[idx], f"{n} rays {path}")


@pytest.mark.parametrize("path", PATHS)
def test_bounds(rt2mod, oraclemod, path):
    o, d, dst, tri = (a[:193] for a in _soup1217(oraclemod))
    scene, _ = _scene(rt2mod, "soup", 1217)
    hit = tri >= 0
    miss = np.full(len(tri), -1, np.int32)
    _same(_trace(rt2mod, scene, path, o, d), dst, tri, "unbounded")
    # tmax = dst: the comparison is strict, every ray misses (a miss's dst is its bound)
    tmax = np.where(hit, dst, F32(0))
    _same(_trace(rt2mod, scene, path, o, d, tmax), dst, miss, "tmax = dst")
    # one ulp above: the same hit, the same bits
    tmax = np.where(hit, np.nextafter(dst, F32(np.inf)), F32(0)).astype(F32)
    _same(_trace(rt2mod, scene, path, o, d, tmax), dst, tri, "tmax = nextafter(dst)")
    # halfway to the hit: a miss with dst == tmax
    tmax = np.where(hit, dst * F32(0.5), F32(0)).astype(F32)
    _same(_trace(rt2mod, scene, path, o, d, tmax), np.where(hit, tmax, T.UNBOUNDED), miss, "tmax = dst / 2")
    for v in (0.0, -1.0, np.nan, np.inf, 2e38):
        with np.errstate(over="ignore"):
            tmax = np.full(len(tri), v).astype(F32)  # 2e38 rounds to +inf in float32: unbounded as well
        _same(_trace(rt2mod, scene, path, o, d, tmax), dst, tri, f"tmax = {v}")


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("order", T.FAN_ORDERS)
def test_fans(rt2mod, oraclemod, order, path):
    """64 triangles all hit by every camera ray: far first, the bound improves
    again and again inside one window."""
    o, d = T.scene_rays("fan_" + order, 64, 97)
    dst, tri, _ = T.scene_ref(oraclemod, "fan_" + order, 64, 97)
    scene, _ = _scene(rt2mod, "fan_" + order, 64)
    _same(_trace(rt2mod, scene, path, o, d), dst, tri, f"fan {order} {path}")


@pytest.mark.parametrize("path", PATHS)
def test_ties_go_to_the_lowest_index(rt2mod, oraclemod, path):
    n = 1217
    o, d = T.scene_rays("ties", n, 193)
    dst, tri, ties = T.scene_ref(oraclemod, "ties", n, 193)
    scene, _ = _scene(rt2mod, "ties", n)
    got = _trace(rt2mod, scene, path, o, d)
    _same(got, dst, tri, f"ties {path}")
    for fam in S.tie_families(n):  # also the family that straddles index 1,216
        assert (got[1] == min(fam)).sum() >= 4 and not np.isin(got[1], sorted(fam)[1:]).any()


MIXED = {"far": (5,), "long": (40,), "nan": (41,), "inf": (50,), "all": (5, 40, 41, 50)}


def _mixed_rays(oraclemod, which):
    o, d = (a[:64].copy() for a in _soup1217(oraclemod)[:2])
    for lane in MIXED[which]:
        if lane == 5:  # |o| = 2^21: outside the filter's range
            o[5] = (T.FAR, 5.0, 10.0)
        elif lane == 40:  # an unnormalised direction of length 3
            d[40] *= F32(3)
        elif lane == 41:
            o[41, 0] = np.nan
        else:
            d[50, 1] = np.inf
    return o, d


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("which", list(MIXED))
def test_mixed_waves(rt2mod, oraclemod, which, path):
    """One 64-ray chunk of ordinary rays with lane 5 far outside, lane 40
    unnormalised, lane 41 a NaN origin, lane 50 an infinite direction
    component (each alone, then all four): all 64 equal the reference."""
    o, d = _mixed_rays(oraclemod, which)
    dst, tri, _ = T.reference(oraclemod, T.scene_tris("soup", 1217), o, d)
    base = _soup1217(oraclemod)[3][:64]
    assert (tri >= 0).sum() >= 16
    assert (tri[[l for l in MIXED[which] if l in (41, 50)]] == -1).all()  # non-finite: the reference misses
    others = np.setdiff1d(np.arange(64), MIXED[which])
    assert np.array_equal(tri[others], base[others])  # the reference's own other rays are undisturbed
    scene, _ = _scene(rt2mod, "soup", 1217)
    _same(_trace(rt2mod, scene, path, o, d), dst, tri, f"mixed {which} {path}")


@pytest.mark.parametrize("path", PATHS)
def test_scene_outside_the_filters_range(rt2mod, oraclemod, path):
    """The 33-triangle soup with one vertex at 2^21 (beyond the matrix
    filter's |a| <= 2^20)."""
    o, d = T.scene_rays("far", 33, 193)
    dst, tri, _ = T.scene_ref(oraclemod, "far", 33, 193)
    scene, _ = _scene(rt2mod, "far", 33)
    _same(_trace(rt2mod, scene, path, o, d), dst, tri, f"far {path}")


@pytest.mark.parametrize("n", (1217, 8193))
def test_bvh_traversal(rt2mod, oraclemod, n):
    """The BVH walk against the array scan over the triangles as uploaded
    (build_bvh reorders them), unbounded and bounded.  The scan is a valid
    reference for the walk here, and only here: the soups have no exact
    distance ties (the walk visits the leaves in another order than the scan,
    so a tie could go to another triangle), and build_bvh's boxes are tight
    around their triangles (a box never hides a hit the scan finds).  On trees
    without these properties (tests/test_gpu_bvh_edges.py) only the oracle's
    own walk is the reference; it is checked here as well."""
    nr = 193 if n == 1217 else 97
    o, d = T.scene_rays("soup", n, nr)
    scene, up = _scene(rt2mod, "soup", n, bvh=True)
    dst, tri, ties = T.scene_ref(oraclemod, "soup", n, nr, tris=up, tag="bvh")
    assert ties.max() == 1
    _same(scene.trace_rays(o, d), dst, tri, f"bvh {n}")
    assert scene.last_kernel() == rt2mod.QUERY_BVH
    nodes = _nodes[("soup", n)]
    wd, wt, wtests, wvisits = oraclemod.closest_hits(up, o, d, None, "bvh", nodes)
    _same(scene.trace_rays(o, d), wd, wt, f"bvh {n} against the oracle's walk")
    scene.stats(reset=True)
    scene.trace_rays(o, d)
    st = scene.stats(reset=True)
    assert st.tests == int(wtests.sum()) and st.node_visits == int(wvisits.sum())
    # bounds by turns one ulp above the hit (the same hit), halfway to it (a miss) and none
    hit, i = tri >= 0, np.arange(nr)
    tmax = np.select([hit & (i % 3 == 0), hit & (i % 3 == 1)],
                     [np.nextafter(dst, F32(np.inf)), dst * F32(0.5)], F32(0)).astype(F32)
    cut = hit & (i % 3 == 1)
    _same(scene.trace_rays(o, d, tmax), np.where(cut, tmax, dst), np.where(cut, -1, tri), f"bvh {n} bounded")
    scene.stats(reset=True)
    scene.trace_rays(o, d)
    st = scene.stats(reset=True)
    assert st.segments == nr and 0 < st.tests < nr * n and st.node_visits > 0


@pytest.mark.parametrize("kind", ("soup", "ties"))
def test_forced_scalar_equals_auto(rt2mod, oraclemod, kind):
    n, nr = 1217, 1025 if kind == "soup" else 193
    o, d = T.scene_rays(kind, n, nr)
    scene, _ = _scene(rt2mod, kind, n)
    a = _trace(rt2mod, scene, "auto", o, d)
    b = _trace(rt2mod, scene, "scalar", o, d)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("path", PATHS)
def test_stats(rt2mod, oraclemod, path):
    o, d = (a[:193] for a in _soup1217(oraclemod)[:2])
    scene, _ = _scene(rt2mod, "soup", 1217)
    scene.stats(reset=True)
    _trace(rt2mod, scene, path, o, d)
    st = scene.stats(reset=True)
    assert st.segments == 193 and st.tests == 193 * 1217 and st.node_visits == 0


@pytest.mark.parametrize("path", PATHS)
def test_device_pointer_form(rt2mod, oraclemod, path):
    """rt2_trace_rays on a non-default stream with torch tensors."""
    import torch
    o, d, dst, tri = (a[:193] for a in _soup1217(oraclemod))
    rays = np.zeros(193, rt2mod.RAY_DTYPE)
    rays["o"], rays["d"] = o, d
    scene, _ = _scene(rt2mod, "soup", 1217)
    flags = rt2mod.TRACE_SCALAR if path == "scalar" else rt2mod.TRACE_AUTO
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        d_rays = torch.from_numpy(rays.view(np.uint8).copy()).to("cuda", non_blocking=False)
        d_hits = torch.full((193 * 8,), 0xAB, dtype=torch.uint8, device="cuda")
        st.synchronize()
        scene.trace_rays_device(d_rays.data_ptr(), 193, d_hits.data_ptr(), flags, st.cuda_stream)
        st.synchronize()
    assert scene.last_kernel() == _expected_kernel(rt2mod, scene, path, 193)
    hits = d_hits.cpu().numpy().view(rt2mod.HIT_DTYPE)
    _same((hits["dst"].copy(), hits["tri"].copy()), dst, tri, f"device form {path}")
    host = _trace(rt2mod, scene, path, o, d)
    _same(host, hits["dst"], hits["tri"], "host form against device form")


def test_render_unchanged_by_queries(rt2mod, oraclemod):
    """One index-coded image before a query and one after it on the same
    scene: identical bits (and the oracle's)."""
    n = 1217
    tris, mats = S.coded_scene("soup", n)
    w, h = S.SIZES[n]
    u = S.coded_uniforms(w, h, n)
    scene = rt2mod.Scene(triangles=tris, materials=mats)
    before = scene.render_host(u, 0, 1)
    o, d, dst, tri = (a[:193] for a in _soup1217(oraclemod))
    for path in PATHS:
        _same(_trace(rt2mod, scene, path, o, d), dst, tri, path)
    after = scene.render_host(u, 0, 1)
    assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
    acc, _, _, _ = oraclemod.render(tris, mats, u, np.arange(h, dtype=np.int32), 0, 1, "brute")
    assert np.array_equal(np.ascontiguousarray(before[..., :3]).view(np.uint32),
                          np.ascontiguousarray(acc[..., :3]).view(np.uint32))
