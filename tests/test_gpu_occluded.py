"""Occlusion queries (rt2_occluded / rt2_occluded_host) against the oracle:
occluded[i] == (oracle.closest_hits(...)[1][i] >= 0), every ray of every case,
nothing sampled.

The scenes, rays and chunks are those of tests/occluded_lib.py and
tests/trace_rays_lib.py; tests/test_occluded_cpu.py asserts on the oracle alone
what they are built to give, so a pass here is not vacuous.

Every brute-force case runs on both paths: "auto" (RT2_TRACE_AUTO: the matrix
kernel occluded_k5r) and "scalar" (RT2_TRACE_SCALAR: occluded_scalar); every
query asserts which kernel ran.
"""
import numpy as np
import pytest

import bvh_edge_scenes as E
import closest_hit_scenes as S
import occluded_lib as O
import trace_rays_lib as T

pytestmark = pytest.mark.gpu

PATHS = ("auto", "scalar")
F32 = np.float32

_scenes = {}
_nodes = {}


def _scene(rt2mod, kind, n, bvh=False):
    """(scene, triangles as uploaded), made once per (scene, traversal)."""
    key = (kind, n, bvh)
    if key not in _scenes:
        tris = O.pickets(n) if kind == "pickets" else T.scene_tris(kind, n)
        mats = S.code_materials(n)
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


def _expected_kernel(rt2mod, scene, path):
    if path == "scalar":
        return rt2mod.OCCLUDED_SCALAR
    return rt2mod.OCCLUDED_RES if scene.n_tris <= 38 * 32 else rt2mod.OCCLUDED_RES_L2


def _query(rt2mod, scene, path, o, d, tmax=None, kernel=None):
    got = scene.occluded(o, d, tmax, rt2mod.TRACE_SCALAR if path == "scalar" else rt2mod.TRACE_AUTO)
    assert scene.last_kernel() == (_expected_kernel(rt2mod, scene, path) if kernel is None else kernel), path
    assert got.dtype == bool and got.shape == (len(o),)
    return got


def _same(got, want, what):
    assert len(got) == len(want)
    bad = got != want
    if bad.any():
        lines = [f"ray {i}: GPU {bool(got[i])}, oracle {bool(want[i])}" for i in np.flatnonzero(bad)[:8]]
        raise AssertionError(f"{what}: {int(bad.sum())} of {len(bad)} rays differ\n" + "\n".join(lines))


_soup_ref = {}


def _soup(oraclemod, n, nr):
    if (n, nr) not in _soup_ref:
        o, d = T.scene_rays("soup", n, nr)
        occ, dst, _, _ = O.occluded_ref(oraclemod, T.scene_tris("soup", n), o, d)
        for a in (occ, dst):
            a.setflags(write=False)
        _soup_ref[(n, nr)] = (o, d, occ, dst)
    return _soup_ref[(n, nr)]


def _soup1217(oraclemod):
    return _soup(oraclemod, 1217, 1025)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("n", T.SOUP_SIZES)
def test_triangle_counts(rt2mod, oraclemod, n, path):
    o, d, occ, _ = (a[:193] for a in _soup1217(oraclemod)) if n == 1217 else _soup(oraclemod, n, T.n_rays_for(n))
    scene, _ = _scene(rt2mod, "soup", n)
    _same(_query(rt2mod, scene, path, o, d), occ, f"soup {n} {path}")


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("k", T.RAY_COUNTS)
def test_ray_counts(rt2mod, oraclemod, k, path):
    """upper = false (<= 32 live rays), both 32-ray blocks, ragged last chunks,
    a second workgroup (1,025)."""
    o, d, occ, _ = (a[:k] for a in _soup1217(oraclemod))
    scene, _ = _scene(rt2mod, "soup", 1217)
    _same(_query(rt2mod, scene, path, o, d), occ, f"{k} rays {path}")


@pytest.mark.parametrize("path", PATHS)
def test_more_than_one_pass_of_the_grid(rt2mod, oraclemod, path):
    """300,001 rays repeating a 257-ray pattern: every output equals its pattern
    entry's, and the GPU's own closest-hit query says the same."""
    n, m = 300_001, 257
    o, d, occ, _ = (a[:m] for a in _soup1217(oraclemod))
    idx = np.arange(n) % m
    scene, _ = _scene(rt2mod, "soup", 1217)
    got = _query(rt2mod, scene, path, o[idx], d[idx])
    _same(got, occ[idx], f"{n} rays {path}")
    tri = scene.trace_rays(o[idx], d[idx], None, rt2mod.TRACE_SCALAR if path == "scalar" else rt2mod.TRACE_AUTO)[1]
    _same(got, tri >= 0, f"{n} rays {path} against trace_rays")


@pytest.mark.parametrize("path", PATHS)
def test_bounds(rt2mod, oraclemod, path):
    o, d, hit, dst = (a[:193] for a in _soup1217(oraclemod))
    scene, _ = _scene(rt2mod, "soup", 1217)
    _same(_query(rt2mod, scene, path, o, d), hit, "unbounded")
    for name, tmax, want in O.bound_cases(dst, hit):
        _same(_query(rt2mod, scene, path, o, d, tmax), want, f"{name} {path}")


# ---- exit logic on the pickets ---------------------------------------------------------------------------------

@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("n", O.PICKETS)
def test_exit_logic(rt2mod, oraclemod, n, path):
    """The chunks of occluded_lib.chunks as one call (adjacent chunks, on
    different waves; each ragged chunk as that call's tail), each chunk alone
    and the first 32 rays of each alone."""
    ch = O.chunks(n)
    tris = O.pickets(n)
    scene, _ = _scene(rt2mod, "pickets", n)
    want = {k: O.occluded_ref(oraclemod, tris, ch[k][0], ch[k][1])[0] for k in ch}
    for k in ch:
        assert np.array_equal(want[k], ch[k][2] >= 0), k  # the oracle's scan and the claim (the premises test)
    for tail in O.RAGGED:
        names = O.FULL + (tail,)
        o, d = O._cat(*[ch[k][:2] for k in names])
        _same(_query(rt2mod, scene, path, o, d), np.concatenate([want[k] for k in names]), f"pickets({n}) +{tail} {path}")
    for k in ch:
        o, d, _ = ch[k]
        _same(_query(rt2mod, scene, path, o, d), want[k], f"pickets({n}) chunk {k} alone {path}")
        if len(o) > 32:
            _same(_query(rt2mod, scene, path, o[:32], d[:32]), want[k][:32], f"pickets({n}) chunk {k}[:32] {path}")


@pytest.mark.parametrize("arm", range(1, 11))
def test_exit_logic_of_the_experiment_arms(rt2mod, oraclemod, arm):
    """The A/B arms of occluded_k5r (experiment build only: RT2_LIB=exp) on the
    picket chunks and the 1,217 soup's 1,025 rays, unbounded and bounded."""
    if not hasattr(rt2mod.lib(), "rt2_scene_set_occluded_arm"):
        pytest.skip("the A/B arms are in the experiment build")
    for n in O.PICKETS:
        ch = O.chunks(n)
        scene = rt2mod.Scene(triangles=O.pickets(n), materials=S.code_materials(n))
        try:
            assert rt2mod.lib().rt2_scene_set_occluded_arm(scene._p, arm) == 0
            for tail in O.RAGGED:
                names = O.FULL + (tail,)
                o, d = O._cat(*[ch[k][:2] for k in names])
                want = np.concatenate([ch[k][2] >= 0 for k in names])
                _same(_query(rt2mod, scene, "auto", o, d), want, f"arm {arm} pickets({n}) +{tail}")
            for k in ch:
                o, d, claim = ch[k]
                _same(_query(rt2mod, scene, "auto", o[:32], d[:32]), claim[:32] >= 0, f"arm {arm} pickets({n}) {k}[:32]")
        finally:
            scene.close()
    o, d, hit, dst = _soup1217(oraclemod)
    scene = rt2mod.Scene(triangles=T.scene_tris("soup", 1217), materials=S.code_materials(1217))
    try:
        assert rt2mod.lib().rt2_scene_set_occluded_arm(scene._p, arm) == 0
        _same(_query(rt2mod, scene, "auto", o, d), hit, f"arm {arm} soup")
        for name, tmax, want in O.bound_cases(dst, hit)[:3]:
            _same(_query(rt2mod, scene, "auto", o, d, tmax), want, f"arm {arm} soup {name}")
    finally:
        scene.close()


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("n", (1, 33, 65))
def test_device_form_on_a_stream(rt2mod, oraclemod, n, path):
    """n + 64 bytes prefilled with 0xAA at an odd address: the results are 0 or
    1, the 64 bytes after them and the byte before them are untouched."""
    import torch
    o, d, occ, _ = (a[:n] for a in _soup1217(oraclemod))
    rays = np.zeros(n, rt2mod.RAY_DTYPE)
    rays["o"], rays["d"] = o, d
    scene, _ = _scene(rt2mod, "soup", 1217)
    flags = rt2mod.TRACE_SCALAR if path == "scalar" else rt2mod.TRACE_AUTO
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        d_rays = torch.from_numpy(rays.view(np.uint8).copy()).to("cuda")
        d_out = torch.full((1 + n + 64,), 0xAA, dtype=torch.uint8, device="cuda")
        st.synchronize()
        scene.occluded_device(d_rays.data_ptr(), n, d_out.data_ptr() + 1, flags, st.cuda_stream)
        st.synchronize()
    assert scene.last_kernel() == _expected_kernel(rt2mod, scene, path)
    out = d_out.cpu().numpy()
    assert out[0] == 0xAA and (out[1 + n:] == 0xAA).all()
    assert np.isin(out[1:1 + n], (0, 1)).all()
    _same(out[1:1 + n].astype(bool), occ, f"device form {n} {path}")


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("order", T.FAN_ORDERS)
def test_fans(rt2mod, oraclemod, order, path):
    """64 triangles all accepted by every ray: every ray is occluded."""
    o, d = O.fan_rays(order)
    scene, _ = _scene(rt2mod, "fan_" + order, 64)
    want = O.occluded_ref(oraclemod, T.scene_tris("fan_" + order, 64), o, d)[0]
    assert want.all()
    _same(_query(rt2mod, scene, path, o, d), want, f"fan {order} {path}")


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
    """One 64-ray chunk of ordinary rays with a far origin, an unnormalised
    direction, a NaN origin, an infinite direction component (each alone, then
    all four): a non-finite ray is unoccluded and the others are undisturbed."""
    o, d = _mixed_rays(oraclemod, which)
    want = O.occluded_ref(oraclemod, T.scene_tris("soup", 1217), o, d)[0]
    base = _soup1217(oraclemod)[2][:64]
    assert want.sum() >= 16 and not want[[l for l in MIXED[which] if l in (41, 50)]].any()
    others = np.setdiff1d(np.arange(64), MIXED[which])
    assert np.array_equal(want[others], base[others])
    scene, _ = _scene(rt2mod, "soup", 1217)
    _same(_query(rt2mod, scene, path, o, d), want, f"mixed {which} {path}")


@pytest.mark.parametrize("path", PATHS)
def test_scene_outside_the_filters_range(rt2mod, oraclemod, path):
    """The 33-triangle soup with one vertex at 2^21 (beyond the matrix filter's
    |a| <= 2^20: that triangle's record always passes)."""
    o, d = T.scene_rays("far", 33, 193)
    want = O.occluded_ref(oraclemod, T.scene_tris("far", 33), o, d)[0]
    assert want.any() and (~want).any()
    scene, _ = _scene(rt2mod, "far", 33)
    _same(_query(rt2mod, scene, path, o, d), want, f"far {path}")


# ---- BVH -------------------------------------------------------------------------------------------------------

def _bvh_query(rt2mod, scene, o, d, tmax=None):
    scene.stats(reset=True)
    got = scene.occluded(o, d, tmax)
    assert scene.last_kernel() == rt2mod.OCCLUDED_BVH
    return got, scene.stats(reset=True)


@pytest.mark.parametrize("n", (1217, 8193))
def test_bvh_soups(rt2mod, oraclemod, n):
    nr = 193 if n == 1217 else 97
    o, d = T.scene_rays("soup", n, nr)
    scene, up = _scene(rt2mod, "soup", n, bvh=True)
    nodes = _nodes[("soup", n)]
    want, dst, tests, visits = O.occluded_ref(oraclemod, up, o, d, None, "bvh", nodes)
    assert want.sum() >= 24 and (~want).sum() >= 8
    got, st = _bvh_query(rt2mod, scene, o, d)
    _same(got, want, f"bvh {n}")
    print(f"bvh {n}: leaf tests {st.tests} / {int(tests.sum())}, node visits {st.node_visits} / {int(visits.sum())}")
    assert st.segments == nr
    # every ray: never more than the closest-hit walk; strictly fewer where occluded rays stop at their first accept
    assert st.tests <= int(tests.sum()) and st.node_visits <= int(visits.sum())
    if n == 1217:
        assert st.tests < int(tests.sum()) and st.node_visits < int(visits.sum())
    # only the unoccluded rays: their walk is the closest-hit walk, to the end
    u = ~want
    got, st = _bvh_query(rt2mod, scene, o[u], d[u])
    assert not got.any()
    assert st.segments == int(u.sum())
    assert st.tests == int(tests[u].sum()) and st.node_visits == int(visits[u].sum())
    # bounds by turns one ulp above the hit (occluded), halfway to it (not) and none
    i = np.arange(nr)
    tmax = np.select([want & (i % 3 == 0), want & (i % 3 == 1)],
                     [np.nextafter(dst, F32(np.inf)), dst * F32(0.5)], F32(0)).astype(F32)
    bounded = O.occluded_ref(oraclemod, up, o, d, tmax, "bvh", nodes)[0]
    assert np.array_equal(bounded, want & (i % 3 != 1))
    _same(_bvh_query(rt2mod, scene, o, d, tmax)[0], bounded, f"bvh {n} bounded")


_edge_scenes = {}


@pytest.mark.parametrize("sc", E.query_scenes(), ids=[s.name for s in E.query_scenes()])
def test_bvh_edge_scenes(rt2mod, oraclemod, sc):
    """The hand-built trees of tests/bvh_edge_scenes.py against the oracle's own
    walk (the array scan is no reference there), without bounds and with
    bounded_tmax's."""
    o, d, _ = E.query_rays(sc, 257)
    if sc.name not in _edge_scenes:
        scene = rt2mod.Scene(triangles=sc.tris, materials=sc.mats, nodes=sc.nodes)
        scene.set_traversal("bvh")
        _edge_scenes[sc.name] = scene
    scene = _edge_scenes[sc.name]
    ref = oraclemod.closest_hits(sc.tris, o, d, None, "bvh", sc.nodes)
    for what, tmax in (("unbounded", None), ("bounded", E.bounded_tmax(sc, o, d, ref[0], ref[1]))):
        want, _, tests, visits = O.occluded_ref(oraclemod, sc.tris, o, d, tmax, "bvh", sc.nodes)
        got, st = _bvh_query(rt2mod, scene, o, d, tmax)
        _same(got, want, f"{sc.name} {what}")
        assert st.segments == len(o)
        assert st.tests <= int(tests.sum()) and st.node_visits <= int(visits.sum())
        u = ~want
        if u.any():
            got, st = _bvh_query(rt2mod, scene, o[u], d[u], None if tmax is None else tmax[u])
            assert not got.any()
            assert st.tests == int(tests[u].sum()) and st.node_visits == int(visits[u].sum()), f"{sc.name} {what}"


# ---- stats, other launches -------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", PATHS)
def test_stats(rt2mod, oraclemod, path):
    """Brute force: tests is the nominal segments * N."""
    o, d = (a[:193] for a in _soup1217(oraclemod)[:2])
    scene, _ = _scene(rt2mod, "soup", 1217)
    scene.stats(reset=True)
    _query(rt2mod, scene, path, o, d)
    st = scene.stats(reset=True)
    assert st.segments == 193 and st.tests == 193 * 1217 and st.node_visits == 0


def test_renders_and_trace_rays_unchanged(rt2mod, oraclemod):
    """Query, render, closest-hit query, occlusion queries, and again: the
    images and the hits have the same bits as before."""
    n = 1217
    tris, mats = S.coded_scene("soup", n)
    w, h = S.SIZES[n]
    u = S.coded_uniforms(w, h, n)
    scene = rt2mod.Scene(triangles=tris, materials=mats)
    try:
        o, d = (a[:193] for a in _soup1217(oraclemod)[:2])
        want = O.occluded_ref(oraclemod, tris, o, d)[0]
        before = scene.render_host(u, 0, 1)
        hits = scene.trace_rays(o, d)
        for path in PATHS:
            _same(_query(rt2mod, scene, path, o, d), want, path)
        after = scene.render_host(u, 0, 1)
        assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
        for path in PATHS:
            _same(_query(rt2mod, scene, path, o, d), want, path + " after the render")
        again = scene.trace_rays(o, d)
        assert np.array_equal(hits[0].view(np.uint32), again[0].view(np.uint32)) and np.array_equal(hits[1], again[1])
        _same(want, hits[1] >= 0, "the oracle against trace_rays")
    finally:
        scene.close()
