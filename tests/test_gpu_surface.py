"""Surface queries (rt2_surface_rays, rt2_camera_rays, Scene.feature_buffers)
on the GPU.

  - (dst, tri) by bits against oracle.closest_hits and Scene.trace_rays, on
    the matrix kernel (resident and L2 forms), the scalar kernel and the BVH
    walk; every query asserts which kernel ran;
  - mtl, mtl_type against the uploaded arrays; the normal with one bit pattern
    per triangle, facing the ray, and within the float64 model's bound; u, v
    with the three sign conditions exact in binary32 and within the model's
    bound; the base colour exactly, for caller's rays on the materials whose
    colour is a function of the material alone, and for every material type
    through Scene.feature_buffers against the oracle's preview render;
  - camera rays against the model, shards, rays outside the filter's range or
    not finite among ordinary ones, bounds, and side effects.

The scenes, rays and the model are those of tests/surface_model.py;
tests/test_surface_cpu.py asserts on the oracle and the model alone what they
are built to give.
"""
import numpy as np
import pytest

import closest_hit_scenes as S
import shading_scenes as ss
import surface_model as M
import trace_rays_lib as T
from test_shading_model import to_uniforms

pytestmark = pytest.mark.gpu

F32 = np.float32
ARMS = ("auto", "scalar", "bvh")
SENTINEL = 0xAB

_scenes = {}


def _make(rt2mod, key, tris, mats, bvh, textures=None):
    """(scene, triangles as uploaded, nodes or None), made once per key."""
    if key not in _scenes:
        if bvh:
            sd = S.scene_data(tris, mats)
            scene = rt2mod.Scene(sd)
            scene.set_traversal("bvh")
            up, nodes = sd.triangles().copy(), sd.nodes().copy()
            up.setflags(write=False)
        else:
            scene, up, nodes = rt2mod.Scene(triangles=tris, materials=mats), tris, None
        if textures:
            scene.set_textures(textures)
        _scenes[key] = (scene, up, nodes)
    return _scenes[key]


def _hit_scene(rt2mod, kind, n, arm):
    mats = M.pure_materials(n)
    return _make(rt2mod, (kind, n, arm == "bvh"), T.scene_tris(kind, n), mats, arm == "bvh") + (mats,)


def _fat_scene(rt2mod, arm):
    tris = M.fat_triangles()
    mats = M.pure_materials(len(tris))
    return _make(rt2mod, ("fat", arm == "bvh"), tris, mats, arm == "bvh") + (mats,)


def _expected_kernel(rt2mod, scene, arm):
    if arm == "bvh":
        return rt2mod.SURFACE_BVH
    if arm == "scalar":
        return rt2mod.SURFACE_SCALAR
    return rt2mod.SURFACE_RES if scene.n_tris <= 38 * 32 else rt2mod.SURFACE_RES_L2


def _flags(rt2mod, arm):
    return rt2mod.TRACE_SCALAR if arm == "scalar" else rt2mod.TRACE_AUTO


def _surface(rt2mod, scene, arm, o, d, tmax=None):
    rec = scene.surface(o, d, tmax, _flags(rt2mod, arm))
    assert scene.last_kernel() == _expected_kernel(rt2mod, scene, arm), arm
    assert rec.dtype == rt2mod.SURFACE_DTYPE and len(rec) == len(o)
    return rec


def _oracle_hits(oraclemod, up, nodes, o, d, bound=None):
    dst, tri, _, _ = oraclemod.closest_hits(up, o, d, bound, "bvh" if nodes is not None else "brute", nodes)
    return dst, tri


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _check_hit_record(rec, dst, tri, what):
    bad = (_bits(rec["dst"]) != _bits(dst)) | (rec["tri"] != tri)
    if bad.any():
        lines = [f"ray {i}: GPU ({rec['dst'][i]!r}, {rec['tri'][i]}), reference ({dst[i]!r}, {tri[i]})"
                 for i in np.flatnonzero(bad)[:6]]
        raise AssertionError(f"{what}: {int(bad.sum())} of {len(bad)} rays differ\n" + "\n".join(lines))


def _check_records(rec, up, mats, d, bound, what, pure=True):
    """Everything about the records that needs no reference beyond the uploaded arrays."""
    hit = rec["tri"] >= 0
    miss = ~hit
    # a miss: three -1, dst = bound, eight floats of +0.0
    assert (rec["tri"][miss] == -1).all() and (rec["mtl"][miss] == -1).all() and (rec["mtl_type"][miss] == -1).all()
    assert np.array_equal(_bits(rec["dst"][miss]), _bits(np.broadcast_to(bound, hit.shape)[miss])), what
    for f in ("normal", "u", "albedo", "v"):
        assert not _bits(rec[f][miss]).any(), f"{what}: {f} of a miss is not +0.0"
    # a hit
    t = rec["tri"][hit]
    assert np.array_equal(rec["mtl"][hit], up["materialIndex"][t]), what
    assert np.array_equal(rec["mtl_type"][hit], mats["materialType"][rec["mtl"][hit]]), what
    nb = _bits(rec["normal"][hit])
    first = {}
    for k, i in enumerate(t):
        assert (nb[k] == first.setdefault(int(i), nb[k])).all(), f"{what}: two normals for triangle {i}"
    facing = (rec["normal"][hit].astype(np.float64) * np.asarray(d, np.float64)[hit]).sum(1)
    assert (facing < 0).all(), what
    u, v = rec["u"][hit], rec["v"][hit]
    assert u.dtype == F32 and (u >= 0).all() and (v >= 0).all() and (F32(1) - u - v >= 0).all(), what
    if pure:
        want = M.pure_albedo(mats)[rec["mtl"][hit]]
        assert np.array_equal(_bits(rec["albedo"][hit]), _bits(want)), what
    return hit


# ---- (dst, tri), materials, pure colours -----------------------------------------------------------------------

@pytest.mark.parametrize("arm", ARMS)
@pytest.mark.parametrize("kind,n", M.HIT_SCENES)
def test_hit_records(rt2mod, oraclemod, kind, n, arm):
    """1 triangle; 33 with a vertex at 2^21; 1,216 (38 groups, all resident);
    1,217 (the last group from L2, with closest hits in it); 1, 63, 64, 65 and
    1,025 rays each."""
    scene, up, nodes, mats = _hit_scene(rt2mod, kind, n, arm)
    o, d = M.hit_scene_rays(kind, n)
    dst, tri = _oracle_hits(oraclemod, up, nodes, o, d)
    for k in M.RAY_COUNTS:
        rec = _surface(rt2mod, scene, arm, o[:k], d[:k])
        _check_hit_record(rec, dst[:k], tri[:k], f"{kind} {n} {arm}, {k} rays")
        gd, gt = scene.trace_rays(o[:k], d[:k], None, _flags(rt2mod, arm))
        _check_hit_record(rec, gd, gt, f"{kind} {n} {arm}, {k} rays against trace_rays")
        _check_records(rec, up, mats, d[:k], T.UNBOUNDED, f"{kind} {n} {arm}, {k} rays")
    if n == 1217 and arm != "bvh":
        assert (rec["tri"] >= 1216).sum() >= 8
    assert (rec["tri"] >= 0).any()
    if n >= 12:
        assert set(rec["mtl_type"][rec["tri"] >= 0].tolist()) == set(M.PURE_TYPES)


@pytest.mark.parametrize("arm", ARMS)
@pytest.mark.parametrize("which", ["soup1216", "soup1217", "fat"])
def test_normals_against_model(rt2mod, oraclemod, which, arm):
    if which == "fat":
        scene, up, nodes, mats = _fat_scene(rt2mod, arm)
        o, d = M.fat_rays()
    else:
        n = int(which[4:])
        scene, up, nodes, mats = _hit_scene(rt2mod, "soup", n, arm)
        o, d = M.hit_scene_rays("soup", n)
    rec = _surface(rt2mod, scene, arm, o, d)
    hit = rec["tri"] >= 0
    model, tol = M.unit_normals(up)
    t = rec["tri"][hit]
    assert len(np.unique(t)) >= 20 and tol[t].max() < M.MAX_TOL
    err = np.abs(rec["normal"][hit].astype(np.float64) - model[t]).max(1)
    print(f"{which} {arm}: worst normal error {err.max():.3e}, its bound {tol[t][err.argmax()]:.3e}, "
          f"largest error / bound {(err / tol[t]).max():.3f}")
    assert (err <= tol[t]).all()


@pytest.mark.parametrize("arm", ARMS)
def test_barycentrics_against_model(rt2mod, oraclemod, arm):
    scene, up, nodes, mats = _fat_scene(rt2mod, arm)
    o, d = M.fat_rays()
    rec = _surface(rt2mod, scene, arm, o, d)
    dst, tri = _oracle_hits(oraclemod, up, nodes, o, d)
    _check_hit_record(rec, dst, tri, f"fat {arm}")
    hit = _check_records(rec, up, mats, d, T.UNBOUNDED, f"fat {arm}")
    assert hit.sum() >= 64 and (~hit).sum() >= 64
    u, v, tol = M.barycentrics(up, rec["tri"][hit], o[hit], d[hit])
    assert tol.max() < M.MAX_TOL
    eu, ev = np.abs(rec["u"][hit] - u), np.abs(rec["v"][hit] - v)
    print(f"fat {arm}: worst u error {eu.max():.3e}, v error {ev.max():.3e}, smallest bound {tol.min():.3e}, "
          f"largest error / bound {max((eu / tol).max(), (ev / tol).max()):.3f}")
    assert (eu <= tol).all() and (ev <= tol).all()
    # the hit point from the barycentrics is the hit point from the distance
    a, b, c = (up[k][rec["tri"][hit], :3].astype(np.float64) for k in "abc")
    w = 1.0 - rec["u"][hit].astype(np.float64) - rec["v"][hit]
    p = w[:, None] * a + rec["u"][hit][:, None] * b + rec["v"][hit][:, None] * c
    q = o[hit].astype(np.float64) + d[hit].astype(np.float64) * rec["dst"][hit][:, None]
    assert np.abs(p - q).max() < 1e-4


# ---- feature buffers against the oracle's preview --------------------------------------------------------------

VIEW_ARMS = {"res": (0, "auto"), "res_l2": (1217, "auto"), "scalar": (0, "scalar"), "bvh": (0, "bvh")}
_view_refs = {}


def _view(rt2mod, w, h, cam, which):
    total, arm = VIEW_ARMS[which]
    sc = M.view_scene(w, h, cam, total)
    # the geometry does not depend on the view: one GPU scene per padding and traversal
    scene, up, nodes = _make(rt2mod, ("view", total, arm == "bvh"), sc["triangles"], sc["materials"], arm == "bvh",
                             M.view_textures())
    return sc, scene, up, nodes, arm


def _view_oracle(oraclemod, rt2mod, sc, up, nodes):
    """The oracle's preview image of a view (basicShading = 1, one bounce, no
    shadow, one frame), numTextures = the images bound; once per view and array."""
    key = (sc["name"], sc["uniforms"]["cameraPos"], nodes is not None)
    if key not in _view_refs:
        u = to_uniforms(rt2mod, sc["uniforms"])
        assert u.numTextures == len(M.view_textures()) and u.basicShading == 1 and u.maxBounceCount == 1
        assert u.basicShadingShadow == 0
        oraclemod.set_textures(M.view_textures())
        try:
            acc, _, _, _ = oraclemod.render(up, sc["materials"], u, np.arange(u.height, dtype=np.int32), 0, 1,
                                            "bvh" if nodes is not None else "brute", nodes=nodes)
        finally:
            oraclemod.set_textures([])
        img = np.ascontiguousarray(acc[..., :3])
        img.setflags(write=False)
        _view_refs[key] = img
    return _view_refs[key]


@pytest.mark.parametrize("which", list(VIEW_ARMS))
@pytest.mark.parametrize("cam", M.VIEW_CAMERAS)
@pytest.mark.parametrize("w,h", M.VIEW_SIZES)
def test_feature_buffers(rt2mod, oraclemod, w, h, cam, which):
    sc, scene, up, nodes, arm = _view(rt2mod, w, h, cam, which)
    mats = sc["materials"]
    u = to_uniforms(rt2mod, sc["uniforms"])
    u.numTextures = 6  # not consulted: a surface query takes the number of images bound
    fb = scene.feature_buffers(u, None, _flags(rt2mod, arm))
    assert scene.last_kernel() == _expected_kernel(rt2mod, scene, arm)
    assert {k: v.shape for k, v in fb.items()} == {
        "depth": (h, w), "tri": (h, w), "mtl": (h, w), "mtl_type": (h, w), "normal": (h, w, 3), "albedo": (h, w, 3),
        "uv": (h, w, 2)}
    # the records are those of the device's own camera rays
    rays = scene.camera_rays(u)
    o, d = np.ascontiguousarray(rays["o"]), np.ascontiguousarray(rays["d"])
    rec = _surface(rt2mod, scene, arm, o, d)
    for name, field in (("depth", "dst"), ("tri", "tri"), ("mtl", "mtl"), ("mtl_type", "mtl_type"),
                        ("normal", "normal"), ("albedo", "albedo")):
        assert np.array_equal(fb[name].reshape(-1).view(np.uint32), rec[field].reshape(-1).view(np.uint32)), name
    assert np.array_equal(_bits(fb["uv"][..., 0]).reshape(-1), _bits(rec["u"]))
    assert np.array_equal(_bits(fb["uv"][..., 1]).reshape(-1), _bits(rec["v"]))
    dst, tri = _oracle_hits(oraclemod, up, nodes, o, d)
    _check_hit_record(rec, dst, tri, f"view {which}")
    hit = _check_records(rec, up, mats, d, T.UNBOUNDED, f"view {which}", pure=False)
    assert (~hit).sum() >= 16
    for t in M.TYPES:
        assert (rec["mtl_type"] == t).sum() >= 16, t
    # the base colour: the oracle's preview at hit pixels, exactly zero at misses (the oracle shows the sky there)
    ref = _view_oracle(oraclemod, rt2mod, sc, up, nodes).reshape(-1, 3)
    same = (_bits(rec["albedo"]) == _bits(ref)).all(1)
    if not same[hit].all():
        i = np.flatnonzero(hit & ~same)[0]
        raise AssertionError(f"view {which}: {int((hit & ~same).sum())} hit pixels differ from the oracle, first {i} "
                             f"(type {rec['mtl_type'][i]}): {rec['albedo'][i]} against {ref[i]}")
    assert (ref[~hit].max(1) > 0).all()
    # pure types once more through the view, and the texture rules by index
    is_pure = hit & np.isin(rec["mtl_type"], M.PURE_TYPES)
    lut = np.zeros((len(mats), 3), F32)
    pm = np.isin(mats["materialType"], M.PURE_TYPES)
    lut[pm] = M.pure_albedo(mats[pm])
    assert np.array_equal(_bits(rec["albedo"][is_pure]), _bits(lut[rec["mtl"][is_pure]]))
    ti = np.where(rec["mtl_type"] == ss.TEXTURE, mats["textureIndex"][np.maximum(rec["mtl"], 0)], -99)
    for index in (0, 1):
        assert (ti == index).any() and (rec["albedo"][ti == index].max(1) > 0).all()
    for index in (2, 7):
        assert (ti == index).any() and not _bits(rec["albedo"][ti == index]).any()
    # u, v and the normal against the model on the view's rays
    um, vm, tol = M.barycentrics(up, rec["tri"][hit], o[hit], d[hit])
    assert tol.max() < M.MAX_TOL
    assert (np.abs(rec["u"][hit] - um) <= tol).all() and (np.abs(rec["v"][hit] - vm) <= tol).all()
    nm, ntol = M.unit_normals(up)
    assert (np.abs(rec["normal"][hit] - nm[rec["tri"][hit]]).max(1) <= ntol[rec["tri"][hit]]).all()


# ---- camera rays ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cam", M.VIEW_CAMERAS)
@pytest.mark.parametrize("w,h", M.VIEW_SIZES)
def test_camera_rays(rt2mod, w, h, cam):
    sc, scene, _, _, _ = _view(rt2mod, w, h, cam, "res")
    scene.stats(reset=True)
    u = to_uniforms(rt2mod, sc["uniforms"])
    rays = scene.camera_rays(u)
    assert rays.dtype == rt2mod.RAY_DTYPE and len(rays) == w * h
    assert np.array_equal(_bits(rays["o"]), _bits(np.broadcast_to(np.array(cam, F32), (w * h, 3))))
    assert not _bits(rays["tmax"]).any() and not _bits(rays["pad"]).any()
    err = np.abs(rays["d"].astype(np.float64) - M.camera_dirs(sc["uniforms"]))
    print(f"{w}x{h} {cam}: worst direction error {err.max():.3e} against {M.CAMERA_TOL:.3e}")
    assert err.max() <= M.CAMERA_TOL
    assert scene.stats(reset=True).segments == 0  # camera rays do not count


def test_camera_rays_of_a_shard(rt2mod):
    """Shard {2, 1, 3} of the 67 x 10 view: the whole view's rows 2, 3, 8, 9."""
    sc, scene, _, _, _ = _view(rt2mod, 67, 10, M.VIEW_CAMERAS[1], "res")
    u = to_uniforms(rt2mod, sc["uniforms"])
    whole = scene.camera_rays(u).reshape(10, 67)
    part = scene.camera_rays(u, rt2mod.shard(2, 1, 3)).reshape(4, 67)
    assert np.array_equal(part.view(np.uint8), np.ascontiguousarray(whole[[2, 3, 8, 9]]).view(np.uint8))
    fb = scene.feature_buffers(u)
    fs = scene.feature_buffers(u, rt2mod.shard(2, 1, 3))
    for k in fb:
        assert np.array_equal(fs[k].view(np.uint32), np.ascontiguousarray(fb[k][[2, 3, 8, 9]]).view(np.uint32)), k


# ---- rays outside the filter's range, bounds -----------------------------------------------------------------

MIXED = {"far": (5,), "long": (40,), "nan": (41,), "inf": (50,), "all": (5, 40, 41, 50)}


def _mixed_rays(which):
    """Two chunks of the 1,217-triangle soup's rays; in the first, lane 5 far
    outside the filter's range, lane 40 unnormalised, lane 41 a NaN origin,
    lane 50 an infinite direction component."""
    o, d = (a[:128].copy() for a in M.hit_scene_rays("soup", 1217))
    for lane in MIXED[which]:
        if lane == 5:
            o[5] = (T.FAR, 5.0, 10.0)
        elif lane == 40:
            d[40] *= F32(3)
        elif lane == 41:
            o[41, 0] = np.nan
        else:
            d[50, 1] = np.inf
    return o, d


@pytest.mark.parametrize("arm", ("auto", "scalar"))
@pytest.mark.parametrize("which", list(MIXED))
def test_mixed_waves(rt2mod, oraclemod, which, arm):
    scene, up, nodes, mats = _hit_scene(rt2mod, "soup", 1217, arm)
    bo, bd = (a[:128] for a in M.hit_scene_rays("soup", 1217))
    base = _surface(rt2mod, scene, arm, bo, bd)
    o, d = _mixed_rays(which)
    rec = _surface(rt2mod, scene, arm, o, d)
    others = np.setdiff1d(np.arange(128), MIXED[which])
    assert (base["tri"][others] >= 0).sum() >= 32
    assert np.array_equal(rec[others].view(np.uint8), base[others].view(np.uint8))  # undisturbed, every byte
    for lane in MIXED[which]:
        if lane in (41, 50):  # not finite: the miss record
            want = np.zeros(1, rt2mod.SURFACE_DTYPE)
            want["dst"], want["tri"], want["mtl"], want["mtl_type"] = T.UNBOUNDED, -1, -1, -1
            assert rec[lane:lane + 1].tobytes() == want.tobytes(), lane
    dst, tri = _oracle_hits(oraclemod, up, nodes, o, d)
    _check_hit_record(rec, dst, tri, f"mixed {which} {arm}")
    finite = np.isfinite(o).all(1) & np.isfinite(d).all(1)
    _check_records(rec[finite], up, mats, d[finite], T.UNBOUNDED, f"mixed {which} {arm}")
    if 40 in MIXED[which]:  # three times as long a direction: the same triangle and normal at a third of the distance
        assert base["tri"][40] >= 0 and rec["tri"][40] == base["tri"][40] and rec["dst"][40] < base["dst"][40] * 0.34
        assert np.array_equal(_bits(rec["normal"][40]), _bits(base["normal"][40]))
    # both kernels give the same bytes, the special rays included
    other = scene.surface(o, d, None, _flags(rt2mod, "scalar" if arm == "auto" else "auto"))
    assert rec.tobytes() == other.tobytes()


@pytest.mark.parametrize("arm", ARMS)
def test_bounds(rt2mod, oraclemod, arm):
    scene, up, nodes, mats = _hit_scene(rt2mod, "soup", 1217, arm)
    o, d = (a[:193] for a in M.hit_scene_rays("soup", 1217))
    free = _surface(rt2mod, scene, arm, o, d)
    hit = free["tri"] >= 0
    assert hit.sum() >= 48 and (~hit).sum() >= 16
    # tmax = dst: the comparison is strict; the miss record with dst = tmax
    tmax = np.where(hit, free["dst"], F32(0)).astype(F32)
    rec = _surface(rt2mod, scene, arm, o, d, tmax)
    assert (rec["tri"] == -1).all()
    _check_records(rec, up, mats, d, T.bound_of(tmax), f"tmax = dst {arm}")
    assert np.array_equal(_bits(rec["dst"][hit]), _bits(free["dst"][hit]))
    # one ulp above: the same record, every byte
    tmax = np.where(hit, np.nextafter(free["dst"], F32(np.inf)), F32(0)).astype(F32)
    rec = _surface(rt2mod, scene, arm, o, d, tmax)
    assert rec.tobytes() == free.tobytes()
    dst, tri = _oracle_hits(oraclemod, up, nodes, o, d, T.bound_of(tmax))
    _check_hit_record(rec, dst, tri, f"tmax = nextafter(dst) {arm}")


# ---- side effects -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("arm", ARMS)
def test_stats(rt2mod, arm):
    scene, up, nodes, mats = _hit_scene(rt2mod, "soup", 1217, arm)
    o, d = (a[:193] for a in M.hit_scene_rays("soup", 1217))
    scene.stats(reset=True)
    _surface(rt2mod, scene, arm, o, d)
    st = scene.stats()
    assert st.segments == 193
    if arm == "bvh":
        assert 0 < st.tests < 193 * 1217 and st.node_visits > 0
    else:
        assert st.tests == 193 * 1217 and st.node_visits == 0
    _surface(rt2mod, scene, arm, o[:65], d[:65])
    assert scene.stats(reset=True).segments == 193 + 65
    # as rt2_trace_rays counts the same rays
    scene.trace_rays(o, d, None, _flags(rt2mod, arm))
    st2 = scene.stats(reset=True)
    assert (st2.segments, st2.tests, st2.node_visits) == (st.segments, st.tests, st.node_visits)


@pytest.mark.parametrize("arm", ARMS)
def test_device_form_and_guard_region(rt2mod, arm):
    """rt2_surface_rays on a non-default stream with torch tensors: the host
    form's bytes; nothing after record n is written, and n = 0 writes nothing."""
    import torch
    n, guard = 193, 5
    scene, up, nodes, mats = _hit_scene(rt2mod, "soup", 1217, arm)
    o, d = (a[:n] for a in M.hit_scene_rays("soup", 1217))
    rays = np.zeros(n, rt2mod.RAY_DTYPE)
    rays["o"], rays["d"] = o, d
    host = _surface(rt2mod, scene, arm, o, d)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        d_rays = torch.from_numpy(rays.view(np.uint8).copy()).to("cuda", non_blocking=False)
        d_out = torch.full(((n + guard) * 48,), SENTINEL, dtype=torch.uint8, device="cuda")
        st.synchronize()
        scene.surface_device(d_rays.data_ptr(), 0, d_out.data_ptr(), _flags(rt2mod, arm), st.cuda_stream)
        st.synchronize()
        assert (d_out.cpu().numpy() == SENTINEL).all()
        for k in (1, 65, n):
            d_out.fill_(SENTINEL)
            st.synchronize()
            scene.surface_device(d_rays.data_ptr(), k, d_out.data_ptr(), _flags(rt2mod, arm), st.cuda_stream)
            st.synchronize()
            assert scene.last_kernel() == _expected_kernel(rt2mod, scene, arm)
            got = d_out.cpu().numpy()
            assert got[:k * 48].tobytes() == host[:k].tobytes(), k
            assert (got[k * 48:] == SENTINEL).all(), k


def test_render_unchanged_by_queries(rt2mod, oraclemod):
    """One index-coded image before the queries and one after them on the same
    scene: identical bits."""
    n = 1217
    tris, mats = S.coded_scene("soup", n)
    w, h = S.SIZES[n]
    u = S.coded_uniforms(w, h, n)
    scene = rt2mod.Scene(triangles=tris, materials=mats)
    before = scene.render_host(u, 0, 1)
    o, d = (a[:193] for a in M.hit_scene_rays("soup", n))
    a = scene.surface(o, d)
    b = scene.surface(o, d, None, rt2mod.TRACE_SCALAR)
    assert a.tobytes() == b.tobytes() and (a["tri"] >= 0).any()
    scene.feature_buffers(u)
    after = scene.render_host(u, 0, 1)
    assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
    # and the queries' tri is the render's winner where the image decodes: the same scan
    dst, tri = _oracle_hits(oraclemod, tris, None, o, d)
    _check_hit_record(a, dst, tri, "coded scene")
