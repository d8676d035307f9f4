"""Preview shading queries (rt2_shade_rays, Scene.preview) on the GPU.  Every
comparison is by bits over every ray, of the colour and of the segment count.

  - against the oracle's traceBasic through one-pixel cameras (the rays are
    rt2_camera_rays_host's for the same uniforms), on the matrix kernel
    (resident and L2 forms), the scalar kernel and the BVH walk, each query
    asserting which kernel ran;
  - whole views through Scene.preview against oracle.render and
    Scene.render_host with basicShading = 1;
  - the deferred shadow sweep, the move of at most 32 live lanes, rays outside
    the filter's range or not finite among ordinary ones, tmax, the device
    form, the counters and side effects.

The scenes, rays and references are those of tests/shade_scenes.py;
tests/test_shade_cpu.py asserts on the oracle alone what they are built to
give.
"""
import numpy as np
import pytest

import closest_hit_scenes as S
import shade_scenes as H
import surface_model as M
import trace_rays_lib as T
from test_shade_cpu import preview_uniforms

pytestmark = pytest.mark.gpu

F32 = np.float32
ARMS = ("auto", "scalar", "bvh")
SENTINEL = 0xAB

_gpu = {}


def _scene(rt2mod, sc, arm):
    """(scene, triangles as uploaded, nodes or None), made once per scene and traversal."""
    key = (sc["name"].split("/")[0], arm == "bvh")
    if key not in _gpu:
        if arm == "bvh":
            sd = S.scene_data(sc["triangles"], sc["materials"])
            scene = rt2mod.Scene(sd)
            scene.set_traversal("bvh")
            up, nodes = sd.triangles().copy(), sd.nodes().copy()
        else:
            scene, up, nodes = rt2mod.Scene(triangles=sc["triangles"], materials=sc["materials"]), sc["triangles"], None
        if sc["textures"]:
            scene.set_textures(sc["textures"])
        _gpu[key] = (scene, up, nodes)
    return _gpu[key]


def _expected_kernel(rt2mod, scene, arm):
    if arm == "bvh":
        return rt2mod.SHADE_BVH
    if arm == "scalar":
        return rt2mod.SHADE_SCALAR
    return rt2mod.SHADE_RES if scene.n_tris <= 38 * 32 else rt2mod.SHADE_RES_L2


def _flags(rt2mod, arm):
    return rt2mod.TRACE_SCALAR if arm == "scalar" else rt2mod.TRACE_AUTO


def _shade(rt2mod, scene, arm, o, d, light, shadow, mb):
    rec = scene.shade_rays(o, d, light, bool(shadow), mb, _flags(rt2mod, arm))
    assert scene.last_kernel() == _expected_kernel(rt2mod, scene, arm), arm
    assert rec.dtype == rt2mod.SHADED_DTYPE and len(rec) == len(o)
    return rec


_dirs = {}


def _device_dirs(rt2mod, scene, sc):
    """d of every ray of the scene from rt2_camera_rays_host through its
    one-pixel camera: the preview's own normalize(viewportFront), bit for bit."""
    key = sc["name"]
    if key not in _dirs:
        d = np.zeros((len(sc["o"]), 3), F32)
        for i in range(len(d)):
            u = H.one_pixel_uniforms(rt2mod, sc["o"][i], sc["f"][i], 1, sc["light"], 0, 1, 0)
            rays = scene.camera_rays(u)
            assert len(rays) == 4 and np.array_equal(rays["o"][3], sc["o"][i])
            d[i] = rays["d"][3]  # pixel (1, 1): px = py = 0
        d.setflags(write=False)
        _dirs[key] = d
    return _dirs[key]


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _check(rec, rgb, segs, what):
    bad = (_bits(rec["rgb"]) != _bits(rgb)).any(1) | (rec["segments"] != segs)
    if bad.any():
        lines = [f"ray {i}: GPU {rec['rgb'][i]} in {rec['segments'][i]} segments, reference {rgb[i]} in {segs[i]}"
                 for i in np.flatnonzero(bad)[:6]]
        raise AssertionError(f"{what}: {int(bad.sum())} of {len(bad)} rays differ\n" + "\n".join(lines))


# ---- against the oracle through one-pixel cameras ---------------------------------------------------------------

@pytest.mark.parametrize("arm", ARMS)
@pytest.mark.parametrize("name", list(H.ORACLE_SCENES))
def test_against_the_oracle(rt2mod, oraclemod, name, arm):
    """1 triangle; the diverse Cornell box with a checker floor, textures of 3
    and 1 channels, a highlight sheet and an unknown type; the mirror corridor;
    1,216 triangles (all resident) and 1,217 (the last group from L2); 1, 63,
    64, 65 and 1,025 rays, with and without the shadow ray, 1, 3 and 8 bounces."""
    sc = H.ORACLE_SCENES[name]()
    scene, up, nodes = _scene(rt2mod, sc, arm)
    d = _device_dirs(rt2mod, scene, sc)
    for shadow, mb in H.SETTINGS:
        rgb, segs = H.oracle_shade(oraclemod, rt2mod, sc, shadow, mb, "bvh" if arm == "bvh" else "brute",
                                   up if arm == "bvh" else None, nodes)
        for k in H.RAY_COUNTS:
            rec = _shade(rt2mod, scene, arm, sc["o"][:k], d[:k], sc["light"], shadow, mb)
            _check(rec, rgb[:k], segs[:k], f"{name} {arm} shadow {shadow} max_bounce {mb}, {k} rays")
    if name == "soup1217" and arm == "auto":
        assert scene.last_kernel() == rt2mod.SHADE_RES_L2
    if name == "soup1216" and arm == "auto":
        assert scene.last_kernel() == rt2mod.SHADE_RES


def test_arms_agree(rt2mod):
    """The matrix and the scalar kernel give the same bytes (the brute-force scan has one answer)."""
    for name in ("cornell", "corridor", "soup1217"):
        sc = H.ORACLE_SCENES[name]()
        scene, _, _ = _scene(rt2mod, sc, "auto")
        d = _device_dirs(rt2mod, scene, sc)
        a = _shade(rt2mod, scene, "auto", sc["o"], d, sc["light"], 1, 8)
        b = _shade(rt2mod, scene, "scalar", sc["o"], d, sc["light"], 1, 8)
        assert a.tobytes() == b.tobytes(), name


# ---- whole views ------------------------------------------------------------------------------------------------

VIEW_ARMS = {"res": (0, "auto"), "res_l2": (1217, "auto"), "scalar": (0, "scalar"), "bvh": (0, "bvh")}


def _view(rt2mod, w, h, cam, which):
    total, arm = VIEW_ARMS[which]
    sc = M.view_scene(w, h, cam, total)
    gs = dict(name=f"view{total}", triangles=sc["triangles"], materials=sc["materials"], textures=M.view_textures())
    scene, up, nodes = _scene(rt2mod, gs, arm)
    return sc, scene, up, nodes, arm


@pytest.mark.parametrize("which", list(VIEW_ARMS))
@pytest.mark.parametrize("cam", M.VIEW_CAMERAS)
@pytest.mark.parametrize("w,h", M.VIEW_SIZES)
def test_preview_views(rt2mod, oraclemod, w, h, cam, which):
    sc, scene, up, nodes, arm = _view(rt2mod, w, h, cam, which)
    u = preview_uniforms(rt2mod, sc)
    img = scene.preview(u, None, _flags(rt2mod, arm))
    assert scene.last_kernel() == _expected_kernel(rt2mod, scene, arm)
    assert img.shape == (h, w, 4) and img.dtype == F32 and (img[..., 3] == 1).all()
    oraclemod.set_textures(M.view_textures())
    try:
        acc, _, segs, _ = oraclemod.render(up, sc["materials"], u, np.arange(h, dtype=np.int32), 0, 1,
                                           "bvh" if nodes is not None else "brute", nodes=nodes)
    finally:
        oraclemod.set_textures([])
    assert np.array_equal(_bits(img[..., :3]), _bits(acc[..., :3])), f"{which}: preview against the oracle"
    scene.stats(reset=True)
    ren = scene.render_host(u, 0, 1)
    rs = scene.stats(reset=True)
    assert rs.segments == segs
    assert np.array_equal(_bits(img), _bits(ren)), f"{which}: preview against render_host"
    scene.preview(u, None, _flags(rt2mod, arm))
    qs = scene.stats(reset=True)
    assert (qs.segments, qs.tests) == (segs, rs.tests)  # what render_basic adds per pixel and frame
    assert (qs.node_visits > 0) == (arm == "bvh")


def test_preview_of_a_shard(rt2mod):
    """Shard {2, 1, 3} of the 67 x 10 view: the whole view's rows 2, 3, 8, 9."""
    sc, scene, _, _, _ = _view(rt2mod, 67, 10, M.VIEW_CAMERAS[1], "res")
    u = preview_uniforms(rt2mod, sc)
    whole = scene.preview(u)
    part = scene.preview(u, rt2mod.shard(2, 1, 3))
    assert part.shape == (4, 67, 4)
    assert np.array_equal(_bits(part), _bits(whole[[2, 3, 8, 9]]))
    assert np.array_equal(_bits(part), _bits(scene.render_host(u, 0, 1, rt2mod.shard(2, 1, 3))))


# ---- the deferred shadow sweep, the move to lanes 0..31 -------------------------------------------------------------

def _corridor_chunk(rt2mod, oraclemod, idx, arm, shadow, mb=8):
    sc = H.corridor()
    scene, _, _ = _scene(rt2mod, sc, arm)
    sub = dict(sc, name="corridor/picked", o=sc["o"][idx], f=sc["f"][idx])
    _dirs.pop("corridor/picked", None)
    d = _device_dirs(rt2mod, scene, sub)
    rgb, segs = H.oracle_shade(oraclemod, rt2mod, sc, shadow, mb)
    rec = _shade(rt2mod, scene, arm, sub["o"], d, sc["light"], shadow, mb)
    _check(rec, rgb[idx], segs[idx], f"corridor chunk {arm} shadow {shadow}")
    return rec


@pytest.mark.parametrize("arm", ("auto", "scalar"))
def test_deferred_shadow_sweep(rt2mod, oraclemod, arm):
    """Three chunks in one call: patch ends at bounces 1, 2 and 3 with the
    light hidden for half of each class; exactly one waiting lane; none, with
    the shadow ray on and every ray ending on the light or in the sky."""
    first, second, third = H.shadow_chunks(oraclemod, rt2mod)
    rec = _corridor_chunk(rt2mod, oraclemod, np.concatenate([first, second, third]), arm, 1)
    ends, occ, _, seg0 = H.corridor_classes(oraclemod, rt2mod)
    idx = np.concatenate([first, second, third])
    assert np.array_equal(rec["segments"], seg0[idx] + (ends[idx] > 0))  # one more search where a lane waited
    assert (ends[idx] > 0).sum() == 60 + 1
    # each of the chunks alone: the same records
    for k, idx in enumerate((first, second, third)):
        alone = _corridor_chunk(rt2mod, oraclemod, idx, arm, 1)
        assert alone.tobytes() == rec[64 * k:64 * k + 64].tobytes(), k


@pytest.mark.parametrize("arm", ("auto", "scalar"))
@pytest.mark.parametrize("shadow", (0, 1))
def test_at_most_32_live_lanes(rt2mod, oraclemod, arm, shadow):
    """40 rays of a chunk end at bounce 1 and the 24 that go on sit in lanes 40
    to 63: they are moved to lanes 0 .. 23, and every record lands at its own
    index."""
    idx = H.compaction_chunk(oraclemod, rt2mod)
    rec = _corridor_chunk(rt2mod, oraclemod, idx, arm, shadow)
    assert (rec["segments"][:40] <= 1 + shadow).all()
    assert (rec["segments"][40:] >= 3).all()
    # and behind a full chunk, in the second wave's place
    both = _corridor_chunk(rt2mod, oraclemod, np.concatenate([np.arange(64), idx]), arm, shadow)
    assert both[64:].tobytes() == rec.tobytes()


# ---- rays outside the filter's range or not finite among ordinary ones ---------------------------------------

MIXED = {"far": (5,), "long": (40,), "nan": (41,), "inf": (50,), "all": (5, 40, 41, 50)}


def _mixed_rays(which):
    """Two chunks of the 1,217-triangle soup's rays; in the first, lane 5 far
    outside the filter's range (2^21), lane 40 unnormalised, lane 41 a NaN
    origin, lane 50 an infinite direction component."""
    sc = H.soup(1217)
    o, d = sc["o"][:128].copy(), sc["f"][:128].copy()
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
def test_mixed_waves(rt2mod, which, arm):
    sc = H.soup(1217)
    scene, _, _ = _scene(rt2mod, sc, arm)
    base = _shade(rt2mod, scene, arm, sc["o"][:128], sc["f"][:128], sc["light"], 1, 8)
    o, d = _mixed_rays(which)
    rec = _shade(rt2mod, scene, arm, o, d, sc["light"], 1, 8)
    others = np.setdiff1d(np.arange(128), MIXED[which])
    assert (base["segments"][others] >= 2).sum() >= 32
    assert np.array_equal(rec[others].view(np.uint8), base[others].view(np.uint8))  # undisturbed, every byte
    # both kernels: equal where both are numbers, NaN in the same components
    other = scene.shade_rays(o, d, sc["light"], True, 8, _flags(rt2mod, "scalar" if arm == "auto" else "auto"))
    assert np.array_equal(rec["segments"], other["segments"])
    nan_a, nan_b = np.isnan(rec["rgb"]), np.isnan(other["rgb"])
    assert np.array_equal(nan_a, nan_b)
    assert np.array_equal(_bits(rec["rgb"])[~nan_a], _bits(other["rgb"])[~nan_a])


def test_tmax_is_not_used(rt2mod):
    """tmax = 0, half the primary hit distance and a NaN: identical records."""
    import torch
    sc = H.soup(1217)
    n = 193
    for arm in ("auto", "scalar"):
        scene, _, _ = _scene(rt2mod, sc, arm)
        dst, tri = scene.trace_rays(sc["o"][:n], sc["f"][:n])
        assert (tri >= 0).sum() >= 48
        want = _shade(rt2mod, scene, arm, sc["o"][:n], sc["f"][:n], sc["light"], 1, 8)
        for tmax in (np.zeros(n, F32), np.where(tri >= 0, dst * F32(0.5), F32(0.25)).astype(F32),
                     np.full(n, np.nan, F32)):
            rays = np.zeros(n, rt2mod.RAY_DTYPE)
            rays["o"], rays["d"], rays["tmax"] = sc["o"][:n], sc["f"][:n], tmax
            d_rays = torch.from_numpy(rays.view(np.uint8).copy()).to("cuda")
            d_out = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            scene.shade_rays_device(d_rays.data_ptr(), n, d_out.data_ptr(), sc["light"], True, 8, _flags(rt2mod, arm),
                                    torch.cuda.current_stream().cuda_stream)
            assert d_out.cpu().numpy().tobytes() == want.tobytes(), arm


# ---- device form, counters, side effects --------------------------------------------------------------------------

@pytest.mark.parametrize("arm", ARMS)
def test_device_form_guard_region_and_stats(rt2mod, arm):
    """rt2_shade_rays on a non-default stream with torch tensors: the host
    form's bytes; nothing before record 0 or after record n is written, n = 0
    writes nothing, and stats().segments is the sum of the records'."""
    import torch
    n, guard = 193, 5
    sc = H.soup(1217)
    scene, _, _ = _scene(rt2mod, sc, arm)
    rays = np.zeros(n, rt2mod.RAY_DTYPE)
    rays["o"], rays["d"] = sc["o"][:n], sc["f"][:n]
    host = _shade(rt2mod, scene, arm, sc["o"][:n], sc["f"][:n], sc["light"], 1, 8)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        d_rays = torch.from_numpy(rays.view(np.uint8).copy()).to("cuda", non_blocking=False)
        d_buf = torch.full(((n + 2 * guard) * 16,), SENTINEL, dtype=torch.uint8, device="cuda")
        d_out = d_buf[guard * 16:]
        st.synchronize()
        scene.shade_rays_device(d_rays.data_ptr(), 0, d_out.data_ptr(), sc["light"], True, 8, _flags(rt2mod, arm),
                                st.cuda_stream)
        st.synchronize()
        assert (d_buf.cpu().numpy() == SENTINEL).all()
        for k in (1, 65, n):
            d_buf.fill_(SENTINEL)
            st.synchronize()
            scene.stats(reset=True)
            scene.shade_rays_device(d_rays.data_ptr(), k, d_out.data_ptr(), sc["light"], True, 8, _flags(rt2mod, arm),
                                    st.cuda_stream)
            st.synchronize()
            assert scene.last_kernel() == _expected_kernel(rt2mod, scene, arm)
            got = d_buf.cpu().numpy()
            assert (got[:guard * 16] == SENTINEL).all(), k
            assert got[guard * 16:(guard + k) * 16].tobytes() == host[:k].tobytes(), k
            assert (got[(guard + k) * 16:] == SENTINEL).all(), k
            stats = scene.stats(reset=True)
            assert stats.segments == int(host["segments"][:k].sum()), k
            if arm == "bvh":
                assert 0 < stats.tests < stats.segments * 1217 and stats.node_visits > 0
            else:
                assert stats.tests == stats.segments * 1217 and stats.node_visits == 0


def test_render_unchanged_by_queries(rt2mod):
    """One index-coded image before the queries and one after them on the same scene: identical bits."""
    n = 1217
    tris, mats = S.coded_scene("soup", n)
    w, h = S.SIZES[n]
    u = S.coded_uniforms(w, h, n)
    scene = rt2mod.Scene(triangles=tris, materials=mats)
    before = scene.render_host(u, 0, 1)
    sc = H.soup(n)
    a = scene.shade_rays(sc["o"][:193], sc["f"][:193], sc["light"], True, 8)
    b = scene.shade_rays(sc["o"][:193], sc["f"][:193], sc["light"], True, 8, rt2mod.TRACE_SCALAR)
    assert a.tobytes() == b.tobytes() and (a["segments"] >= 1).all() and np.isfinite(a["rgb"]).all()
    scene.preview(u)
    after = scene.render_host(u, 0, 1)
    assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
