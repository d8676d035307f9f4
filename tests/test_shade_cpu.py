"""Preview shading queries without a GPU: the C-ABI's layouts, symbols and
argument checks, and the premises of tests/test_gpu_shade.py on the CPU oracle
alone (the one-pixel camera gives traceBasic for one ray; the ray sets reach
every branch of traceBasic; the chunks of the shadow, compaction and whole-view
tests hold what those tests say they hold), so none of them passes vacuously."""
import ctypes as C

import numpy as np
import pytest

import shade_scenes as H
import shading_scenes as ss
import surface_model as M
from test_shading_model import to_uniforms

F32 = np.float32


def test_layouts_and_symbols(rt2mod):
    s = rt2mod.SHADED_DTYPE
    assert s.itemsize == 16 and s.fields["rgb"][1] == 0 and s.fields["segments"][1] == 12  # one 16-byte store
    assert s.fields["rgb"][0].shape == (3,) and s.fields["segments"][0] == np.dtype("<i4")
    o = rt2mod.ShadeOpts
    assert C.sizeof(o) == 32 and (o.light.offset, o.shadow.offset, o.max_bounce.offset, o.pad.offset) == (0, 12, 16, 20)
    L = rt2mod.lib()
    assert L.rt2_abi_version() == 4  # the entry points only add to the interface
    for name in ("rt2_shade_rays", "rt2_shade_rays_host"):
        assert hasattr(L, name) and name in rt2mod.EXPORTED
    codes = (rt2mod.SHADE_RES, rt2mod.SHADE_RES_L2, rt2mod.SHADE_SCALAR, rt2mod.SHADE_BVH)
    assert codes == (-14, -15, -16, -17)  # the next four after the surface queries'
    assert min(rt2mod.SURFACE_RES, rt2mod.SURFACE_RES_L2, rt2mod.SURFACE_SCALAR, rt2mod.SURFACE_BVH) == -13
    for f in ("shade_rays", "shade_rays_device", "preview"):
        assert callable(getattr(rt2mod.Scene, f))


def _fake_scene():
    """Zeroed memory in place of a scene: brute-force traversal, no nodes, nothing on a device."""
    buf = C.create_string_buffer(4096)
    return buf, C.c_void_p(C.addressof(buf))


def test_argument_validation(rt2mod):
    """Every bad argument returns < 0 with "bad argument" before any device
    call (there is no device here; `fake` is no scene)."""
    L = rt2mod.lib()
    rays = np.zeros(4, rt2mod.RAY_DTYPE)
    out = np.full(6 * 16, 0xAA, np.uint8).view(rt2mod.SHADED_DTYPE)
    pr, po = rays.ctypes.data, out.ctypes.data
    assert pr % 16 == 0 and po % 16 == 0
    keep, fake = _fake_scene()
    good = rt2mod.shade_opts((1.0, 2.0, 3.0), True, 8)

    def opts(**kw):
        o = rt2mod.shade_opts((1.0, 2.0, 3.0), True, 8)
        for k, v in kw.items():
            if k.startswith("pad"):
                o.pad[int(k[3])] = v
            else:
                setattr(o, k, v)
        return o

    g = C.byref(good)
    bad_opts = [opts(pad0=1), opts(pad1=-1), opts(pad2=7), opts(max_bounce=0), opts(max_bounce=-3), opts(max_bounce=257)]
    bad_both = [(None, pr, 4, g, po, 0), (fake, pr, 4, None, po, 0), (fake, pr, -1, g, po, 0), (fake, None, 4, g, po, 0),
                (fake, pr, 4, g, None, 0), (fake, pr, 4, g, po, 2), (fake, pr, 4, g, po, -1)]
    bad_both += [(fake, pr, 4, C.byref(b), po, 0) for b in bad_opts]
    bad_dev = bad_both + [(fake, pr + 4, 4, g, po, 0), (fake, pr + 8, 4, g, po, 0), (fake, pr, 4, g, po + 8, 0),
                          (fake, pr, 4, g, po + 4, 0)]
    for s, r, n, op, o, fl in bad_dev:
        L.rt2_scene_create(None, 0, None, 0, None, 0, 0, None)  # leaves another message behind
        assert L.rt2_shade_rays(s, r, n, op, o, fl, None) < 0, (r, n, o, fl)
        assert b"rt2_shade_rays: bad argument" in L.rt2_last_error()
    for s, r, n, op, o, fl in bad_both:
        L.rt2_scene_create(None, 0, None, 0, None, 0, 0, None)
        assert L.rt2_shade_rays_host(s, r, n, op, o, fl) < 0, (r, n, o, fl)
        assert b"rt2_shade_rays_host: bad argument" in L.rt2_last_error()
    # a null scene or options, bad options: whatever n
    for op in (None, C.byref(bad_opts[0]), C.byref(bad_opts[3])):
        assert L.rt2_shade_rays(fake, None, 0, op, None, 0, None) < 0
        assert L.rt2_shade_rays_host(fake, None, 0, op, None, 0) < 0
    assert L.rt2_shade_rays(None, None, 0, g, None, 0, None) < 0
    # the largest and smallest bounce limits are arguments like any other
    for mb in (1, 256):
        assert L.rt2_shade_rays(fake, None, 0, C.byref(opts(max_bounce=mb)), None, 0, None) == 0
    # n = 0: nothing to do, nothing launched (no device here to launch on)
    assert L.rt2_shade_rays(fake, None, 0, g, None, 0, None) == 0
    assert L.rt2_shade_rays(fake, pr, 0, g, po, rt2mod.TRACE_SCALAR, None) == 0
    assert L.rt2_shade_rays_host(fake, None, 0, g, None, 0) == 0
    assert (out.view(np.uint8) == 0xAA).all()


def test_bvh_traversal_needs_nodes(rt2mod):
    """The only way into BVH traversal without nodes through the ABI,
    rt2_scene_set_traversal on a scene made without them, is refused; the
    query's own check ("BVH traversal needs the node array", before any device
    call) stands behind it."""
    L = rt2mod.lib()
    keep, fake = _fake_scene()
    assert L.rt2_scene_set_traversal(fake, 1) < 0
    assert b"BVH traversal needs the node array" in L.rt2_last_error()
    assert not any(keep.raw)


# ---- the one-pixel camera ---------------------------------------------------------------------------------------

def test_one_pixel_camera_is_trace_basic_for_one_ray(rt2mod, oraclemod):
    """Sky, diffuse and mirror-then-sky rays: 1, 1 and 2 segments; the diffuse
    colour is the hit triangle's material colour (oracle.closest_hits names the
    triangle) and the miss is oracle_sky of the normalised direction."""
    b = ss._Builder()
    dif = b.material(ss.DIFFUSE, color=(0.3, 1.0, 0.6))
    b.quad((-1, -1, -3), (2, 0, 0), (0, 2, 0), dif)                       # faces +z
    b.quad((3, -1, -2), (0, 2, 0), (0, 0, -2), b.mirror())               # faces -x
    sc0 = b.scene("premise", 2, 2, 8, 1, True)
    o = np.array([(0, 0, 0), (0, 0, 0), (0, 0, 0)], F32)
    f = np.array([(0.1, 0.2, -2.0), (0.0, 3.0, 0.5), (1.5, 0.1, -1.5)], F32)  # not of unit length
    sc = dict(name="premise", triangles=sc0["triangles"], materials=sc0["materials"], o=o, f=f, light=(0, 0, 0),
              textures=[])
    rgb, segs = H.oracle_shade(oraclemod, rt2mod, sc, 0, 8)
    d = (f.astype(np.float64) / np.linalg.norm(f.astype(np.float64), axis=1, keepdims=True)).astype(F32)
    _, tri, _, _ = oraclemod.closest_hits(sc["triangles"], o, d)
    assert tri[0] in (0, 1) and tri[1] == -1 and tri[2] in (2, 3)
    assert segs.tolist() == [1, 1, 2]
    assert np.array_equal(rgb[0], sc["materials"]["color"][sc["triangles"]["materialIndex"][tri[0]], :3])

    def sky(v):
        v = np.ascontiguousarray(v, F32)
        out = np.zeros(3, F32)
        oraclemod.lib().oracle_sky(v.ctypes.data, out.ctypes.data)
        return out

    assert np.allclose(rgb[1], sky(d[1]), rtol=0, atol=1e-6) and rgb[1].max() > 0
    # mirror then sky: (mirror colour 1 + sky(reflected)) / 2
    r = d[2] * np.array((-1, 1, 1), F32)
    assert np.allclose(rgb[2], (F32(1) + sky(r)) / F32(2), rtol=0, atol=1e-6)
    # the shadow ray adds a segment to the diffuse ray alone
    _, segs1 = H.oracle_shade(oraclemod, rt2mod, dict(sc, name="premise/shadow", light=(0.0, 5.0, 0.0)), 1, 8)
    assert segs1.tolist() == [2, 1, 2]


# ---- branch coverage, decided by the oracle ----------------------------------------------------------------------

def test_ray_sets_reach_every_branch(rt2mod, oraclemod):
    """Every entry of shade_scenes.BRANCHES is met by some ray of the oracle
    scenes at max_bounce = 8 with the shadow ray on (the limit inside a mirror
    pair also at 3), in the prefix of 1,025 rays the GPU tests compare.  The
    walk's segment counts are the oracle's for every ray: it followed the
    oracle's paths."""
    seen = {}
    for name, get in H.ORACLE_SCENES.items():
        sc = get()
        assert len(sc["o"]) == 1025
        for mb in (8, 3):
            events, segs = H.walk(oraclemod, sc, mb, 1)
            _, ref = H.oracle_shade(oraclemod, rt2mod, sc, 1, mb)
            same = segs == ref
            assert same.mean() > 0.99, (name, mb, float(same.mean()))  # binary32 numpy against the oracle's C
            for i in np.flatnonzero(same):
                for e in events[i]:
                    seen.setdefault(e, set()).add(name)
    for branch in H.BRANCHES:
        assert branch in seen, f"no ray reaches: {branch}"
    print({k: sorted(v) for k, v in seen.items()})


def test_soup_rays_hit_the_group_read_from_l2(rt2mod, oraclemod):
    sc = H.soup(1217)
    d = (sc["f"] / np.linalg.norm(sc["f"], axis=1, keepdims=True)).astype(F32)
    _, tri, _, _ = oraclemod.closest_hits(sc["triangles"], sc["o"], d)
    assert (tri[:63] >= 1216).sum() >= 4 and (tri >= 1216).sum() >= 8
    assert len(H.soup(1216)["triangles"]) == 38 * 32  # every group resident


def test_corridor_lanes_end_at_bounces_1_to_6(rt2mod, oraclemod):
    """In the first wave of the corridor's rays, patch ends at every bounce
    from 1 to 6 with max_bounce = 8."""
    ends, occ, early, seg0 = H.corridor_classes(oraclemod, rt2mod)
    assert set(range(1, 7)) <= set(ends[:64].tolist())
    assert set(range(1, 7)) <= set(ends[:1025].tolist())


def test_shadow_and_compaction_chunks(rt2mod, oraclemod):
    ends, occ, early, seg0 = H.corridor_classes(oraclemod, rt2mod)
    first, second, third = H.shadow_chunks(oraclemod, rt2mod)
    for k in (1, 2, 3):
        for v in (False, True):
            assert ((ends[first] == k) & (occ[first] == v)).sum() == 10
    assert 24 <= occ[first].sum() <= 36  # the light is hidden for about half of them
    assert (ends[second] > 0).sum() == 1 and ends[second][37] > 0
    assert (ends[third] == 0).all() and early[third].all()
    chunk = H.compaction_chunk(oraclemod, rt2mod)
    assert len(chunk) == 64 and (seg0[chunk[:40]] == 1).all() and (seg0[chunk[40:]] >= 3).all()


# ---- whole views ---------------------------------------------------------------------------------------------------

def preview_uniforms(rt2mod, sc):
    """surface_model's view with three bounces and the shadow ray on."""
    u = to_uniforms(rt2mod, sc["uniforms"])
    u.basicShading, u.basicShadingShadow, u.maxBounceCount = 1, 1, 3
    u.basicShadingLightPosition = rt2mod.Vec4(0.4, 3.0, 1.0, 1.0)
    return u


@pytest.mark.parametrize("w,h", M.VIEW_SIZES)
def test_views_take_several_paths(rt2mod, oraclemod, w, h):
    """The whole-view images hold pixels of one segment and of more (a second bounce or the shadow ray)."""
    sc = M.view_scene(w, h, M.VIEW_CAMERAS[1])
    u = preview_uniforms(rt2mod, sc)
    assert u.numTextures == len(M.view_textures())  # what a ray query takes
    oraclemod.set_textures(M.view_textures())
    try:
        xs, ys = np.meshgrid(np.arange(w), np.arange(h))
        seg = [oraclemod.render_pixels(sc["triangles"], sc["materials"], u, [x], [y], threads=1)[2]
               for x, y in zip(xs.ravel(), ys.ravel())]
    finally:
        oraclemod.set_textures([])
    assert {1, 2} <= set(seg) and seg.count(1) >= 16 and seg.count(2) >= 16
