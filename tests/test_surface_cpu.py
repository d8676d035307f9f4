"""Surface queries without a GPU: the C-ABI's record layout, symbols and
argument checks, and the premises of tests/test_gpu_surface.py on the CPU
oracle and the float64 model of tests/surface_model.py alone (every material
type and misses in every view, the texture-index rules and both LIGHT branches
reached, hits beyond the resident groups, bounds of the model below 1e-4 on
every scene they are used on), so none of those tests can pass vacuously."""
import ctypes as C

import numpy as np
import pytest

import shading_scenes as ss
import surface_model as M
import trace_rays_lib as T
from test_shading_model import to_uniforms

F32 = np.float32


def test_record_layout_and_symbols(rt2mod):
    s = rt2mod.SURFACE_DTYPE
    assert s.itemsize == 48  # sizeof(rt2_surface): three 16-byte stores
    want = {"dst": (0, "<f4"), "tri": (4, "<i4"), "mtl": (8, "<i4"), "mtl_type": (12, "<i4"), "normal": (16, "<f4"),
            "u": (28, "<f4"), "albedo": (32, "<f4"), "v": (44, "<f4")}
    assert set(s.names) == set(want)
    for name, (off, kind) in want.items():
        assert s.fields[name][1] == off and s.fields[name][0].base == np.dtype(kind), name
    assert s.fields["normal"][0].shape == (3,) and s.fields["albedo"][0].shape == (3,)
    L = rt2mod.lib()
    assert L.rt2_abi_version() == 4  # the entry points only add to the interface
    for name in ("rt2_surface_rays", "rt2_surface_rays_host", "rt2_camera_rays", "rt2_camera_rays_host"):
        assert hasattr(L, name) and name in rt2mod.EXPORTED
    codes = (rt2mod.SURFACE_RES, rt2mod.SURFACE_RES_L2, rt2mod.SURFACE_SCALAR, rt2mod.SURFACE_BVH,
             rt2mod.OCCLUDED_RES, rt2mod.OCCLUDED_RES_L2, rt2mod.OCCLUDED_SCALAR, rt2mod.OCCLUDED_BVH,
             rt2mod.QUERY_RES, rt2mod.QUERY_RES_L2, rt2mod.QUERY_SCALAR, rt2mod.QUERY_BVH)
    assert len(set(codes)) == 12 and all(c < -1 for c in codes)  # -1 is the preview, >= 0 a render's variant
    for f in ("surface", "surface_device", "camera_rays", "camera_rays_device", "feature_buffers"):
        assert callable(getattr(rt2mod.Scene, f))


def _fake_scene():
    """Zeroed memory in place of a scene: brute-force traversal, no nodes, nothing on a device."""
    buf = C.create_string_buffer(4096)
    return buf, C.c_void_p(C.addressof(buf))


def test_surface_argument_validation(rt2mod):
    """Bad arguments return < 0 with "bad argument" before any device call
    (there is no device here; `fake` is no scene)."""
    L = rt2mod.lib()
    rays = np.zeros(4, rt2mod.RAY_DTYPE)
    out = np.full(6, 0xAA, np.uint8).repeat(48).view(rt2mod.SURFACE_DTYPE)
    pr, po = rays.ctypes.data, out.ctypes.data
    assert pr % 16 == 0 and po % 16 == 0
    keep, fake = _fake_scene()
    bad_dev = [(None, pr, 4, po, 0), (fake, pr, -1, po, 0), (fake, None, 4, po, 0), (fake, pr, 4, None, 0),
               (fake, pr, 4, po, 2), (fake, pr, 4, po, -1), (fake, pr + 4, 4, po, 0), (fake, pr + 8, 4, po, 0),
               (fake, pr, 4, po + 8, 0), (fake, pr, 4, po + 4, 0)]
    for s, r, n, o, fl in bad_dev:
        L.rt2_scene_create(None, 0, None, 0, None, 0, 0, None)  # leaves another message behind
        assert L.rt2_surface_rays(s, r, n, o, fl, None) < 0, (r, n, o, fl)
        assert b"rt2_surface_rays: bad argument" in L.rt2_last_error()
    for s, r, n, o, fl in bad_dev[:6]:
        L.rt2_scene_create(None, 0, None, 0, None, 0, 0, None)
        assert L.rt2_surface_rays_host(s, r, n, o, fl) < 0, (r, n, o, fl)
        assert b"rt2_surface_rays_host: bad argument" in L.rt2_last_error()
    assert L.rt2_surface_rays(None, None, 0, None, 0, None) < 0  # a null scene, whatever n
    assert L.rt2_surface_rays_host(None, None, 0, None, 0) < 0
    # n = 0: nothing to do, nothing launched (no device here to launch on)
    assert L.rt2_surface_rays(fake, None, 0, None, 0, None) == 0
    assert L.rt2_surface_rays(fake, pr, 0, po, rt2mod.TRACE_SCALAR, None) == 0
    assert L.rt2_surface_rays_host(fake, None, 0, None, 0) == 0
    assert (out.view(np.uint8) == 0xAA).all()


def test_bvh_traversal_needs_nodes(rt2mod):
    """BVH traversal without nodes.  The only way into that state through the
    ABI, rt2_scene_set_traversal on a scene made without nodes, is refused, so
    the scene stays on the array scan; the queries' own check of it ("BVH
    traversal needs the node array", before any device call) is a second line
    behind this one."""
    L = rt2mod.lib()
    keep, fake = _fake_scene()
    assert L.rt2_scene_set_traversal(fake, 1) < 0
    assert b"BVH traversal needs the node array" in L.rt2_last_error()
    assert not any(keep.raw)  # nothing was recorded in the scene


def test_camera_rays_argument_validation(rt2mod):
    L = rt2mod.lib()
    keep, fake = _fake_scene()
    u = rt2mod.offline_uniforms(8, 6, 1, 1, 1)
    whole = rt2mod.shard()
    rays = np.full(8 * 6 * 32, 0xAA, np.uint8)
    pr = rays.ctypes.data
    assert pr % 16 == 0

    def zero(field):
        z = rt2mod.offline_uniforms(8, 6, 1, 1, 1)
        setattr(z, field, 0)
        return z

    pu = C.byref(u)
    bad = [(None, pu, whole, pr), (fake, None, whole, pr), (fake, C.byref(zero("width")), whole, pr),
           (fake, C.byref(zero("height")), whole, pr), (fake, pu, rt2mod.shard(2, 3, 3), pr),
           (fake, pu, rt2mod.shard(2, 4, 3), pr), (fake, pu, rt2mod.shard(0, 0, 1), pr),
           (fake, pu, rt2mod.shard(1, -1, 1), pr), (fake, pu, whole, None)]
    for s, up, sh, r in bad + [(fake, pu, whole, pr + 8)]:
        L.rt2_scene_create(None, 0, None, 0, None, 0, 0, None)  # leaves another message behind
        assert L.rt2_camera_rays(s, up, sh, r, None) < 0
        assert b"rt2_camera_rays: bad argument" in L.rt2_last_error()
    for s, up, sh, r in bad:
        L.rt2_scene_create(None, 0, None, 0, None, 0, 0, None)
        assert L.rt2_camera_rays_host(s, up, sh, r) < 0
        assert b"rt2_camera_rays_host: bad argument" in L.rt2_last_error()
    # a shard without rows (6 rows in tiles of 4: rank 2 of 3 owns none): nothing to do, nothing launched
    empty = rt2mod.shard(4, 2, 3)
    assert rt2mod.shard_rows(6, empty) == 0
    assert L.rt2_camera_rays(fake, pu, empty, None, None) == 0
    assert L.rt2_camera_rays_host(fake, pu, empty, None) == 0
    assert (rays == 0xAA).all()


# ---- premises -------------------------------------------------------------------------------------------------

VIEWS = [(w, h, cam, total) for (w, h) in M.VIEW_SIZES for cam in M.VIEW_CAMERAS for total in (0, 1217)]


def _view_hits(oraclemod, sc):
    o, d = M.view_rays(sc["uniforms"])
    _, tri, _, _ = oraclemod.closest_hits(sc["triangles"], o, d)
    mi = sc["triangles"]["materialIndex"][np.maximum(tri, 0)]
    return o, d, tri, mi


@pytest.mark.parametrize("w,h,cam,total", VIEWS)
def test_views_show_every_material_type(rt2mod, oraclemod, w, h, cam, total):
    """At least 16 hit pixels of each of the seven material types and of the
    unknown type 9, at least 16 miss pixels; texture indices in range, at or
    above numTextures (a unit without an image) and at or above 5; LIGHT with
    an emission below and above 1."""
    sc = M.view_scene(w, h, cam, total)
    assert len(sc["triangles"]) == max(total, 24)  # 12 quads
    mats = sc["materials"]
    o, d, tri, mi = _view_hits(oraclemod, sc)
    hit = tri >= 0
    assert (~hit).sum() >= 16
    types = mats["materialType"][mi]
    assert set(M.TYPES) == set(range(7)) | {9}
    for t in M.TYPES:
        assert (hit & (types == t)).sum() >= 16, f"type {t}: {int((hit & (types == t)).sum())} pixels"
    tex = hit & (types == ss.TEXTURE)
    seen = set(mats["textureIndex"][mi][tex].tolist())
    assert seen == set(M.VIEW_TEXTURE_INDICES)
    nt = M.VIEW_NUM_TEXTURES
    assert len(M.view_textures()) == nt == sc["uniforms"]["numTextures"]
    # With numTextures the number of images bound, "in range but unbound" and "at or above numTextures" are one
    # case: index 2 names a unit of the shader (< 5) that has no image.
    assert sum(0 <= i < nt for i in seen) == 2 and any(nt <= i < 5 for i in seen) and any(i >= 5 for i in seen)
    emax = mats["emissionColor"][mi][hit & (types == ss.LIGHT)][:, :3].max(1)
    assert (emax > 1).any() and (emax < 1).any()
    # the model's bounds on this view's rays
    _, _, tol = M.barycentrics(sc["triangles"], tri[hit], o[hit], d[hit])
    assert tol.max() < M.MAX_TOL
    assert M.unit_normals(sc["triangles"])[1][np.unique(tri[hit])].max() < M.MAX_TOL


@pytest.mark.parametrize("w,h", M.VIEW_SIZES)
def test_oracle_preview_gives_the_base_colour(rt2mod, oraclemod, w, h):
    """oracle.render with basicShading = 1, one bounce and no shadow returns,
    at pixels whose material is a pure function of the material, exactly
    surface_model.pure_albedo; CHECKER pixels are 0 or 1, both present; the
    sampled textures are neither black nor magenta, the other two indices
    black."""
    sc = M.view_scene(w, h, M.VIEW_CAMERAS[0])
    u = to_uniforms(rt2mod, sc["uniforms"])
    assert u.basicShading == 1 and u.maxBounceCount == 1 and u.basicShadingShadow == 0
    oraclemod.set_textures(M.view_textures())
    try:
        acc, _, _, _ = oraclemod.render(sc["triangles"], sc["materials"], u, np.arange(h, dtype=np.int32), 0, 1)
    finally:
        oraclemod.set_textures([])
    img = acc[..., :3].reshape(-1, 3)
    _, _, tri, mi = _view_hits(oraclemod, sc)
    mats = sc["materials"]
    types = np.where(tri >= 0, mats["materialType"][mi], -1)
    # pixels well inside a band: the oracle's own rays differ from the model's by roundings
    pure = np.isin(types, M.PURE_TYPES)
    want = M.pure_albedo(mats[np.isin(mats["materialType"], M.PURE_TYPES)])
    lut = np.zeros((len(mats), 3), F32)
    lut[np.isin(mats["materialType"], M.PURE_TYPES)] = want
    same = (img[pure].view(np.uint32) == lut[mi[pure]].view(np.uint32)).all(1)
    assert same.mean() > 0.9 and pure.sum() >= 6 * 16
    chk = img[types == ss.CHECKER]
    assert np.isin(chk, (0.0, 1.0)).all() and (chk == 0).any() and (chk == 1).any()
    ti = mats["textureIndex"][mi]
    for index in (0, 1):
        px = img[(types == ss.TEXTURE) & (ti == index)]
        assert (px.max(1) > 0).all() and not (px == (1.0, 0.0, 1.0)).all(1).any()
    for index in (2, 7):
        assert (img[(types == ss.TEXTURE) & (ti == index)] == 0).all()
    assert (img[types == -1].max(1) > 0).all()  # the oracle's misses show the sky: the record's zeros are not its


@pytest.mark.parametrize("kind,n", M.HIT_SCENES)
def test_hit_scenes(rt2mod, oraclemod, kind, n):
    """Hits and misses in every prefix the tests use; on 1,217 triangles some
    closest hits are in the group read from L2."""
    tris = T.scene_tris(kind, n)
    o, d = M.hit_scene_rays(kind, n)
    _, tri, _, _ = oraclemod.closest_hits(tris, o, d)
    assert tri[0] >= 0  # the 1-ray case is a hit
    for k in M.RAY_COUNTS[1:]:
        assert (tri[:k] >= 0).sum() >= 16 and (tri[:k] < 0).sum() >= 16, k
    assert tri[1024] >= 0  # the second workgroup's only ray
    if n == 1217:
        assert (tri[:63] >= 1216).sum() >= 4 and (tri >= 1216).sum() >= 8
    if kind == "far":
        assert np.abs(tris["a"]).max() == T.FAR
    else:  # the normal is compared with the model on these
        assert M.unit_normals(tris)[1].max() < M.MAX_TOL
    m = M.pure_materials(n)
    assert n < 12 or all((m["materialType"] == t).any() for t in M.PURE_TYPES)
    if n >= 12:
        e = m["emissionColor"][m["materialType"] == ss.LIGHT][:, :3].max(1)
        assert (e > 1).any() and (e < 1).any()


def test_fat_triangles_keep_the_bounds_small(rt2mod, oraclemod):
    tris = M.fat_triangles()
    o, d = M.fat_rays()
    _, tri, _, _ = oraclemod.closest_hits(tris, o, d)
    hit = tri >= 0
    assert hit.sum() >= 64 and (~hit).sum() >= 64 and len(np.unique(tri[hit])) >= 20
    u, v, tol = M.barycentrics(tris, tri[hit], o[hit], d[hit])
    assert tol.max() < M.MAX_TOL and M.unit_normals(tris)[1].max() < M.MAX_TOL
    # the model's barycentrics are those of the hit the oracle found: inside the triangle, and on its plane at dst
    assert (u > -tol).all() and (v > -tol).all() and (1 - u - v > -tol).all()
    assert (u > 0.2).any() and (v > 0.2).any() and (1 - u - v > 0.2).any()


def test_model_camera_directions():
    """Unit length, the centre column and row look along viewportFront, and a shard's rows are the interleave's."""
    un = M.view_scene(64, 4, M.VIEW_CAMERAS[0])["uniforms"]
    d = M.camera_dirs(un).reshape(4, 64, 3)
    assert np.allclose(np.sqrt((d * d).sum(-1)), 1.0, atol=1e-15)
    assert np.allclose(d[2, 32], (0.0, 0.0, -1.0), atol=1e-15)
    un = M.view_scene(67, 10, M.VIEW_CAMERAS[0])["uniforms"]
    assert M.slab_rows(un, (2, 1, 3)).tolist() == [2, 3, 8, 9]
    whole = M.camera_dirs(un).reshape(10, 67, 3)
    assert np.array_equal(M.camera_dirs(un, (2, 1, 3)).reshape(4, 67, 3), whole[[2, 3, 8, 9]])
