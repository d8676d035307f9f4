"""MfmaSpec::cluster_rows on the GPU where a wrong need bit, or a wrong row of
cluster_rows_frag, cannot hide (rt2_k5_resident.h sweep_kt_res; DESIGN.md
"Compact clusters"; the scenes: tests/cluster_scenes.py "comb scenes").

tests/test_gpu_cluster_rows.py compares whole images of the strips scene.  Two
things let a wrong sweep leave such an image unchanged: a group's hot mask is
OR-ed over the fragment's rows and exact_window_lanes then gives all 64 rays
their own pass masks over the hot triangles, so a ray left out of a sweep still
finds its triangle when any swept ray passes the filter for it; and the
one-block fragment always holds 32 rays, so a ray left out can ride along as
filler.  The comb scenes take both away: every triangle used as evidence is
private (of its row's 64 rays only its owner's passes the matrix filter for it:
test_privacy, on the device's own filter terms), and the row model
(cluster_scenes.row_model, checked in tests/test_cluster_need.py) says which
rays a sweep holds, so the negative controls know exactly which pixels must go
wrong when a box leaves a ray out.

A wave's sweep holds the 64 pixels of one image row, lane l = column l.  From
advance() (rt2_path.h) and render_mfma_k5r: with W = 64, one ray per pixel and a
bounce limit of 1 every lane's path ends after its first segment, so all 64
lanes of a wave ask for an item in the same trip; a wave claims popcount(m) = 64
items with one atomicAdd per region, item lo + base + lanes_below(m); the 8
regions hold n_items / 8 = 8 H items each, a multiple of 64 when H is a multiple
of 8, so every base is a multiple of 64 and a claim is either one whole image
row (item / W = row, item % W = lane; one rank, so shard_row is the identity) or
past the region's end for all 64 lanes alike; cost order is off (p.order is
null), so items are not renumbered.  No wave ever has fewer than 64 live rays:
`upper` is true in every sweep and the cooperative tail never runs.

With the camera at the origin the render's primary rays are the bits of
rt2_camera_rays_host (Scene.camera_rays): advance() forms the end point as
((cam + front) + right px) + up py and the direction as normalize(end - o) with
o = (cam + 0 cs) + 0 sn = cam; with cam = 0 every one of these additions of
zero is exact, so the direction is normalize((front + right px) + up py), which
is camera_rays_kernel's expression, render_basic's.  (Only the sign of a zero
component can differ: +0 + -0 = +0.  Such a ray needs every cluster either
way.)  test_device_need_bits backs this with sky pixels."""
import ctypes as C

import numpy as np
import pytest

import cluster_scenes as cs
from closest_hit_scenes import mixed_materials
from conftest import require_variant

pytestmark = pytest.mark.gpu

RES, RES_SLAB, RES_NOCR, RES_SLAB_NOCR, RES_DIAG = 353, 354, 409, 410, 411
PRODUCT = (RES, RES_SLAB)
VARIANTS = (RES, RES_SLAB, RES_NOCR, RES_SLAB_NOCR, RES_DIAG)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch  # torch's HIP runtime first: librt2 then shares it
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.cuda.set_device(0)
    return torch


_ref = {}


def reference(oraclemod, name, mode):
    """(uniforms, materials, the oracle's image, its segments) of a comb scene, once per scene and mode:
    "primary" = the deterministic one-segment render, "paths" = 4 bounces, 2 jittered rays per pixel, mixed materials
    and the sky."""
    if (name, mode) not in _ref:
        sc = cs.named_comb_scene(name)
        tris = sc["triangles"]
        if mode == "primary":
            u, mats = cs.comb_uniforms(sc["H"], len(tris)), sc["materials"]
        else:
            u, mats = cs.comb_uniforms(sc["H"], len(tris), bounces=4, rays=2, env=1, jitter=True), mixed_materials(len(tris))
        acc, _, segs, _ = oraclemod.render(tris, mats, u, np.arange(sc["H"], dtype=np.int32), 0, 1, "brute")
        _ref[(name, mode)] = (u, mats, acc[..., :3], segs)
    return _ref[(name, mode)]


def exact(img, ref, what):
    bad = (img[..., :3] != ref).any(-1)
    assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} pixels differ, first at {np.argwhere(bad)[0]}"


def device_rays(scene, u):
    rays = scene.camera_rays(u)
    return np.ascontiguousarray(rays["o"]), np.ascontiguousarray(rays["d"])


def diag_counts(rt2mod, scene):
    """ClusterDiag of the renders since the last stats reset: (wave, compact cluster) skipped, one block, two blocks,
    and the needing rays summed."""
    c = (C.c_ulonglong * 32)()
    rt2mod.lib().rt2_scene_diag_ex(scene._p, c, 32)
    return tuple(int(c[i]) for i in (25, 26, 27, 28))


def predicted_counts(rt2mod, t, o, d):
    """The same four numbers from rt2_cluster_need of the rays, a wave per 64 rays (an image row), all of them live."""
    bits = rt2mod.cluster_need(t, o, d)
    skipped = one = two = rays = 0
    for k in range(int(t["n"])):
        if not cs.compact_mask(t) >> k & 1:
            continue
        c = ((bits >> np.uint32(k)) & 1).reshape(-1, 64).sum(1)
        rays += int(c.sum())
        skipped += int((c == 0).sum())
        one += int(((c > 0) & (c <= 32)).sum())
        two += int((c > 32).sum())
    return skipped, one, two, rays


# ------------------------------------------------------------------ premises

@pytest.mark.parametrize("name", ["one", "two", "full", "ragged"])
def test_privacy(rt2mod, torch_cuda, name):
    """Every comb triangle, evidence and the copies behind it: of the 64 rays of
    its row exactly its column's passes the filter's U, -V and X terms (the
    conditions of a sweep's only window, which has no distance bound; layout 5
    is the shipping kernels' form, a wave of the probe the 64 rays of a row,
    whose shared factors the terms carry).  And the device's rays need what
    the numpy model's rays need, so the CPU premises hold for them."""
    sc = cs.named_comb_scene(name)
    tris = sc["triangles"]
    u = cs.comb_uniforms(sc["H"], len(tris))
    scene = rt2mod.Scene(triangles=tris, materials=sc["materials"], device=0)
    o, d = device_rays(scene, u)
    mo, md = cs.camera_rays_model(u)
    print(f"{name}: {(d != md).any(1).sum()} of {len(d)} device rays differ from the numpy model's")
    t = sc["table"]()
    assert np.array_equal(rt2mod.cluster_need(t, o, d), rt2mod.cluster_need(t, mo, md))
    r8 = np.zeros((len(o), 8), np.float32)
    r8[:, 0:3], r8[:, 3], r8[:, 4:7] = o, 1e38, d
    terms, _, rinfo, accept = scene.mfma_probe(5, r8)
    assert np.all(rinfo[:, 0] == 1.0)
    passes = (np.ascontiguousarray(terms[:, :len(tris), :3]).view(np.int32) < 0).all(-1)  # [ray, triangle]
    private = 0
    for band, bd in enumerate(sc["bands"]):
        mine = np.flatnonzero(sc["band_of"] == band)
        row = slice(64 * bd["row"], 64 * bd["row"] + 64)
        want = np.arange(64)[:, None] == sc["column"][mine][None, :]
        got = passes[row][:, mine]
        assert np.array_equal(got, want), (f"band {band}: {(got & ~want).sum()} pairs pass beside the owners', "
                                           f"{(want & ~got).sum()} owners do not pass")
        assert np.array_equal(accept[row][:, mine], want)  # the reference test: the owner hits, nobody else
        private += len(mine)
    print(f"{name}: {private} comb triangles, all private (pitch {sc['pitch']})")
    assert private == (sc["band_of"] >= 0).sum()


# -------------------------------------------------------------------- images

def set_table(scene, sc, table):
    own = scene.cluster_table()
    if table == "explicit":
        scene.set_cluster_table(sc["table"]())
        assert scene.cluster_table()["n"] == len(sc["ranges"])
    elif table == "none":
        empty = own.copy()
        empty["n"] = 0
        scene.set_cluster_table(empty)
    else:
        cs.check_table(own, sc["triangles"])
        assert own["n"] >= 2 and cs.compact_mask(own) != 0


@pytest.mark.parametrize("table", ["explicit", "rule", "none"])
@pytest.mark.parametrize("name", ["one", "two"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_comb_images(rt2mod, oraclemod, torch_cuda, variant, name, table):
    require_variant(rt2mod, variant)
    sc = cs.named_comb_scene(name)
    u, mats, ref, segs = reference(oraclemod, name, "primary")
    scene = rt2mod.Scene(triangles=sc["triangles"], materials=mats, device=0)
    set_table(scene, sc, table)
    scene.set_variant(variant)
    scene.stats(reset=True)
    img = scene.render_host(u, 0, 1)
    st = scene.stats(reset=True)
    exact(img, ref, f"variant {variant}, comb scene {name}, table {table}")
    assert st.segments == segs == 64 * sc["H"]
    if variant == RES_DIAG:
        # the diagnostic build's cases are the rows' needing sets (a table with n = 0: the loop without clusters)
        got = diag_counts(rt2mod, scene)
        want = (0, 0, 0, 0) if table == "none" else predicted_counts(rt2mod, scene.cluster_table(), *device_rays(scene, u))
        print(f"{name}, table {table}: skipped, one, two, rays = {got}")
        assert got == want
        if table == "explicit":
            assert want[1:3] == {"one": (12, 0), "two": (3, 4)}[name]
            assert want[3] == sum(bd["x1"] - bd["x0"] for bd in sc["bands"])


@pytest.mark.parametrize("name", ["one", "two"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_comb_paths(rt2mod, oraclemod, torch_cuda, variant, name):
    """4 bounces, 2 jittered rays per pixel, mixed materials: refilled lanes and incoherent rays on the comb scenes."""
    require_variant(rt2mod, variant)
    sc = cs.named_comb_scene(name)
    u, mats, ref, segs = reference(oraclemod, name, "paths")
    scene = rt2mod.Scene(triangles=sc["triangles"], materials=mats, device=0)
    set_table(scene, sc, "explicit")
    scene.set_variant(variant)
    scene.stats(reset=True)
    img = scene.render_host(u, 0, 1)
    st = scene.stats(reset=True)
    exact(img, ref, f"variant {variant}, comb scene {name}, paths")
    assert st.segments == segs


# --------------------------------------------------------- negative controls

@pytest.mark.parametrize("control", range(len(cs.COMB_CONTROLS)))
@pytest.mark.parametrize("variant", PRODUCT)
def test_negative_control(rt2mod, oraclemod, torch_cuda, variant, control):
    """One box shrunk in x so that an owned column's ray no longer needs it.
    The row model says whether the sweep still holds that ray (more than 32
    needing rays: two blocks, every ray; at most 32: rows 0 .. c - 1 and
    fillers from block 1 only).  Where it does not, the render differs from
    the oracle at exactly the victim's pixel, where the wall shows; otherwise
    nowhere.  (A wrong table only skips work: nothing here can fault.)"""
    name, band, shrink, victim = cs.COMB_CONTROLS[control]
    sc = cs.named_comb_scene(name)
    bd = sc["bands"][band]
    u, mats, ref, segs = reference(oraclemod, name, "primary")
    scene = rt2mod.Scene(triangles=sc["triangles"], materials=mats, device=0)
    t = sc["table"]({band: shrink})
    assert np.all(t["c"][bd["k"]]["lo"] < t["c"][bd["k"]]["hi"])
    o, d = device_rays(scene, u)
    mask = cs.need_counts(t, o, d, bd["k"])[2][bd["row"]]
    assert mask == sum(1 << x for x in range(*shrink)) and not mask >> victim & 1
    rides = victim in cs.swept_lanes(mask)
    assert rides == (victim >= 32 or bin(mask).count("1") > 32)  # what the controls were chosen for
    scene.set_cluster_table(t)
    scene.set_variant(variant)
    scene.stats(reset=True)
    img = scene.render_host(u, 0, 1)
    st = scene.stats(reset=True)
    want = np.zeros(ref.shape[:2], bool)
    want[bd["row"], victim] = not rides
    diff = (img[..., :3] != ref).any(-1)
    print(f"control {control} ({name}, band {band}, {shrink}, victim {victim}): rides {rides}, "
          f"differing pixels {np.argwhere(diff).tolist()}")
    assert np.array_equal(diff, want), f"differing pixels {np.argwhere(diff).tolist()}, expected {np.argwhere(want).tolist()}"
    if not rides:
        assert sc["H"] > len(sc["bands"])  # the last image row is wall only
        assert np.array_equal(img[bd["row"], victim, :3], ref[sc["H"] - 1, 0])
        assert not np.array_equal(ref[bd["row"], victim], ref[sc["H"] - 1, 0])
    assert st.segments == segs


# ------------------------------------------------------------ the full table

@pytest.mark.parametrize("name", ["full", "ragged"])
@pytest.mark.parametrize("variant", PRODUCT + (RES_DIAG,))
def test_full_table(rt2mod, oraclemod, torch_cuda, variant, name):
    """38 groups in 13 clusters: the hot masks fill lanes 0..37 of maskv and the
    need masks lanes 38..63 (kNeedLane == kResGroups).  The diagnostic build's
    counters are those of the rays' need bits."""
    require_variant(rt2mod, variant)
    sc = cs.named_comb_scene(name)
    tris = sc["triangles"]
    assert (len(tris) + 31) // 32 == 38 and len(tris) == (1216 if name == "full" else 1184 + cs.FULL_RAGGED_LAST)
    t = sc["table"]()
    assert t["n"] == rt2mod.MAX_CLUSTERS == 13 and cs.compact_mask(t) == 0b1010101010101
    assert sum(r[1] - r[0] == 1 for r in sc["ranges"]) >= 3 and sc["ranges"][-1] == (34, 38, True)
    u, mats, ref, segs = reference(oraclemod, name, "primary")
    scene = rt2mod.Scene(triangles=tris, materials=mats, device=0)
    scene.set_cluster_table(t)
    scene.set_variant(variant)
    scene.stats(reset=True)
    img = scene.render_host(u, 0, 1)
    st = scene.stats(reset=True)
    exact(img, ref, f"variant {variant}, {name} table")
    assert st.segments == segs
    if variant == RES_DIAG:
        got, want = diag_counts(rt2mod, scene), predicted_counts(rt2mod, t, *device_rays(scene, u))
        print(f"{name}: skipped, one, two, rays = {got}")
        assert got == want


# ------------------------------------------- the device's need bits (411 only)

P = 2.0 ** -110  # a direction component below RT2_CLUSTER_DMIN
# the comb view rounded to multiples of 2^-8, so that a camera at (0.5, 0, 0) keeps every end-point addition exact
DYADIC = dict(front=(5 * 2.0 ** -8, 3 * 2.0 ** -8, -1.0), right=(0.625, 0.0, 0.0), up=(0.0, 0.078125, 0.0))
# name -> where the geometry goes (a shift, or a recipe worked out from the table), the view, and table edits
VIEWS = {
    "home": dict(),
    "inside a box": dict(place=("centre", 3)),
    "on a face plane": dict(place=("face", 3)),
    "at far_o": dict(far_o=0.0),
    "at far_o, camera moved": dict(cam=(0.5, 0.0, 0.0), far_o=0.5, **DYADIC),
    "beyond far_o": dict(cam=(0.5, 0.0, 0.0), far_o=0.25, **DYADIC),
    "zero components": dict(front=(0.0, 0.0, -1.0)),  # column 32 and row H / 2
    "negative zeros": dict(cam=(-0.0, -0.0, -0.0), front=(-0.0, -0.0, -1.0), right=(-cs.COMB_HX, -0.0, -0.0),
                           up=(-0.0, -8 * cs.COMB_ROW, -0.0)),
    "one tiny column": dict(front=(P, cs.COMB_FRONT[1], -1.0)),
    "all tiny": dict(front=(P, cs.COMB_FRONT[1], -1.0), right=(64 * P, 0.0, 0.0)),
    "grazing a corner": dict(place=("corner", 3)),
    "looking away": dict(front=(cs.COMB_FRONT[0], cs.COMB_FRONT[1], 1.0)),
}


def view_setup(rt2mod, name):
    """(triangles, table, uniforms) of a view of the `two` comb scene: the geometry translated, the camera at the
    origin (or, for far_o, at a point where every addition of advance()'s end point is exact: asserted)."""
    v = VIEWS[name]
    sc = cs.named_comb_scene("two")
    tris = sc["triangles"].copy()
    base = sc["table"]()
    cam = np.array(v.get("cam", (0.0, 0.0, 0.0)), np.float32)
    shift = cam.astype(np.float64).copy()
    if "place" in v:
        how, k = v["place"]
        lo, hi = base["c"][k]["lo"].astype(np.float64), base["c"][k]["hi"].astype(np.float64)
        if how == "centre":
            shift = -(lo + hi) / 2
        elif how == "face":  # the origin a little outside the box in x: its lo.x becomes exactly 0 below
            shift = -(lo + hi) / 2
            shift[0] = -lo[0]
        else:  # the ray of pixel (10, 2) runs from the origin through the box's corner (lo.x, lo.y, hi.z)
            shift = np.zeros(3)
    for key in ("a", "b", "c"):
        tris[key][:, :3] = (tris[key][:, :3].astype(np.float64) + shift).astype(np.float32)
    t = cs.explicit_table(tris, sc["ranges"], pad=cs.COMB_PAD, far_o=v.get("far_o"))
    u = cs.comb_uniforms(sc["H"], len(tris), env=1, front=v.get("front", cs.COMB_FRONT), right=v.get("right"),
                         up=v.get("up"))
    u.cameraPos.x, u.cameraPos.y, u.cameraPos.z = (float(c) for c in cam)
    if v.get("place", ("", 0))[0] == "face":
        k = v["place"][1]
        assert 0.0 < t["c"][k]["lo"][0] + cs.COMB_PAD  # the vertices stay inside
        t["c"][k]["lo"][0] = 0.0
        assert t["c"][k]["lo"][0] < t["c"][k]["hi"][0]
    if v.get("place", ("", 0))[0] == "corner":
        k = v["place"][1]
        corner = np.array([t["c"][k]["lo"][0], t["c"][k]["lo"][1], t["c"][k]["hi"][2]], np.float64)
        px, py = (2 * 10 - 64) / 64, (2 * 2 - sc["H"]) / sc["H"]
        aim = corner / -corner[2]
        u.viewportFront.x = float(aim[0] - cs.COMB_HX * px)
        u.viewportFront.y = float(aim[1] - cs.COMB_ROW * sc["H"] * py)
    return tris, t, u


def end_points_exact(u):
    """Whether ((cam + front) + right px) + up py and its difference from cam are exact in float32 for every pixel."""
    f = np.float32
    W, H = int(u.width), int(u.height)
    v3 = lambda v: np.array([v.x, v.y, v.z], f)
    cam, right, up, front = v3(u.cameraPos), v3(u.viewportRight), v3(u.viewportUp), v3(u.viewportFront)
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    px = ((x.ravel() * 2 - W).astype(f) / f(W))[:, None]
    py = ((y.ravel() * 2 - H).astype(f) / f(H))[:, None]
    e32 = (((cam + front)[None, :] + right[None, :] * px) + up[None, :] * py) - cam[None, :]
    c, r, p, fr = (a.astype(np.float64) for a in (cam, right, up, front))
    e64 = fr[None, :] + r[None, :] * px.astype(np.float64) + p[None, :] * py.astype(np.float64)
    direct = (front[None, :] + right[None, :] * px) + up[None, :] * py  # camera_rays_kernel's
    return np.array_equal(e32.astype(np.float64), e64) and np.array_equal(direct.astype(np.float64), e64)


@pytest.mark.parametrize("view", list(VIEWS))
def test_device_need_bits(rt2mod, oraclemod, torch_cuda, view):
    """The diagnostic kernel's counters against rt2_cluster_need of the same
    rays.  `rays`, the needing rays summed over sweeps and compact clusters, is
    exact and does not depend on how waves form; `skipped`, `one` and `two`
    follow from each image row's popcount, a row being a wave.  The camera
    stays within the filter's range in every view, so no wave goes to the
    drain (there sweep_kt_res returns before the need test and the wave would
    add nothing to any of the four).  A pixel whose ray hits nothing is
    tonemap(sky(d)) of the camera ray: the render's rays are those rays."""
    require_variant(rt2mod, RES_DIAG)
    tris, t, u = view_setup(rt2mod, view)
    sc = cs.named_comb_scene("two")
    if any(c != 0 for c in VIEWS[view].get("cam", ())):
        assert end_points_exact(u)
    scene = rt2mod.Scene(triangles=tris, materials=sc["materials"], device=0)
    scene.set_cluster_table(t)
    scene.set_variant(RES_DIAG)
    o, d = device_rays(scene, u)
    scene.stats(reset=True)
    img = scene.render_host(u, 0, 1)
    st = scene.stats(reset=True)
    got, want = diag_counts(rt2mod, scene), predicted_counts(rt2mod, t, o, d)
    bits = rt2mod.cluster_need(t, o, d)
    always = (bits == (1 << int(t["n"])) - 1).sum()
    print(f"{view}: skipped, one, two, rays = {got}; rays that need every cluster: {always} of {len(o)}")
    assert got[3] == want[3], "the device's need bits are not the host's"
    assert got == want
    acc, _, segs, _ = oraclemod.render(tris, sc["materials"], u, np.arange(sc["H"], dtype=np.int32), 0, 1, "brute")
    exact(img, acc[..., :3], f"view {view}")
    assert st.segments == segs
    # sky pixels
    _, tri, _, _ = oraclemod.closest_hits(tris, o, d)
    miss = np.flatnonzero(tri < 0)
    L = oraclemod.lib()
    flat = img.reshape(-1, img.shape[-1])
    sky = np.zeros(3, np.float32)
    for i in miss:
        dd = np.ascontiguousarray(d[i])
        L.oracle_sky(dd.ctypes.data, sky.ctypes.data)
        px = np.array([L.oracle_tonemap_srgb(float(s)) for s in sky], np.float32)
        assert np.array_equal(flat[i, :3], px), (view, int(i))
    if view == "looking away":
        assert len(miss) == len(o) and want[:3] == (7 * sc["H"], 0, 0)
    if view in ("beyond far_o", "all tiny"):
        assert always == len(o) and want == (0, 0, 7 * sc["H"], 7 * 64 * sc["H"])
    if view in ("zero components", "negative zeros", "one tiny column"):
        assert always >= sc["H"]
    if view == "inside a box":
        assert want[2] >= sc["H"]  # every ray starts inside cluster 3's box
