"""MfmaSpec::slot_order on the GPU (rt2_k5_resident.h; DESIGN.md "Slot order"):
353 / 354 and the diagnostic 416 sweep the scene's slot image, in which the
triangles are regrouped by place, and give the index-order scan's image bit for
bit: distance ties go to the lower index whatever the slots' order, the hit's
slot is mapped back to its index, and the need test follows the slot table.

The comb scenes and their frame are tests/cluster_scenes.py's (W = 64, one
image row per wave, lane = column); the tie scene and the orders are
tests/slot_order_scenes.py's, checked on the CPU in tests/test_slot_order.py
(a scan with the strict rule alone loses every pair's pixel there)."""
import ctypes as C

import numpy as np
import pytest

import cluster_scenes as cs
import slot_order_scenes as sos
from closest_hit_scenes import mixed_materials
from conftest import require_variant

pytestmark = pytest.mark.gpu

RES, RES_SLAB, RES_DIAG = 353, 354, 416
VARIANTS = (RES, RES_SLAB, RES_DIAG)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch  # torch's HIP runtime first: librt2 then shares it
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.cuda.set_device(0)
    return torch


_ref = {}


def reference(oraclemod, key, tris, mats, u):
    """(the oracle's image, its segments), once per key."""
    if key not in _ref:
        acc, _, segs, _ = oraclemod.render(tris, mats, u, np.arange(u.height, dtype=np.int32), 0, 1, "brute")
        _ref[key] = (acc[..., :3], segs)
    return _ref[key]


def exact(img, ref, what):
    bad = (img[..., :3] != ref).any(-1)
    assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} pixels differ, first at {np.argwhere(bad)[0]}"


def render(scene, u, variant):
    scene.set_variant(variant)
    scene.stats(reset=True)
    img = scene.render_host(u, 0, 1)
    st = scene.stats(reset=True)
    assert scene.last_kernel() == variant
    return img, st


def device_rays(scene, u):
    rays = scene.camera_rays(u)
    return np.ascontiguousarray(rays["o"]), np.ascontiguousarray(rays["d"])


def diag_counts(rt2mod, scene):
    c = (C.c_ulonglong * 32)()
    rt2mod.lib().rt2_scene_diag_ex(scene._p, c, 32)
    return tuple(int(c[i]) for i in (25, 26, 27, 28, 29))


def predicted_counts(rt2mod, t, o, d):
    """ClusterDiag's five sums from rt2_cluster_need of table t (whole waves of 64 live rays, one per image row)."""
    bits = rt2mod.cluster_need(t, o, d)
    skipped = one = two = rays = r16 = 0
    for k in range(int(t["n"])):
        if not cs.compact_mask(t) >> k & 1:
            continue
        c = ((bits >> np.uint32(k)) & 1).reshape(-1, 64).sum(1)
        rays += int(c.sum())
        skipped += int((c == 0).sum())
        one += int(((c > 0) & (c <= 32)).sum())
        two += int((c > 32).sum())
        r16 += int(((c > 0) & (c <= 16)).sum())
    return skipped, one, two, rays, r16


def scene_of(name):
    """(triangles, materials, uniforms) of a named scene in its tests' frame."""
    import rt2
    if name == "strips":
        tris, mats, _ = cs.strips_scene()
        return tris, mats, rt2.offline_uniforms(64, 16, 6, 2, len(tris))
    sc = cs.named_comb_scene(name)
    return sc["triangles"], sc["materials"], cs.comb_uniforms(sc["H"], len(sc["triangles"]))


def order_of(rt2mod, tris, order):
    """(slot_tri, table over the slot groups) of a named order."""
    if order == "rule":
        return rt2mod.cluster_order(tris)
    st = sos.orders(len(tris))[order]
    return st, sos.chunk_table(tris, st)


# --------------------------------------------------------------------- ties

@pytest.mark.parametrize("variant", VARIANTS)
def test_ties_go_to_the_lower_index(rt2mod, oraclemod, torch_cuda, variant):
    """Duplicate pairs (i < j) with i in the later slot: in one group, in two groups of one cluster, in a compact
    and a full cluster, in two compact clusters, across a round of 32 hot triangles of the episode, and with the
    winner in the ragged last group.  The image is the oracle's; every pair's pixel shows index i's colour."""
    require_variant(rt2mod, variant)
    sc = sos.tie_scene()
    tris, mats = sc["triangles"], sc["materials"]
    u = cs.comb_uniforms(sc["H"], len(tris))
    ref, segs = reference(oraclemod, "tie", tris, mats, u)
    scene = rt2mod.Scene(triangles=tris, materials=mats, device=0)
    scene.set_slot_order(sc["slot_tri"], sc["table"])
    assert np.array_equal(scene.slot_tri(), sc["slot_tri"]) and scene.slot_table()["n"] == len(sc["ranges"])
    img, st = render(scene, u, variant)
    for name, i, j, row, col in sc["pairs"]:
        assert np.array_equal(img[row, col, :3], ref[row, col]), f"'{name}': pixel ({row}, {col}) of pair ({i}, {j})"
    exact(img, ref, f"variant {variant}, tie scene")
    assert st.segments == segs


def test_set_slot_order_rejects_bad_orders(rt2mod, torch_cuda):
    sc = sos.tie_scene()
    scene = rt2mod.Scene(triangles=sc["triangles"], materials=sc["materials"], device=0)
    for name in ("repeat", "range"):
        st = sc["slot_tri"].copy()
        st[3] = st[4] if name == "repeat" else len(st)
        with pytest.raises(rt2mod.RT2Error):
            scene.set_slot_order(st, sc["table"])
    bad = sc["table"].copy()
    bad["c"][1]["g0"] += 1
    with pytest.raises(rt2mod.RT2Error):
        scene.set_slot_order(sc["slot_tri"], bad)


# ------------------------------------------------------------------- orders

@pytest.mark.parametrize("order", ["identity", "reversed", "random", "rule"])
@pytest.mark.parametrize("name", ["one", "two", "strips", "full", "ragged"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_orders(rt2mod, oraclemod, torch_cuda, variant, name, order):
    """The comb scenes, the strips scene (6 bounces, 2 rays, its mixed materials and its two ties) and the 38-group
    scenes under the identity, the reversed, a random and the rule's own order: the oracle's image and segments.
    The diagnostic variant's counters on the one-segment renders are the sums rt2_cluster_need predicts from the
    slot table for the device's rays."""
    require_variant(rt2mod, variant)
    tris, mats, u = scene_of(name)
    ref, segs = reference(oraclemod, name, tris, mats, u)
    scene = rt2mod.Scene(triangles=tris, materials=mats, device=0)
    st, t = order_of(rt2mod, tris, order)
    if order == "rule":  # what the upload installed
        assert np.array_equal(scene.slot_tri(), st) and scene.slot_table().tobytes() == t.tobytes()
    else:
        scene.set_slot_order(st, t)
    img, stats = render(scene, u, variant)
    exact(img, ref, f"variant {variant}, {name}, {order} order")
    assert stats.segments == segs
    if variant == RES_DIAG and name != "strips" and t["n"] > 0:
        got = diag_counts(rt2mod, scene)
        want = predicted_counts(rt2mod, t, *device_rays(scene, u))
        print(f"{name}, {order}: skipped, one, two, rays, rows16 = {got}")
        assert got == want


@pytest.mark.parametrize("variant", VARIANTS)
def test_set_cluster_table_resets_the_order(rt2mod, oraclemod, torch_cuda, variant):
    """rt2_scene_set_clusters installs its index-order table with the identity order in the slot image too."""
    require_variant(rt2mod, variant)
    sc = cs.named_comb_scene("full")
    tris, mats, u = scene_of("full")
    ref, segs = reference(oraclemod, "full", tris, mats, u)
    scene = rt2mod.Scene(triangles=tris, materials=mats, device=0)
    st, t = order_of(rt2mod, tris, "random")
    scene.set_slot_order(st, t)
    scene.set_cluster_table(sc["table"]())
    assert np.array_equal(scene.slot_tri(), np.arange(len(tris)))
    assert scene.slot_table().tobytes() == scene.cluster_table().tobytes()
    img, stats = render(scene, u, variant)
    exact(img, ref, f"variant {variant}, full, reset")
    assert stats.segments == segs
    if variant == RES_DIAG:
        assert diag_counts(rt2mod, scene) == predicted_counts(rt2mod, sc["table"](), *device_rays(scene, u))


# -------------------------------------------------------------------- paths

@pytest.mark.parametrize("variant", VARIANTS)
def test_config_B_small(rt2mod, oraclemod, config_scene, torch_cuda, variant):
    """Config B at 64 x 16, 4 rays, 8 bounces, under the order the upload chose (regrouped)."""
    require_variant(rt2mod, variant)
    sd, spec = config_scene("B")
    u = rt2mod.offline_uniforms(64, 16, 8, 4, sd.num_triangles)
    ref, segs = reference(oraclemod, "B", sd.triangles(), sd.materials(), u)
    scene = rt2mod.Scene(sd, 0)
    st = scene.slot_tri()
    assert np.array_equal(np.sort(st), np.arange(sd.num_triangles)) and not np.array_equal(st, np.sort(st))
    cs.check_table(scene.slot_table(), np.ascontiguousarray(sd.triangles()[st]))
    img, stats = render(scene, u, variant)
    exact(img, ref, f"variant {variant}, config B")
    assert stats.segments == segs


@pytest.mark.parametrize("order", ["reversed", "random"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_comb_paths(rt2mod, oraclemod, torch_cuda, variant, order):
    """4 bounces of 2 jittered rays per pixel on the `one` comb scene with mixed materials and the sky."""
    require_variant(rt2mod, variant)
    sc = cs.named_comb_scene("one")
    tris = sc["triangles"]
    mats = mixed_materials(len(tris))
    u = cs.comb_uniforms(sc["H"], len(tris), bounces=4, rays=2, env=1, jitter=True)
    ref, segs = reference(oraclemod, "one paths", tris, mats, u)
    scene = rt2mod.Scene(triangles=tris, materials=mats, device=0)
    scene.set_slot_order(*order_of(rt2mod, tris, order))
    img, stats = render(scene, u, variant)
    exact(img, ref, f"variant {variant}, paths, {order} order")
    assert stats.segments == segs


# --------------------------------------------------------- negative control

@pytest.mark.parametrize("variant", (RES, RES_SLAB))
def test_negative_control(rt2mod, oraclemod, torch_cuda, variant):
    """The `one` comb scene in reversed order with its own boxes, band 0's shrunk in x until column 0's ray no
    longer needs it: 31 rays still do, the one-block sweep's filler row comes from lanes 32..63, so lane 0's ray
    misses its triangle and the wall shows at exactly that pixel.  (A wrong table only skips work.)"""
    require_variant(rt2mod, variant)
    name, band, shrink, victim = cs.COMB_CONTROLS[0]
    sc = cs.named_comb_scene(name)
    tris, mats, u = scene_of(name)
    bd = sc["bands"][band]
    ref, segs = reference(oraclemod, name, tris, mats, u)
    scene = rt2mod.Scene(triangles=tris, materials=mats, device=0)
    n = int(sc["table"]()["n"])
    st = sos.orders(len(tris))["reversed"]
    for shrunk in (False, True):
        t = sos.reversed_table(sc["table"]({band: shrink} if shrunk else None), len(tris))
        if not shrunk:
            cs.check_table(t, np.ascontiguousarray(tris[st]))
        k = n - 1 - bd["k"]
        mask = cs.need_counts(t, *device_rays(scene, u), k)[2][bd["row"]]
        scene.set_slot_order(st, t)
        img, stats = render(scene, u, variant)
        diff = (img[..., :3] != ref).any(-1)
        want = np.zeros(ref.shape[:2], bool)
        if shrunk:
            assert mask == sum(1 << x for x in range(*shrink)) and victim not in cs.swept_lanes(mask)
            want[bd["row"], victim] = True
        else:
            assert mask >> victim & 1
        assert np.array_equal(diff, want), f"differing pixels {np.argwhere(diff).tolist()}"
        assert stats.segments == segs
    assert np.array_equal(img[bd["row"], victim, :3], ref[sc["H"] - 1, 0])  # the wall
    assert not np.array_equal(ref[bd["row"], victim], ref[sc["H"] - 1, 0])
