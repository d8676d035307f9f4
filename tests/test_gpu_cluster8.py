"""MfmaSpec::cluster_rows8 on the GPU (rt2_k5_resident.h cluster_rows_frag8,
rt2_mfma.h kt_group8; DESIGN.md "8-row products"): a compact cluster that at
most 8 rays of a wave need is swept with one 16-row fragment holding each ray
twice, three products per group for the triangles' two halves.

tests/test_gpu_cluster_private.py explains why whole images hide a wrong sweep
and how the comb scenes take that away (private triangles, one image row per
wave, lane = column).  The scene here (tests/cluster8_scenes.py) has its
evidence in both triangle halves of a group, in every cluster's last group
(the loop's odd remainder) and in the ragged last group's upper half, with
needing sets on both sides of the 8-ray threshold; the 16-row tests' comb scene
and the slot-order tests' tie scene are rendered as well.  The row model
(cluster8_scenes.row_model8, checked on the CPU in tests/test_cluster8_model.py)
says which rays an 8-row sweep holds, so the negative controls' outcomes are
predicted before the render.

The probe (rt2_mfma_probe layout 8) runs kt_group8's products on the
filter-probe draws."""
import ctypes as C
import json

import numpy as np
import pytest

import cluster16_scenes as c16
import cluster8_scenes as c8
import cluster_scenes as cs
import filter_probe_lib as fpl
import slot_order_scenes as sos
from closest_hit_scenes import mixed_materials
from conftest import require_variant

pytestmark = pytest.mark.gpu

RES, RES_SLAB, RES_R16, RES_SLAB_R16, RES_DIAG = 353, 354, 417, 418, 419
PRODUCT = (RES, RES_SLAB)
VARIANTS = (RES, RES_SLAB, RES_R16, RES_SLAB_R16, RES_DIAG)


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


def comb_reference(oraclemod, name, mode):
    """(scene dict, uniforms, materials, image, segments) of comb scene "8" / "16": "primary" = the deterministic
    one-segment render, "paths" = 4 bounces, 2 jittered rays per pixel, mixed materials and the sky."""
    sc = c8.comb8_scene() if name == "8" else c16.comb16_scene()
    tris = sc["triangles"]
    if mode == "primary":
        u, mats = cs.comb_uniforms(sc["H"], len(tris)), sc["materials"]
    else:
        u, mats = cs.comb_uniforms(sc["H"], len(tris), bounces=4, rays=2, env=1, jitter=True), mixed_materials(len(tris))
    ref, segs = reference(oraclemod, (name, mode), tris, mats, u)
    return sc, u, mats, ref, segs


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
    """ClusterDiag since the last stats reset: (wave, compact cluster) skipped, one block, two blocks, the needing
    rays summed, the cases of 1 to 16 needing rays and those of 1 to 8."""
    c = (C.c_ulonglong * 32)()
    rt2mod.lib().rt2_scene_diag_ex(scene._p, c, 32)
    return tuple(int(c[i]) for i in (25, 26, 27, 28, 29, 31))


def predicted_counts(rt2mod, t, o, d):
    bits = rt2mod.cluster_need(t, o, d)
    skipped = one = two = rays = r16 = r8 = 0
    for k in range(int(t["n"])):
        if not cs.compact_mask(t) >> k & 1:
            continue
        c = ((bits >> np.uint32(k)) & 1).reshape(-1, 64).sum(1)
        rays += int(c.sum())
        skipped += int((c == 0).sum())
        one += int(((c > 0) & (c <= 32)).sum())
        two += int((c > 32).sum())
        r16 += int(((c > 0) & (c <= 16)).sum())
        r8 += int(((c > 0) & (c <= 8)).sum())
    return skipped, one, two, rays, r16, r8


# ------------------------------------------------------------------ premises

def test_privacy_and_needing_sets(rt2mod, torch_cuda):
    """Every comb triangle passes the filter's U, -V, X terms for exactly its
    owner among the 64 rays of its row, in the 32-row products (layout 5) and
    in the 8-row ones (layout 8); the owner's ray hits it.  The needing sets
    of the rows, from rt2_cluster_need of the device's own rays, are the
    intervals': every required (c0, c1) is reached."""
    sc = c8.comb8_scene()
    tris = sc["triangles"]
    u = cs.comb_uniforms(sc["H"], len(tris))
    scene = rt2mod.Scene(triangles=tris, materials=sc["materials"], device=0)
    o, d = device_rays(scene, u)
    t = sc["table"]()
    reached = set()
    for bd in sc["bands"]:
        c0, c1, masks = cs.need_counts(t, o, d, bd["k"])
        assert masks[bd["row"]] == sum(1 << x for x in range(bd["x0"], bd["x1"]))
        reached.add((int(c0[bd["row"]]), int(c1[bd["row"]])))
    print("needing sets reached:", sorted(reached))
    assert reached == set(c8.REQUIRED8)
    r8 = np.zeros((len(o), 8), np.float32)
    r8[:, 0:3], r8[:, 3], r8[:, 4:7] = o, 1e38, d
    for layout in (5, 8):
        terms, _, rinfo, accept = scene.mfma_probe(layout, r8)
        assert np.all(rinfo[:, 0] == 1.0)
        passes = (np.ascontiguousarray(terms[:, :len(tris), :3]).view(np.int32) < 0).all(-1)  # [ray, triangle]
        private = 0
        for band, bd in enumerate(sc["bands"]):
            mine = np.flatnonzero(sc["band_of"] == band)
            row = slice(64 * bd["row"], 64 * bd["row"] + 64)
            want = np.arange(64)[:, None] == sc["column"][mine][None, :]
            got = passes[row][:, mine]
            assert np.array_equal(got, want), (f"layout {layout}, band {band}: {(got & ~want).sum()} pairs pass beside "
                                               f"the owners', {(want & ~got).sum()} owners do not pass")
            assert np.array_equal(accept[row][:, mine], want)
            private += len(mine)
        assert private == (sc["band_of"] >= 0).sum()
    print(f"{private} comb triangles, all private in both forms")


# -------------------------------------------------------------------- images

@pytest.mark.parametrize("mode", ["primary", "paths"])
@pytest.mark.parametrize("name", ["8", "16"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_comb_images(rt2mod, oraclemod, torch_cuda, variant, name, mode):
    """Bit-equal to the oracle, with its segment count, on 353 / 354, their forms before (417 / 418) and the
    diagnostic 419: the one-segment render, and 4 bounces of 2 jittered rays per pixel with mixed materials
    (refilled lanes, incoherent rays), on this file's comb scene and on the 16-row tests' (evidence in in-group slots
    0, 31, 15, 16, 8, 23, 7, 24, 12).  419's six counters on the one-segment render are the sums predicted from
    rt2_cluster_need."""
    require_variant(rt2mod, variant)
    sc, u, mats, ref, segs = comb_reference(oraclemod, name, mode)
    scene = rt2mod.Scene(triangles=sc["triangles"], materials=mats, device=0)
    scene.set_cluster_table(sc["table"]())
    assert scene.cluster_table()["n"] == len(sc["ranges"])
    img, st = render(scene, u, variant)
    exact(img, ref, f"variant {variant}, comb{name}, {mode}")
    assert st.segments == segs
    if variant == RES_DIAG and mode == "primary":
        got = diag_counts(rt2mod, scene)
        want = predicted_counts(rt2mod, scene.slot_table(), *device_rays(scene, u))
        print(f"skipped, one, two, rays, rows16, rows8 = {got}")
        assert got == want
        if name == "8":  # the bands' own cases: 7 of 11 at or below 8 rays, 4 at 9
            own = [bd["x1"] - bd["x0"] for bd in sc["bands"]]
            assert sum(c <= 8 for c in own) == 7 and want[5] >= 7 and want[4] - want[5] >= 4


@pytest.mark.parametrize("variant", VARIANTS)
def test_ties_go_to_the_lower_index(rt2mod, oraclemod, torch_cuda, variant):
    """The slot-order tests' tie scene through rt2_scene_set_slot_order: the oracle's image."""
    require_variant(rt2mod, variant)
    sc = sos.tie_scene()
    tris, mats = sc["triangles"], sc["materials"]
    u = cs.comb_uniforms(sc["H"], len(tris))
    ref, segs = reference(oraclemod, "tie", tris, mats, u)
    scene = rt2mod.Scene(triangles=tris, materials=mats, device=0)
    scene.set_slot_order(sc["slot_tri"], sc["table"])
    img, st = render(scene, u, variant)
    for name, i, j, row, col in sc["pairs"]:
        assert np.array_equal(img[row, col, :3], ref[row, col]), f"'{name}': pixel ({row}, {col}) of pair ({i}, {j})"
    exact(img, ref, f"variant {variant}, tie scene")
    assert st.segments == segs


@pytest.mark.parametrize("variant", VARIANTS)
def test_config_B_small(rt2mod, oraclemod, config_scene, torch_cuda, variant):
    """Config B at 64 x 16, 4 rays, 8 bounces, under the order the upload chose."""
    require_variant(rt2mod, variant)
    sd, spec = config_scene("B")
    u = rt2mod.offline_uniforms(64, 16, 8, 4, sd.num_triangles)
    ref, segs = reference(oraclemod, "B", sd.triangles(), sd.materials(), u)
    scene = rt2mod.Scene(sd, 0)
    assert cs.compact_mask(scene.slot_table()) != 0
    img, st = render(scene, u, variant)
    exact(img, ref, f"variant {variant}, config B")
    assert st.segments == segs


# --------------------------------------------------------- negative controls

@pytest.mark.parametrize("control", range(len(c8.CONTROLS8)))
@pytest.mark.parametrize("variant", PRODUCT)
def test_negative_control8(rt2mod, oraclemod, torch_cuda, variant, control):
    """One box shrunk in x so that an owned column's ray no longer needs it.
    Where the row model says the 8-row sweep no longer holds that ray, the
    render differs from the oracle at exactly the victim's pixel, where the
    wall shows; where the victim rides as filler row 6 or 7, nowhere.  (A
    wrong table only skips work: nothing here can fault.)  Predictions:
    cluster8_scenes.CONTROLS8, tests/test_cluster8_model.py
    test_control_predictions."""
    band, shrink, victim, rides = c8.CONTROLS8[control]
    sc, u, mats, ref, segs = comb_reference(oraclemod, "8", "primary")
    bd = sc["bands"][band]
    scene = rt2mod.Scene(triangles=sc["triangles"], materials=mats, device=0)
    t = sc["table"]({band: shrink})
    assert np.all(t["c"][bd["k"]]["lo"] < t["c"][bd["k"]]["hi"])
    o, d = device_rays(scene, u)
    mask = cs.need_counts(t, o, d, bd["k"])[2][bd["row"]]
    assert mask == sum(1 << x for x in range(*shrink)) and not mask >> victim & 1
    assert bin(mask).count("1") <= 8
    assert (victim in c8.swept_lanes8(mask)) == rides
    scene.set_cluster_table(t)
    img, st = render(scene, u, variant)
    want = np.zeros(ref.shape[:2], bool)
    want[bd["row"], victim] = not rides
    diff = (img[..., :3] != ref).any(-1)
    print(f"control {control} (band {band}, {shrink}, victim {victim}): rides {rides}, "
          f"differing pixels {np.argwhere(diff).tolist()}")
    assert np.array_equal(diff, want), f"differing pixels {np.argwhere(diff).tolist()}, expected {np.argwhere(want).tolist()}"
    if not rides:
        assert sc["H"] > len(sc["bands"])  # the last image row is wall only
        assert np.array_equal(img[bd["row"], victim, :3], ref[sc["H"] - 1, 0])
        assert not np.array_equal(ref[bd["row"], victim], ref[sc["H"] - 1, 0])
    assert st.segments == segs


# ------------------------------------------------- the products on the probe

KINDS = ["unit", "far", "tiny", "mixed"]


def _tri_array(rt2mod, V):
    t = np.zeros(len(V), dtype=rt2mod.TRI_DTYPE)
    t["a"][:, :3], t["b"][:, :3], t["c"][:, :3] = V[:, 0], V[:, 1], V[:, 2]
    return t


@pytest.mark.parametrize("kind", KINDS)
def test_rows8_products_on_hardware(rt2mod, torch_cuda, kind):
    """kt_group8's products on the filter-probe draws of
    tests/test_gpu_cluster16.py's probe test (the same generator and seeds, 437
    triangles so that the last group has 11 padding columns).

    - Every term is bit-equal to the 16-row product's term (layout 7) for the
      same (ray, triangle), U, -V and X alike.
    - No pair the reference accepts is rejected.
    - A padding column's three terms are exactly -Tw'.
    - The accumulation error stays within the bound layout 7's test reports
      against: 31 x 2^-24 sum|p| of the term's 16 f16 products, the proof's
      bound."""
    rng = np.random.default_rng(300 + KINDS.index(kind))
    V, rays = fpl.scene_and_rays(kind, rng, n_tris=437)
    sd = rt2mod.SceneData()
    sd.add_material(rt2mod.Material.diffuse((0.8, 0.8, 0.8)))
    scene = rt2mod.Scene(triangles=_tri_array(rt2mod, V), materials=sd.materials())
    raw = scene.export(6, np.uint16)
    assert ((raw & 0x7c00) != 0x7c00).all(), "a record holds an infinity or a NaN"
    n_pad = 448
    Bkt = fpl.records_kt(raw, n_pad)
    terms7, frags, rinfo, accept = scene.mfma_probe(7, rays)
    terms, frags8, rinfo8, accept8 = scene.mfma_probe(8, rays)
    assert np.array_equal(frags, frags8) and np.array_equal(rinfo, rinfo8) and np.array_equal(accept, accept8)
    assert terms.shape[1] == n_pad
    live = rinfo[:, 0] == 1.0
    assert live.sum() >= len(rays) // 2 and accept[live].sum() > 0
    t8 = np.ascontiguousarray(terms[live][..., :3])
    t7 = np.ascontiguousarray(terms7[live][..., :3])
    assert np.isfinite(t8).all()
    assert np.array_equal(t8.view(np.uint32), t7.view(np.uint32)), "a term differs from the 16-row product's"
    assert not terms[live][..., 3:].any()
    A = frags.astype(np.float64)[live, 48:64]
    hw = t8.astype(np.float64)
    worst = 0.0
    for q in range(3):
        ex = A @ Bkt[:, q, :].T
        sabs = np.abs(A) @ np.abs(Bkt[:, q, :]).T
        ulp = 2.0 ** -24 * sabs
        worst = max(worst, float((np.abs(hw[..., q] - ex) / np.where(ulp > 0, ulp, 1.0)).max()))
    passes = (t8.view(np.int32) < 0).all(-1)
    viol = np.argwhere(accept[live] & ~passes[:, :len(V)])
    print(json.dumps({"kind": kind, "acc_err_max_in_2^-24_sum_abs": worst, "acc_err_bound_assumed": 31.0,
                      "accepted_pairs": int(accept[live].sum()), "violations": int(len(viol))}))
    assert len(viol) == 0, f"reference-accepted pairs rejected by the 8-row products: {viol[:10]}"
    assert worst <= 31.0
    tw = A[:, 14]
    pad = hw[:, len(V):, :]
    assert np.array_equal(pad, np.broadcast_to(-tw[:, None, None], pad.shape))
