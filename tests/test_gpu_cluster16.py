"""MfmaSpec::cluster_rows16 on the GPU (rt2_k5_resident.h cluster_rows_frag16,
rt2_mfma.h kt_group16; DESIGN.md "16-row products"): a compact cluster that at
most 16 rays of a wave need is swept with 16-row products, six per group for
the triangles' two halves.

tests/test_gpu_cluster_private.py explains why whole images hide a wrong sweep
and how the comb scenes take that away (private triangles, one image row per
wave, lane = column); all of it holds here, on a comb scene whose evidence
sits in both triangle halves of a group (tests/cluster16_scenes.py: in-group
indices 0, 15, 16, 31 and more), with needing sets on both sides of the 16-ray
threshold.  The row model (cluster16_scenes.row_model16, checked on the CPU in
tests/test_cluster16_model.py) says which rays a 16-row sweep holds, so the
negative controls' outcomes are predicted before the render.

The probe (rt2_mfma_probe layout 7) runs kt_group16's products on the
filter-probe draws: U, -V and X of every (ray, triangle) pair from
v_mfma_f32_16x16x32_f16 with the [rays | 0] and [0 | rays] fragments and the
records read through kt16_record_lane."""
import ctypes as C
import json

import numpy as np
import pytest

import cluster16_scenes as c16
import cluster_scenes as cs
import filter_probe_lib as fpl
from closest_hit_scenes import mixed_materials
from conftest import require_variant

pytestmark = pytest.mark.gpu

RES, RES_SLAB, RES_CR32, RES_SLAB_CR32, RES_DIAG = 353, 354, 412, 413, 411
PRODUCT = (RES, RES_SLAB)
VARIANTS = (RES, RES_SLAB, RES_CR32, RES_SLAB_CR32, RES_DIAG)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch  # torch's HIP runtime first: librt2 then shares it
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.cuda.set_device(0)
    return torch


_ref = {}


def reference(oraclemod, mode):
    """(uniforms, materials, the oracle's image, its segments), once per mode: "primary" = the deterministic
    one-segment render, "paths" = 4 bounces, 2 jittered rays per pixel, mixed materials and the sky."""
    if mode not in _ref:
        sc = c16.comb16_scene()
        tris = sc["triangles"]
        if mode == "primary":
            u, mats = cs.comb_uniforms(sc["H"], len(tris)), sc["materials"]
        else:
            u, mats = cs.comb_uniforms(sc["H"], len(tris), bounces=4, rays=2, env=1, jitter=True), mixed_materials(len(tris))
        acc, _, segs, _ = oraclemod.render(tris, mats, u, np.arange(sc["H"], dtype=np.int32), 0, 1, "brute")
        _ref[mode] = (u, mats, acc[..., :3], segs)
    return _ref[mode]


def exact(img, ref, what):
    bad = (img[..., :3] != ref).any(-1)
    assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} pixels differ, first at {np.argwhere(bad)[0]}"


def device_rays(scene, u):
    rays = scene.camera_rays(u)
    return np.ascontiguousarray(rays["o"]), np.ascontiguousarray(rays["d"])


def diag_counts(rt2mod, scene):
    """ClusterDiag since the last stats reset: (wave, compact cluster) skipped, one block, two blocks, the needing
    rays summed, and the cases of 1 to 16 needing rays."""
    c = (C.c_ulonglong * 32)()
    rt2mod.lib().rt2_scene_diag_ex(scene._p, c, 32)
    return tuple(int(c[i]) for i in (25, 26, 27, 28, 29))


def predicted_counts(rt2mod, t, o, d):
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


# ------------------------------------------------------------------ premises

def test_privacy_and_needing_sets(rt2mod, torch_cuda):
    """Every comb triangle passes the filter's U, -V, X terms for exactly its
    owner among the 64 rays of its row, in the 32-row products (layout 5, as
    tests/test_gpu_cluster_private.py) and in the 16-row ones (layout 7); the
    owner's ray hits it.  The needing sets of the rows, from rt2_cluster_need
    of the device's own rays, are the intervals': every required (c0, c1) is
    reached."""
    sc = c16.comb16_scene()
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
    assert set(c16.REQUIRED16) <= reached
    r8 = np.zeros((len(o), 8), np.float32)
    r8[:, 0:3], r8[:, 3], r8[:, 4:7] = o, 1e38, d
    for layout in (5, 7):
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
@pytest.mark.parametrize("variant", VARIANTS)
def test_comb16_images(rt2mod, oraclemod, torch_cuda, variant, mode):
    """Bit-equal to the oracle on 353 / 354, their forms before (412 / 413) and the diagnostic 411: the one-segment
    render, and 4 bounces of 2 jittered rays per pixel with mixed materials (refilled lanes, incoherent rays).  411's
    counters on the one-segment render are the sums predicted from rt2_cluster_need, the 16-row count among them."""
    require_variant(rt2mod, variant)
    sc = c16.comb16_scene()
    u, mats, ref, segs = reference(oraclemod, mode)
    scene = rt2mod.Scene(triangles=sc["triangles"], materials=mats, device=0)
    scene.set_cluster_table(sc["table"]())
    assert scene.cluster_table()["n"] == len(sc["ranges"])
    scene.set_variant(variant)
    scene.stats(reset=True)
    img = scene.render_host(u, 0, 1)
    st = scene.stats(reset=True)
    exact(img, ref, f"variant {variant}, {mode}")
    assert st.segments == segs
    if variant == RES_DIAG and mode == "primary":
        got = diag_counts(rt2mod, scene)
        want = predicted_counts(rt2mod, scene.cluster_table(), *device_rays(scene, u))
        print(f"skipped, one, two, rays, rows16 = {got}")
        assert got == want
        # per image row of a band: its own cluster by its interval, every other compact cluster skipped or not
        # by the boxes; the bands' own cases: 8 of 12 at or below 16 rays, 4 above
        own = [bd["x1"] - bd["x0"] for bd in sc["bands"]]
        assert sum(c <= 16 for c in own) == 8 and want[4] >= 8 and want[1] - want[4] >= 4


# --------------------------------------------------------- negative controls

@pytest.mark.parametrize("control", range(len(c16.CONTROLS16)))
@pytest.mark.parametrize("variant", PRODUCT)
def test_negative_control16(rt2mod, oraclemod, torch_cuda, variant, control):
    """One box shrunk in x so that an owned column's ray no longer needs it.
    Where the row model says the 16-row sweep no longer holds that ray, the
    render differs from the oracle at exactly the victim's pixel, where the
    wall shows; where the victim rides as a filler row, nowhere.  (A wrong
    table only skips work: nothing here can fault.)  Predictions:
    tests/test_cluster16_model.py test_control_predictions."""
    band, shrink, victim = c16.CONTROLS16[control]
    sc = c16.comb16_scene()
    bd = sc["bands"][band]
    u, mats, ref, segs = reference(oraclemod, "primary")
    scene = rt2mod.Scene(triangles=sc["triangles"], materials=mats, device=0)
    t = sc["table"]({band: shrink})
    assert np.all(t["c"][bd["k"]]["lo"] < t["c"][bd["k"]]["hi"])
    o, d = device_rays(scene, u)
    mask = cs.need_counts(t, o, d, bd["k"])[2][bd["row"]]
    assert mask == sum(1 << x for x in range(*shrink)) and not mask >> victim & 1
    assert bin(mask).count("1") <= 16
    rides = victim in c16.swept_lanes16(mask)
    assert rides == (control >= 3)  # what the controls were chosen for
    scene.set_cluster_table(t)
    scene.set_variant(variant)
    scene.stats(reset=True)
    img = scene.render_host(u, 0, 1)
    st = scene.stats(reset=True)
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
def test_rows16_products_on_hardware(rt2mod, torch_cuda, kind):
    """kt_group16's products on the filter-probe draws of
    tests/test_gpu_filter_probe.py's kthr test (the same generator and seeds,
    437 triangles so that the last group has 11 padding columns).

    - Every f16 of every record is finite, the padding columns' too: the
      zeroed K-half of a fragment multiplies them.
    - The terms are the exact sum of their 16 f16 products (the fragment layout
      6 reports, the kt records) within the proof's 31 x 2^-24 sum|p|, the only
      bound DESIGN.md's argument allows; the largest ratio seen is printed, not
      compared with any smaller number.
    - No pair the reference accepts is rejected.
    - Padding columns.  In the K-slot threshold form a padding column's U, -V,
      X records hold only -tau (prep_mfma_kt), so in every form without Y,
      kt_group<false> and this one alike, its three terms are exactly -Tw':
      negative, the column is hot, and it is exact_window_lanes' index bound
      that keeps a padding index from being tested (layout 6's Y term does
      not reject it on these draws either).  What
      the 16-row form adds is the zeroed K-half, so the assertion is that the
      terms are that one exact product: finite, no NaN from 0 x record, bit
      for bit what the 32-row products give.  The ragged last group of the
      comb scene above carries evidence and renders bit-equal."""
    rng = np.random.default_rng(300 + KINDS.index(kind))
    V, rays = fpl.scene_and_rays(kind, rng, n_tris=437)
    sd = rt2mod.SceneData()
    sd.add_material(rt2mod.Material.diffuse((0.8, 0.8, 0.8)))
    scene = rt2mod.Scene(triangles=_tri_array(rt2mod, V), materials=sd.materials())
    raw = scene.export(6, np.uint16)
    assert ((raw & 0x7c00) != 0x7c00).all(), "a record holds an infinity or a NaN"
    n_pad = 448
    Bkt = fpl.records_kt(raw, n_pad)
    terms6, frags, rinfo, accept = scene.mfma_probe(6, rays)
    terms, frags7, rinfo7, accept7 = scene.mfma_probe(7, rays)
    assert np.array_equal(frags, frags7) and np.array_equal(rinfo, rinfo7) and np.array_equal(accept, accept7)
    assert terms.shape[1] == n_pad
    live = rinfo[:, 0] == 1.0
    assert live.sum() >= len(rays) // 2 and accept[live].sum() > 0
    A = frags.astype(np.float64)[live, 48:64]
    hw = terms[live][..., :3].astype(np.float64)
    assert np.isfinite(hw).all()
    worst = 0.0
    for q in range(3):
        ex = A @ Bkt[:, q, :].T
        sabs = np.abs(A) @ np.abs(Bkt[:, q, :]).T
        ulp = 2.0 ** -24 * sabs
        worst = max(worst, float((np.abs(hw[..., q] - ex) / np.where(ulp > 0, ulp, 1.0)).max()))
    passes = (np.ascontiguousarray(terms[live][..., :3]).view(np.int32) < 0).all(-1)
    viol = np.argwhere(accept[live] & ~passes[:, :len(V)])
    same = float((terms[live][..., :3] == terms6[live][..., :3]).mean())
    print(json.dumps({"kind": kind, "acc_err_max_in_2^-24_sum_abs": worst, "acc_err_bound_assumed": 31.0,
                      "accepted_pairs": int(accept[live].sum()), "violations": int(len(viol)),
                      "terms_bit_equal_to_32_row_frac": same}))
    assert len(viol) == 0, f"reference-accepted pairs rejected by the 16-row products: {viol[:10]}"
    assert worst <= 31.0
    tw = A[:, 14]
    pad = terms[live][:, len(V):, :3].astype(np.float64)
    assert np.array_equal(pad, np.broadcast_to(-tw[:, None, None], pad.shape))
    assert np.array_equal(terms[live][:, len(V):, :3], terms6[live][:, len(V):, :3])
