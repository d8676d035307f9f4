"""MfmaSpec::cluster_rows on the GPU (rt2_k5_resident.h sweep_kt_res; DESIGN.md
"Compact clusters"): small images of hand-built scenes, bit for bit against
the CPU oracle, on the kernels that follow the cluster table (353, 354 and the
diagnostic 411) and, in the experiment build, their forms without it.

tests/cluster_scenes.py says what the strips scene puts in front of a wave:
compact clusters that 0, 1, about 32 (both sides of the threshold) and all 64
of a row's primary rays need, clusters of 1, 2 and 3 groups, a compact cluster
first, last and beside a full one, a flat box, a ragged last group, and index
ties across the compact / full border.  The table is once the explicit one of
that file (rt2_scene_set_clusters) and once the upload rule's own.  After the
first bounce the rays are incoherent and the lanes refilled, so the general
case runs in every image too."""
import numpy as np
import pytest

import cluster_scenes as cs
from conftest import require_variant

pytestmark = pytest.mark.gpu

RES, RES_SLAB, RES_NOCR, RES_SLAB_NOCR, RES_DIAG = 353, 354, 409, 410, 411
VARIANTS = (RES, RES_SLAB, RES_DIAG, RES_NOCR, RES_SLAB_NOCR)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch  # torch's HIP runtime first: librt2 then shares it
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.cuda.set_device(0)
    return torch


# name -> (width, height, rays per pixel, bounce limit, camera z or None)
IMAGES = {
    "rows": (64, 36, 2, 6, None),     # every image row a wave: the threshold cases of the strips
    "few": (16, 2, 8, 6, None),       # 32 pixels: one wave with at most 32 live rays (the one-block waves: skip only)
    "far": (64, 4, 2, 4, 2.0 ** 21),  # origins outside the filter's range: the wave goes to the drain
}
_ref = {}


def reference(rt2mod, oraclemod, image):
    """The oracle's image of the strips scene, once per image."""
    if image not in _ref:
        tris, mats, _ = cs.strips_scene()
        w, h, rays, bounces, cam_z = IMAGES[image]
        u = rt2mod.offline_uniforms(w, h, bounces, rays, len(tris))
        if cam_z is not None:
            u.cameraPos.z = float(cam_z)
        acc, _, segs, _ = oraclemod.render(tris, mats, u, np.arange(h, dtype=np.int32), 0, 1, "brute")
        _ref[image] = (u, acc[..., :3], segs)
    return _ref[image]


def exact(img, ref, what):
    bad = (img[..., :3] != ref).any(-1)
    assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} pixels differ"


@pytest.mark.parametrize("table", ["explicit", "rule", "none"])
@pytest.mark.parametrize("image", list(IMAGES))
@pytest.mark.parametrize("variant", VARIANTS)
def test_strips_scene(rt2mod, oraclemod, torch_cuda, variant, image, table):
    require_variant(rt2mod, variant)
    tris, mats, ranges = cs.strips_scene()
    u, ref, segs = reference(rt2mod, oraclemod, image)
    scene = rt2mod.Scene(triangles=tris, materials=mats, device=0)
    own = scene.cluster_table()
    cs.check_table(own, tris)
    if table == "explicit":
        scene.set_cluster_table(cs.explicit_table(tris, ranges))
        got = scene.cluster_table()
        assert got["n"] == len(ranges) and cs.compact_mask(got) == 0b1111101
    elif table == "none":
        empty = own.copy()
        empty["n"] = 0
        scene.set_cluster_table(empty)  # the loop without clusters, inside the kernels that carry both
    else:
        assert own["n"] >= 2 and cs.compact_mask(own) != 0
    scene.set_variant(variant)
    img = scene.render_host(u, 0, 1)
    st = scene.stats(reset=True)
    exact(img, ref, f"variant {variant}, {image}, table {table}")
    assert st.segments == segs


def test_cases_are_met(rt2mod, oraclemod, torch_cuda):
    """The diagnostic build's counts on the `rows` image with the explicit
    table: every one of the three cases occurs (a cluster skipped, swept in the
    one-block form, swept in the two-block form), so the images above are
    images of them."""
    require_variant(rt2mod, RES_DIAG)
    import ctypes as C
    tris, mats, ranges = cs.strips_scene()
    u, ref, _ = reference(rt2mod, oraclemod, "rows")
    scene = rt2mod.Scene(triangles=tris, materials=mats, device=0)
    scene.set_cluster_table(cs.explicit_table(tris, ranges))
    scene.set_variant(RES_DIAG)
    scene.stats(reset=True)
    img = scene.render_host(u, 0, 1)
    scene.stats(reset=True)
    c = (C.c_ulonglong * 32)()
    rt2mod.lib().rt2_scene_diag_ex(scene._p, c, 32)
    skipped, one, two, rays = (int(c[i]) for i in (25, 26, 27, 28))
    print(f"(wave, compact cluster): skipped {skipped}, one block {one}, two blocks {two}, needing rays {rays}")
    exact(img, ref, "diagnostic build")
    assert skipped > 0 and one > 0 and two > 0 and rays > 32 * two


def test_set_clusters_rejects_bad_ranges(rt2mod, torch_cuda):
    tris, mats, ranges = cs.strips_scene()
    scene = rt2mod.Scene(triangles=tris, materials=mats, device=0)
    good = cs.explicit_table(tris, ranges)
    for breakage in ("gap", "short", "long", "count"):
        t = good.copy()
        if breakage == "gap":
            t["c"][2]["g0"] += 1
        elif breakage == "short":
            t["c"][t["n"] - 1]["g1_flags"] -= 1
        elif breakage == "long":
            t["c"][t["n"] - 1]["g1_flags"] += 1
        else:
            t["n"] = rt2mod.MAX_CLUSTERS + 1
        with pytest.raises(rt2mod.RT2Error):
            scene.set_cluster_table(t)
    scene.set_cluster_table(good)


@pytest.mark.parametrize("variant", (RES, RES_SLAB))
def test_config_B_small(rt2mod, oraclemod, config_scene, torch_cuda, variant):
    sd, spec = config_scene("B")
    u = rt2mod.offline_uniforms(64, 16, spec.bounces, 4, sd.num_triangles)
    scene = rt2mod.Scene(sd, 0)
    t = scene.cluster_table()
    cs.check_table(t, sd.triangles())
    assert t["n"] >= 3
    scene.set_variant(variant)
    img = scene.render_host(u, 0, 1)
    acc, _, segs, _ = oraclemod.render(sd.triangles(), sd.materials(), u, np.arange(16, dtype=np.int32), 0, 1, "brute")
    exact(img, acc[..., :3], f"config B, variant {variant}")
    assert scene.stats(reset=True).segments == segs
