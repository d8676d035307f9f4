"""The premises of tests/test_gpu_closest_hit.py, on the CPU oracle alone: the
index-coded scenes of tests/closest_hit_scenes.py give what the GPU tests
rely on (every group is the closest hit somewhere, ties occur and go to the
lowest index, the fans' winners lie where the scan order puts them, the mixed
soup has secondary segments), so none of those tests can pass vacuously.

Also recorded here: what the oracle's own BVH traversal gives on these scenes
(the same winner as brute force, or another member of the same tie family).
"""
import numpy as np
import pytest

import closest_hit_scenes as S

CODED = [(kind, n) for n in S.SIZES for kind in S.KINDS]

_imgs = {}


def _winners(rt2mod, oraclemod, kind, n, mode="brute"):
    """Decoded oracle image of a coded scene (cached): per-pixel winner, the image and its segment count."""
    if (kind, n, mode) not in _imgs:
        tris, mats = S.coded_scene(kind, n)
        w, h = S.SIZES[n]
        u = S.coded_uniforms(w, h, n)
        nodes = None
        if mode == "bvh":
            sd = S.scene_data(tris, mats)
            tris, mats, nodes = sd.triangles(), sd.materials(), sd.nodes()
        acc, _, segs, _ = oraclemod.render(tris, mats, u, np.arange(h, dtype=np.int32), 0, 1, mode, nodes=nodes)
        _imgs[(kind, n, mode)] = (S.decode(acc), acc, segs)
    return _imgs[(kind, n, mode)]


def test_levels_are_distinct(oraclemod):
    t = S.tone_levels()
    assert t.dtype == np.float32 and len(t) == S.LEVELS
    assert np.diff(t).min() > 5e-3  # far more than an ulp: a wrong level is a wrong bit pattern
    assert S.MAX_CODES > max(S.SIZES)


def test_decode_rejects_other_values(oraclemod):
    t = S.tone_levels()
    img = S.encode(np.array([[0, 5, -1, 8192]]), t)
    assert S.decode(img, t).tolist() == [[0, 5, -1, 8192]]
    bad = img.copy()
    bad[0, 1, 2] = np.nextafter(bad[0, 1, 2], np.float32(1))
    with pytest.raises(ValueError):
        S.decode(bad, t)
    bad = img.copy()
    bad[0, 0, 1] = 0.0  # a zero channel beside levels is no miss
    with pytest.raises(ValueError):
        S.decode(bad, t)


@pytest.mark.parametrize("kind,n", CODED)
def test_decode_round_trip(rt2mod, oraclemod, kind, n):
    idx, acc, segs = _winners(rt2mod, oraclemod, kind, n)
    assert idx.max() < n and idx.min() >= -1
    assert np.array_equal(S.encode(idx).view(np.uint32), np.ascontiguousarray(acc[..., :3]).view(np.uint32))
    assert segs == idx.size  # one segment per pixel: trace ends at the first light, or misses


def _soup_premise(idx, n, w):
    g = idx[idx >= 0] // 32
    cnt = np.bincount(g, minlength=S.n_groups(n))
    assert cnt.min() >= 3, f"group {int(cnt.argmin())} is the closest hit of {int(cnt.min())} pixels"
    assert (idx == n - 1).any()
    if w == 128:
        assert (idx < 0).mean() < 0.05


@pytest.mark.parametrize("n", list(S.SIZES))
def test_soup_hits_every_group(rt2mod, oraclemod, n):
    idx, _, _ = _winners(rt2mod, oraclemod, "soup", n)
    _soup_premise(idx, n, S.SIZES[n][0])


def test_row_run_soup_hits_every_group(rt2mod, oraclemod):
    """The geometry of the full-size row run (the mixed soup of 2,400
    triangles): with index-coded lights in place of its materials every one of
    its 75 groups is a closest hit, and so are the groups read from L2 (38 and
    up) in the four image rows that test compares."""
    n = S.ROW_RUN_TRIS
    tris, mats = S.mixed_scene(n)[0], S.code_materials(n)
    u = S.coded_uniforms(96, 54, n)
    acc, _, _, _ = oraclemod.render(tris, mats, u, np.arange(54, dtype=np.int32), 0, 1, "brute")
    idx = S.decode(acc)
    cnt = np.bincount(idx[idx >= 0] // 32, minlength=S.n_groups(n))
    assert cnt.min() >= 3, f"group {int(cnt.argmin())} is the closest hit of {int(cnt.min())} pixels"
    u = S.coded_uniforms(1920, 1080, n)
    acc, _, _, _ = oraclemod.render(tris, mats, u, np.array([0, 539, 540, 1079], np.int32), 0, 1, "brute")
    idx = S.decode(acc)
    far = idx[idx >= 38 * 32]
    assert len(far) >= 1000 and len(np.unique(far // 32)) >= 30


@pytest.mark.parametrize("n", list(S.SIZES))
def test_ties_go_to_the_lowest_index(rt2mod, oraclemod, n):
    idx, _, _ = _winners(rt2mod, oraclemod, "ties", n)
    tris, _ = S.coded_scene("ties", n)
    for fam in S.tie_families(n):
        for i in fam[1:]:  # the copies are the source's vertices bit for bit
            assert all(np.array_equal(tris[k][i], tris[k][fam[0]]) for k in "abc")
        own = {i: int((idx == i).sum()) for i in sorted(fam)}
        low = min(fam)
        assert own[low] >= 3, f"family {fam}: {own}"
        assert all(v == 0 for i, v in own.items() if i != low), f"family {fam}: {own}"


@pytest.mark.parametrize("n", list(S.SIZES))
@pytest.mark.parametrize("order", ["far_first", "near_first", "shuffled"])
def test_fan_winners(rt2mod, oraclemod, order, n):
    idx, _, _ = _winners(rt2mod, oraclemod, "fan_" + order, n)
    assert (idx >= 0).all()
    win = np.unique(idx)
    assert len(win) >= 8
    if order == "far_first":
        assert win.min() >= n - n // 4
    elif order == "near_first":
        assert win.max() < n // 4
    else:
        assert len(np.unique(win // 32)) >= 8


@pytest.mark.parametrize("kind,n", CODED)
def test_oracle_bvh_on_decoded_scenes(rt2mod, oraclemod, kind, n):
    """The reference's own behaviour, recorded (not a kernel check): its BVH
    traversal visits the leaves in another order than the array scan, so among
    equal distances it may keep another member of a tie family."""
    brute, _, _ = _winners(rt2mod, oraclemod, kind, n)
    bvh, _, _ = _winners(rt2mod, oraclemod, kind, n, "bvh")
    fam_of = np.arange(n + 1)  # miss (-1) -> n
    if kind == "ties":
        for fam in S.tie_families(n):
            fam_of[fam] = min(fam)
    other = fam_of[bvh] != fam_of[brute]
    assert not other.any(), f"{int(other.sum())} pixels whose BVH winner is outside the brute-force winner's family"
    tied = np.isin(brute, [i for fam in S.tie_families(n) for i in fam]) if kind == "ties" else np.zeros_like(other)
    # (so every pixel outside the tie families has the same winner)  Overall
    # agreement: 99 %, except where the families themselves own more than 1 %
    # of the image (the 38- and 39-group scenes at 64x36: 4 champions of 45 cells)
    if tied.mean() <= 0.01:
        assert (bvh == brute).mean() >= 0.99
    else:
        assert n < 8192 and tied.mean() < 0.04


# every mixed soup the GPU tests render, with their settings: (triangles, width,
# height, rays, bounces, first frame, frames, rows or None for all)
ROWS = np.array([0, 539, 540, 1079], np.int32)
MIXED = ([(n, 64, 36, 2, 6, 3, 2, None) for n in (1217, 8192, 8193)] +
         [(32 * g - 13, 64, 36, 2, 6, 0, 1, None) for g in S.TILE_SHAPE_GROUPS] +
         [(S.ROW_RUN_TRIS, 1920, 1080, 1, 4, 0, 1, ROWS)])


@pytest.mark.parametrize("n,w,h,rays,bounces,fb,fc,rows", MIXED, ids=[f"{m[0]}-{m[1]}x{m[2]}" for m in MIXED])
def test_mixed_soup_has_two_segments_per_sample(rt2mod, oraclemod, n, w, h, rays, bounces, fb, fc, rows):
    """Below 8,192 triangles the mixed soups' triangles are larger (mixed_extent:
    the same total area at every count), so that also 19 triangles leave few
    primary rays without a hit and send scattered rays on to further hits."""
    tris, mats = S.mixed_scene(n)
    u = rt2mod.offline_uniforms(w, h, bounces, rays, n)
    rows = np.arange(h, dtype=np.int32) if rows is None else rows
    _, _, segs, _ = oraclemod.render(tris, mats, u, rows, fb, fc, "brute")
    assert segs / (len(rows) * w * rays * fc) >= 2.0
