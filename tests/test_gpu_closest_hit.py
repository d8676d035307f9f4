"""The closest-hit sweeps on scenes that say which triangle won.

Every image is compared with the CPU oracle as uint32 views (no tolerance), and
the segment counts are compared too.  The scenes are those of
tests/closest_hit_scenes.py; tests/test_closest_hit_scenes.py asserts on the
oracle alone what they are built to give (every 32-triangle group is the
closest hit of some pixels, exact ties occur and go to the lowest index, the
fans' winners lie at the end, the start or all over the scan), so a pass here
is not vacuous.  With index-coded lights a differing pixel is reported as the
triangle (and group) the GPU chose against the oracle's.

Every test asserts which kernel ran (rt2_scene_diag): the launcher falls back
to the automatic choice when a forced variant cannot hold the scene.

  a. decoded winners: soup, ties and the three fans at 1,216 / 1,217 / 8,192 /
     8,193 triangles (38 full groups; a 39th of one triangle; the L2
     continuation's 256-group limit; the smallest tile-stream scene, 257
     groups) on the automatic kernel, the forced resident kernels, 227, the
     scalar kernels 136, 86 and 92, and the BVH traversal (against the
     oracle's BVH mode).  (In the ties scenes of 1,217 and 8,193 triangles the
     last group's only triangle is a tie copy that must lose everywhere: they
     check that it does not win, the soup that the group is swept at all.);
  b. incoherent secondary rays: the soup with diffuse, mirror and light
     triangles, 2 rays, 6 bounces, 2 frames;
  c. tile-stream shapes: variant 380 forced on 1, 2 and 3 tiles with last
     tiles of 1, 9, 10 and 19 groups;
  d. the L2 continuation's whole-image build (355) on a 1920x1080 frame, four
     rows against the oracle.
"""
import ctypes as C

import numpy as np
import pytest

import closest_hit_scenes as S
from conftest import require_variant

pytestmark = pytest.mark.gpu

# kernel variants (rt2_render.hip kVariants): the resident matrix-filter kernel,
# its rank-slab build, their L2 continuations, the tile stream; 109 is the BVH
# traversal.  Forced by id in the tests: 227 (every wave reads the records from
# L2) and the scalar path's 136, 86 (LDS tiles) and 92 (assist).
RES, RES_SLAB, RES_L2, RES_L2_SLAB, TILES, BVH = 353, 354, 355, 356, 380, 109

# the automatic kernel of a small image (fewer than 6 items per resident lane:
# the rank-slab builds) and the resident kernel to force, by triangle count
AUTO = {1216: RES_SLAB, 1217: RES_L2_SLAB, 8192: RES_L2_SLAB, 8193: TILES}
FORCED_RES = {1216: RES, 1217: RES_L2, 8192: RES_L2}


def _bits(img):
    return np.ascontiguousarray(img[..., :3], dtype=np.float32).view(np.uint32)


def _same_bits(gpu, ref, what):
    bad = (_bits(gpu) != _bits(ref)).any(-1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} pixels differ in their bits"


def _winner(px, levels):
    try:
        i = int(S.decode(px[None], levels)[0])
    except ValueError:
        return f"no index code {px[:3]}"
    return "a miss" if i < 0 else f"triangle {i} (group {i // 32})"


def _same_winners(gpu, ref, what):
    """_same_bits for an index-coded image: names the winners at the first differing pixels."""
    bad = (_bits(gpu) != _bits(ref)).any(-1)
    if not bad.any():
        return
    levels = S.tone_levels()
    lines = [f"pixel x={x} y={y}: GPU {_winner(gpu[y, x], levels)}, oracle {_winner(ref[y, x], levels)}"
             for y, x in np.argwhere(bad)[:6]]
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} pixels differ in their bits\n" + "\n".join(lines))


_refs = {}
_bvh = {}


def _bvh_arrays(key, tris, mats):
    """The scene after build_bvh (which reorders the triangles, each keeping
    its material) with its nodes; built once per scene."""
    if key not in _bvh:
        sd = S.scene_data(tris, mats)
        _bvh[key] = (sd.triangles(), sd.materials(), sd.nodes())
    return _bvh[key]


def _ref(oraclemod, key, tris, mats, u, mode, fb=0, fc=1, rows=None):
    """One oracle image (the mean over the frames, as render_host returns it)
    and segment count per (scene, traversal, settings), shared by the tests
    and left unchanged."""
    rows = np.arange(u.height, dtype=np.int32) if rows is None else rows
    ck = (key, mode, bytes(u), fb, fc, rows.tobytes())
    if ck not in _refs:
        nodes = None
        if mode == "bvh":
            tris, mats, nodes = _bvh_arrays(key, tris, mats)
        acc, _, segs, _ = oraclemod.render(tris, mats, u, rows, fb, fc, mode, nodes=nodes)
        img = acc[..., :3] / np.float32(fc)
        img.setflags(write=False)
        _refs[ck] = (img, segs)
    return _refs[ck]


def _render(rt2mod, key, tris, mats, u, variant, fb=0, fc=1):
    """Renders on the forced variant (0: automatic; BVH: the BVH traversal);
    returns the image, the segment count and the id of the kernel that ran."""
    if variant == BVH:
        tris, mats, nodes = _bvh_arrays(key, tris, mats)
        scene = rt2mod.Scene(triangles=tris, materials=mats, nodes=nodes)
        scene.set_traversal("bvh")
    else:
        scene = rt2mod.Scene(triangles=tris, materials=mats)
        if variant:
            scene.set_variant(variant)
    img = scene.render_host(u, fb, fc)
    segs = scene.stats(reset=True).segments
    c = (C.c_ulonglong * 8)()
    lv = C.c_int(-1)
    assert rt2mod.lib().rt2_scene_diag(scene._p, c, C.byref(lv)) == 0
    scene.close()
    return img, segs, lv.value


def _ran(rt2mod, got, want):
    name = rt2mod.lib().rt2_variant_name
    assert got == want and name(got) == name(want), \
        f"kernel {got} ({name(got).decode() if name(got) else None}) ran, not {want} ({name(want).decode()})"


# ---- a. decoded winners ------------------------------------------------------

def _kernel(how, n):
    """(variant to force, kernel that must run) of a test id: the automatic
    choice, the forced resident kernel of that size, "v<id>", the BVH traversal."""
    if how == "auto":
        return 0, AUTO[n]
    v = FORCED_RES[n] if how == "res" else BVH if how == "bvh" else int(how[1:])
    return v, v


def _hows(n):
    return ["auto"] + (["res"] if n in FORCED_RES else []) + ["v227", "v136", "v86", "v92", "bvh"]


@pytest.mark.parametrize("kind,n,how", [(k, n, how) for n in S.SIZES for k in S.KINDS for how in _hows(n)])
def test_decoded_winners(rt2mod, oraclemod, kind, n, how):
    force, want = _kernel(how, n)
    require_variant(rt2mod, want)
    tris, mats = S.coded_scene(kind, n)
    w, h = S.SIZES[n]
    u = S.coded_uniforms(w, h, n)
    ref, segs = _ref(oraclemod, (kind, n), tris, mats, u, "bvh" if how == "bvh" else "brute")
    img, gsegs, ran = _render(rt2mod, (kind, n), tris, mats, u, force)
    _ran(rt2mod, ran, want)
    _same_winners(img, ref, f"{kind}, {n} triangles, {how}")
    assert gsegs == segs == w * h


# ---- b. incoherent rays ------------------------------------------------------

@pytest.mark.parametrize("how", ["auto", "v136", "bvh"])
@pytest.mark.parametrize("n", [1217, 8192, 8193])
def test_incoherent_rays(rt2mod, oraclemod, n, how):
    force, want = _kernel(how, n)
    require_variant(rt2mod, want)
    tris, mats = S.mixed_scene(n)
    u = rt2mod.offline_uniforms(64, 36, 6, 2, n)
    ref, segs = _ref(oraclemod, ("mixed", n), tris, mats, u, "bvh" if how == "bvh" else "brute", 3, 2)
    img, gsegs, ran = _render(rt2mod, ("mixed", n), tris, mats, u, force, 3, 2)
    _ran(rt2mod, ran, want)
    _same_bits(img, ref, f"mixed soup, {n} triangles, {how}")
    assert gsegs == segs


# ---- c. tile-stream shapes ---------------------------------------------------

@pytest.mark.parametrize("ng", S.TILE_SHAPE_GROUPS)
def test_tile_stream_shapes(rt2mod, oraclemod, ng):
    """Variant 380 (19-group tiles, two LDS buffers) on one tile of 1, 9, 10 and
    19 groups (the same tile alternates between the buffers from segment to
    segment), two tiles with a last tile of 1, 9 and 10 groups (9: the mid-tile
    issue at group 9 is never reached) and three tiles (the buffer parity of a
    tile alternates between segments); the last group is ragged (19 triangles)."""
    require_variant(rt2mod, TILES)
    n = 32 * ng - 13
    tris, mats = S.mixed_scene(n)
    u = rt2mod.offline_uniforms(64, 36, 6, 2, n)
    ref, segs = _ref(oraclemod, ("mixed-shape", n), tris, mats, u, "brute")
    img, gsegs, ran = _render(rt2mod, ("mixed-shape", n), tris, mats, u, TILES)
    _ran(rt2mod, ran, TILES)
    _same_bits(img, ref, f"tile stream, {ng} groups")
    assert gsegs == segs


# ---- d. the L2 continuation's whole-image build --------------------------------

def test_l2_continuation_full_size_rows(rt2mod, oraclemod):
    """The mixed soup of 2,400 triangles (75 groups, 37 of them read from L2) at
    1920x1080, 1 ray, 4 bounces: a whole image takes the build without
    fair-share priority (355); rows 0, 539, 540 and 1079 against the oracle."""
    require_variant(rt2mod, RES_L2)
    n = S.ROW_RUN_TRIS
    tris, mats = S.mixed_scene(n)
    u = rt2mod.offline_uniforms(1920, 1080, 4, 1, n)
    rows = np.array([0, 539, 540, 1079], np.int32)
    ref, _ = _ref(oraclemod, ("mixed-rows", n), tris, mats, u, "brute", rows=rows)
    img, gsegs, ran = _render(rt2mod, ("mixed-rows", n), tris, mats, u, 0)
    _ran(rt2mod, ran, RES_L2)
    assert img.shape == (1080, 1920, 4)
    _same_bits(img[rows], ref, "mixed soup, 2,400 triangles, 1920x1080 rows")
    assert 1920 * 1080 < gsegs <= 4 * 1920 * 1080
