"""The resident kernel's changes around the matrix sweep, bit for bit:
MfmaSpec::pair_loop (two groups per trip of the products' loop, hot masks by
v_writelane; rt2_k5_resident.h sweep_kt_res) and MfmaSpec::cam_park (a pixel's
camera end point computed once per pixel-frame and parked in the lane's 16
bytes of the wave's own unused T1 piece; rt2_path.h advance<.., PARK>).

Every case renders on the shipped kernels that take both knobs (353, 354) and,
in the experiment build, on each arm (353's spec with one knob) and on the
parent's form of 353 and 354 (neither knob).  Every image is compared as
uint32 views with the CPU oracle's brute mode, and each arm's with its parent
form's.

  - config A's Cornell box: 2 groups, so every wave's parking slot (the T1
    piece of group `wave`, 0..15) lies beyond the scene's groups, and the
    products' loop is one pair; config B's scene: 38 groups, 19 pairs.  Scenes
    of 1, 3 and 37 groups (fans): no pair and a remainder, a pair and a
    remainder, 18 pairs and a remainder;
  - images of 40 x 6 and 130 x 5: partially filled waves, widths that are no
    multiple of 64; the 40 x 6 image (240 items on 1,024-lane workgroups) ends
    in the cooperative drain and the move of the live rays to the low lanes,
    which carries the parked end points along;
  - 5 and 64 rays per pixel (a parked value read once per ray); 2 frames from
    frame 5 on, as whole-pixel items (the end point parked again at each
    ST_NEW_FRAME of the same lane) and as (frame, pixel) items (frame_split);
    the two rank slabs of tile_rows = 1, nranks = 2 (the item's row is not
    its image row);
  - a box with diffuse, mirror, glossy, checker, glass and edge-highlight
    surfaces, 12 bounces: one wave's hits have three material kinds that draw
    a direction beside kinds that draw none;
  - a large diffuse plane under a light, 64 x 4 pixels, 64 rays, 8 bounces:
    tens of thousands of rnd_dir calls, so long rejection runs occur.
"""
import numpy as np
import pytest

import closest_hit_scenes as S
from conftest import EXPERIMENTS, require_variant
from test_gpu_closest_hit import _bits, _same_bits
from test_gpu_exact_window import _fan

gpu = pytest.mark.gpu

SHIPPED = (353, 354)
# the experiment build's arms and the parent's form each is compared with
# (rt2_render.hip kVariants): 353 / 406 / 407 against 405, 354 against 408
PARENT_FORM = {353: 405, 406: 405, 407: 405, 354: 408}
VARIANTS = list(SHIPPED) + ([405, 406, 407, 408] if EXPERIMENTS else [])
by_variant = pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: f"v{v}")

SIZES = [(40, 6), (130, 5)]
# name: rays per pixel, first frame, frames, frame_split, ranks
SETTINGS = {
    "r5": (5, 0, 1, False, 1),
    "r64": (64, 0, 1, False, 1),
    "f2": (5, 5, 2, False, 1),
    "f2split": (5, 5, 2, True, 1),
    "slabs": (5, 5, 2, True, 2),
}

_refs = {}
_imgs = {}


def _case(rt2mod, config_scene, cfg, w, h, setting):
    sd, spec = config_scene(cfg)
    R, fb, fc, split, nranks = SETTINGS[setting]
    u = rt2mod.offline_uniforms(w, h, spec.bounces, R, sd.num_triangles)
    shards = [rt2mod.shard(1, r, nranks) for r in range(nranks)]
    return sd, u, fb, fc, split, shards


def _oracle(oraclemod, rt2mod, key, tris, mats, u, fb, fc, shards):
    """The oracle's slabs (mean over the frames) and segment counts of a case, computed once and left unchanged."""
    if key not in _refs:
        out = []
        for sh in shards:
            acc, _, segs, _ = oraclemod.render(tris, mats, u, rt2mod.shard_row_ids(u.height, sh), fb, fc, "brute")
            img = acc[..., :3] / np.float32(fc)
            img.setflags(write=False)
            out.append((img, segs))
        _refs[key] = out
    return _refs[key]


def _gpu(rt2mod, key, variant, make_scene, u, fb, fc, split, shards):
    """The variant's slabs and segment counts of a case, rendered once (an arm is compared with its parent form's)."""
    if (key, variant) not in _imgs:
        require_variant(rt2mod, variant)
        scene = make_scene()
        scene.set_variant(variant)
        scene.set_frame_split(split)
        out = []
        for sh in shards:
            img = scene.render_host(u, fb, fc, sh)
            out.append((img, scene.stats(reset=True).segments))
            assert scene.last_kernel() == variant
        scene.close()
        _imgs[(key, variant)] = out
    return _imgs[(key, variant)]


def _compare(rt2mod, oraclemod, key, variant, make_scene, tris, mats, u, fb, fc, split, shards, what):
    got = _gpu(rt2mod, key, variant, make_scene, u, fb, fc, split, shards)
    ref = _oracle(oraclemod, rt2mod, key, tris, mats, u, fb, fc, shards)
    for r, ((img, segs), (rimg, rsegs)) in enumerate(zip(got, ref)):
        _same_bits(img, rimg, f"{what}, slab {r}, variant {variant} against the oracle")
        assert segs == rsegs
    if EXPERIMENTS and variant in PARENT_FORM:
        par = _gpu(rt2mod, key, PARENT_FORM[variant], make_scene, u, fb, fc, split, shards)
        for r, ((img, segs), (pimg, psegs)) in enumerate(zip(got, par)):
            assert np.array_equal(_bits(img), _bits(pimg)), \
                f"{what}, slab {r}: variant {variant} differs from its parent form {PARENT_FORM[variant]}"
            assert segs == psegs


def _holds(rt2mod, variant, n_tris):
    require_variant(rt2mod, variant)
    assert S.n_groups(n_tris) <= 38  # every variant here is a resident kernel without the L2 continuation


@gpu
@by_variant
@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("cfg", ["A", "B"])
def test_config_scenes(rt2mod, oraclemod, config_scene, cfg, w, h, setting, variant):
    sd, u, fb, fc, split, shards = _case(rt2mod, config_scene, cfg, w, h, setting)
    assert S.n_groups(sd.num_triangles) == {"A": 2, "B": 38}[cfg]
    _holds(rt2mod, variant, sd.num_triangles)
    _compare(rt2mod, oraclemod, (cfg, w, h, setting), variant, lambda: rt2mod.Scene(sd, 0), sd.triangles(),
             sd.materials(), u, fb, fc, split, shards, f"config {cfg}, {w}x{h}, {setting}")


@gpu
@by_variant
@pytest.mark.parametrize("ng", [1, 3, 37])
def test_odd_group_counts(rt2mod, oraclemod, ng, variant):
    """The pair loop's remainder: fans of 32 ng - 13 triangles whose winners lie all over the scan."""
    tris, mats = _fan(ng, "shuffled")
    _holds(rt2mod, variant, len(tris))
    u = S.coded_uniforms(40, 6, len(tris))
    _compare(rt2mod, oraclemod, ("fan", ng), variant, lambda: rt2mod.Scene(triangles=tris, materials=mats), tris, mats,
             u, 0, 1, False, [rt2mod.shard()], f"fan of {ng} groups")


_scenes = {}


def _materials_box(rt2mod):
    if "box" not in _scenes:
        M = rt2mod.Material
        sd = rt2mod.SceneData()
        red, green, white = (sd.add_material(M.diffuse(c)) for c in ((1, 0, 0), (0, 1, 0), (1, 1, 1)))
        light = sd.add_material(M.light((1, 1, 1), 15.0))
        glass = sd.add_material(M.glass((0.9, 0.95, 1.0), 1.5))
        mirror = sd.add_material(M.specular((1, 1, 1), (1, 1, 1), 1.0, 1.0))
        checker = sd.add_material(M.checker(8.0))
        metal = sd.add_material(M.specular((0.8, 0.6, 0.3), (1, 1, 1), 0.7, 0.4))
        edge = M.diffuse((0.5, 0.5, 0.9))
        edge.isEdgeHighlight = 1
        sd.add_material(edge)
        sd.create_diverse_cornell_box(10.0, red, green, white, light, glass, mirror, checker, metal)
        sd.add_cube((0.0, -2.0, 0.0), (1.0, 1.0, 1.0), (0.3, 0.2, 0.1), 8)
        _scenes["box"] = sd
    return _scenes["box"]


def _diffuse_plane(rt2mod):
    """A wide white floor, a ceiling with a light panel under it and a wall ahead of the camera, all two-sided: the
    paths bounce between diffuse surfaces until the bounce limit or the roulette ends them."""
    if "plane" not in _scenes:
        M = rt2mod.Material
        sd = rt2mod.SceneData()
        white = sd.add_material(M.diffuse((0.9, 0.9, 0.9)))
        light = sd.add_material(M.light((1, 1, 1), 4.0))

        def quad(a, b, c, d, mat):
            for t in ((a, b, c), (a, c, d), (a, c, b), (a, d, c)):
                sd.add_triangle(*t, mat)

        for y, h, mat in ((-2.0, 200.0, white), (12.0, 200.0, white), (11.5, 20.0, light)):
            quad((-h, y, -h), (h, y, -h), (h, y, h), (-h, y, h), mat)
        quad((-200.0, -2.0, -20.0), (200.0, -2.0, -20.0), (200.0, 12.0, -20.0), (-200.0, 12.0, -20.0), white)
        _scenes["plane"] = sd
    return _scenes["plane"]


@gpu
@by_variant
@pytest.mark.parametrize("w,h", SIZES)
def test_three_material_kinds_in_a_wave(rt2mod, oraclemod, w, h, variant):
    sd = _materials_box(rt2mod)
    _holds(rt2mod, variant, sd.num_triangles)
    u = rt2mod.offline_uniforms(w, h, 12, 5, sd.num_triangles)
    mats = sd.materials()
    assert {0, 1, 3} <= set(mats["materialType"].tolist())  # diffuse, specular, checker
    _compare(rt2mod, oraclemod, ("box", w, h), variant, lambda: rt2mod.Scene(sd, 0), sd.triangles(), mats, u, 0, 2,
             False, [rt2mod.shard()], f"materials box, {w}x{h}")


@gpu
@by_variant
def test_diffuse_plane_long_rejection_runs(rt2mod, oraclemod, variant):
    sd = _diffuse_plane(rt2mod)
    _holds(rt2mod, variant, sd.num_triangles)
    u = rt2mod.offline_uniforms(64, 4, 8, 64, sd.num_triangles)
    _compare(rt2mod, oraclemod, ("plane",), variant, lambda: rt2mod.Scene(sd, 0), sd.triangles(), sd.materials(), u, 0,
             1, False, [rt2mod.shard()], "diffuse plane")
    segs = _refs[("plane",)][0][1]
    assert segs > 4 * 64 * 4 * 64  # the paths bounce: all but a path's last segment end in a diffuse hit and its draw
