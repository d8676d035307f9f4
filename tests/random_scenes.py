"""Scenes whose pixels depend on the random numbers, for
tests/random_path_model.py: pixel jitter, a defocus disk, diffuse scatter,
partial specular probability and survival below 1 (DESIGN.md "Random paths").

Built with the builders of shading_scenes.py and in its scene format.  The
images are 50 x 36: width and height differ, so y * width and y * height do, and
1800 pixels are no multiple of 64.  Rays per pixel are 1 or 3 (2 in the box, as
its issue set it); the frame ranges are (0, 1) and (5, 3): 5 * 968824447 is past
2^32, and a first frame other than 0 shows in the seed.
"""
import numpy as np

import shading_scenes as ss
from shading_scenes import CHECKER, DIFFUSE, GLASS, SPECULAR, TEXTURE

W, H = 50, 36
RIGHT, UP = (0.8, 0.0, 0.0), (0.0, 0.6, 0.0)
PIXEL = (2 * RIGHT[0] / W, 2 * UP[1] / H)     # one pixel in the viewport plane

# draw_is_one: jitter_sky, one ray, one frame.  At this first frame the ray of
# pixel (x, y) draws 1.0 (generator output >= 2^32 - 128) as its draw number
# DRAW_IS_ONE["draw"], a jitter draw.  Found by running the generator in numpy
# over frames 0, 1, 2, ... for all 1800 pixels; the first frame with such a draw
# is kept (4.6e7 generator steps).  tests/test_random_paths.py re-derives it.
DRAW_IS_ONE = dict(frame=8499, x=0, y=22, draw=2, bits=4294967240)


def _with(scene, **uniforms):
    scene["uniforms"].update({k: tuple(map(float, v)) for k, v in uniforms.items()})
    return scene


def _jitter(pixels):
    return dict(pixelRight=(pixels * PIXEL[0], 0, 0), pixelUp=(0, pixels * PIXEL[1], 0))


def jitter_sky(rays=1, frames=None, name=None):
    """Nothing is hit; the jitter spans 8 pixels, the defocus disk is zero: a
    pixel is a function of draws 2 and 3 of each ray, draw 1 is consumed."""
    frames = frames or ((0, 1) if rays == 1 else (5, 3))
    s = ss._sky_builder().scene(name or f"jitter_sky/r{rays}", W, H, 1, rays, True, frames=frames,
                                front=ss.HORIZON_FRONT)
    return _with(s, **_jitter(8))


def draw_is_one():
    return jitter_sky(1, (DRAW_IS_ONE["frame"], 1), "draw_is_one")


def defocus_sky():
    """No jitter; the origin moves on the arc 0.3 * (cos a, sin a), a in [0, 1]."""
    s = ss._sky_builder().scene("defocus_sky", W, H, 1, 3, True, frames=(0, 1), front=ss.HORIZON_FRONT)
    return _with(s, defocusDiskRight=(0.3, 0, 0), defocusDiskUp=(0, 0.3, 0))


def jitter_defocus_ramp():
    """Both on, before 12 light quads of three pixel rows each: a ray's row decides its strength."""
    b = ss._Builder()
    for k, strength in enumerate(ss.RAMP_STRENGTHS[2:14]):
        ss._pixel_rect(b, -3.0, W, H, -3, W + 4, 3 * k, 3 * k + 3, b.light((1.0, 0.5, 0.25), strength))
    s = b.scene("jitter_defocus_ramp", W, H, 4, 3, False, frames=(5, 3))
    return _with(s, defocusDiskRight=(0.05, 0, 0), defocusDiskUp=(0, 0.05, 0), **_jitter(2))


FLOOR_CAMERA = dict(cam=(0.0137, 0.0071, 0.0), front=(0.0, -0.3, -1.0))


def _floor(b, mat, uv=None):
    """y = -1, front up.  A ray scattered on it starts just under it (the
    shader's offset goes past the surface) and leaves through its culled back."""
    b.quad((-50, -1, 50), (100, 0, 0), (0, 0, -100), mat, uv)


def diffuse_floor(bounces=2):
    b = ss._Builder()
    _floor(b, b.material(DIFFUSE, color=(0.9, 0.6, 0.3)))
    rays, frames = ((3, (0, 1)) if bounces == 2 else (1, (5, 3)))
    return _with(b.scene(f"diffuse_floor/b{bounces}", W, H, bounces, rays, True, frames=frames, **FLOOR_CAMERA),
                 **_jitter(1))


def specular_mix():
    b = ss._Builder()
    _floor(b, b.material(SPECULAR, color=(0.8, 0.8, 0.2), prob=0.5, smooth=0.6))
    return _with(b.scene("specular_mix", W, H, 3, 3, True, frames=(5, 3), **FLOOR_CAMERA), **_jitter(1))


def floor_texture():
    """8 x 5 x 3, every channel in 60 .. 230: max(rayColor) stays below 1."""
    return np.random.default_rng(20240911).integers(60, 231, (5, 8, 3), dtype=np.uint8)


def texture_floor():
    b = ss._Builder()
    _floor(b, b.material(TEXTURE, texture=0), uv=[(-3.3, -2.1), (4.7, -2.1), (4.7, 5.2), (-3.3, 5.2)])
    return _with(b.scene("texture_floor", W, H, 3, 1, True, textures=[floor_texture()], frames=(0, 1),
                         **FLOOR_CAMERA), **_jitter(1))


def checker_floor():
    b = ss._Builder()
    _floor(b, b.material(CHECKER, checker=0.75))
    return _with(b.scene("checker_floor", W, H, 3, 3, True, frames=(0, 1), **FLOOR_CAMERA), **_jitter(1))


# Two more frames found the same way, on mirror_floor, where every ray's first
# hit draws a direction (three draws per candidate), then the probability draw,
# then the roulette's: at PROBABILITY_IS_ONE the probability draw of the pixel
# is 1.0, so `specularProbability > random` is 1.0 > 1.0 and the bounce is not
# specular; at ROULETTE_IS_ONE the roulette's is, so `random > p` is 1.0 > 1.0
# with p = 1 and the path survives.  `draw` counts from the seed.
PROBABILITY_IS_ONE = dict(frame=33998, x=1, y=15, draw=7)
ROULETTE_IS_ONE = dict(frame=3609, x=37, y=12, draw=8)


def mirror_floor(which, name):
    """Straight down onto a floor of specular probability 1 and smoothness 1
    that fills the image: no jitter, one ray, one frame."""
    b = ss._Builder()
    _floor(b, b.material(SPECULAR, color=(0.8, 0.8, 0.2), prob=1.0, smooth=1.0))
    return b.scene(name, W, H, 3, 1, True, frames=(which["frame"], 1), cam=FLOOR_CAMERA["cam"],
                   front=(0.0, -1.0, -0.3), right=(0.8, 0, 0), up=(0, 0, -0.6))


def glass_tinted():
    """The slab of shading_scenes.glass_slab in a colour that attenuates every
    channel: no scatter draw, one roulette draw with p = 0.9 per bounce."""
    b = ss._Builder()
    g = b.material(GLASS, color=(0.7, 0.9, 0.8), ior=1.5)
    ss._slab_front(b, g)
    b.quad((-2.8, -2.2, -3.2), (0, 4.4, -0.4), (5.6, 0, 0.5), g)
    return b.scene("glass_tinted", W, H, 12, 3, True, frames=(5, 3), front=ss.HORIZON_FRONT)


def edge_after_scatter():
    """Camera -> a mirror (plane z = x - 4, normal (-1, 0, 1)) that turns -z
    into -x -> a diffuse quad marked isEdgeHighlight in the plane x = -8, up to
    y = 0.7 -> the sky.  At bounce 2 the quad draws its scatter and drops it,
    keeps the direction and does not attenuate.  Nothing a pixel shows depends
    on that by itself; the 4-pixel jitter of the next ray, whose draws come
    after, does."""
    b = ss._Builder()
    b.quad((-14, -12, -18), (28, 0, 28), (0, 24, 0), b.mirror())
    b.quad((-8, -20, -30), (0, 20.7, 0), (0, 0, 60), b.material(DIFFUSE, color=(0.3, 1.0, 0.6), edge=1))
    s = b.scene("edge_after_scatter", W, H, 4, 3, True, frames=(0, 1), right=(0.5, 0, 0), up=(0, 0.36, 0))
    return _with(s, pixelRight=(4 * 1.0 / W, 0, 0), pixelUp=(0, 4 * 0.72 / H, 0))


def open_box():
    """Floor, ceiling, two sides and a back wall of different colours around
    (0, 0, -4), open towards the camera, and a light under the ceiling."""
    b = ss._Builder()
    h, c = 2.0, np.array([0.0, 0.0, -4.0])
    walls = (((0, -1, 0), (1, 0, 0), (0, 0, -1), (0.8, 0.8, 0.8)),     # floor: normal +y
             ((0, 1, 0), (1, 0, 0), (0, 0, 1), (0.9, 0.9, 0.7)),       # ceiling: -y
             ((-1, 0, 0), (0, 1, 0), (0, 0, 1), (0.9, 0.3, 0.2)),      # left: +x
             ((1, 0, 0), (0, 0, 1), (0, 1, 0), (0.2, 0.7, 0.3)),       # right: -x
             ((0, 0, -1), (1, 0, 0), (0, 1, 0), (0.4, 0.5, 0.9)))      # back: +z
    for at, eu, ev, colour in walls:
        at, eu, ev = (np.array(v, np.float64) for v in (at, eu, ev))
        assert np.allclose(np.cross(eu, ev), -at)
        b.quad(c + h * (at - eu - ev), 2 * h * eu, 2 * h * ev, b.material(DIFFUSE, color=colour))
    b.quad(c + (-0.7, h - 0.05, -0.7), (1.4, 0, 0), (0, 0, 1.4), b.light((1.0, 0.9, 0.7), 6.0))   # normal -y
    return _with(b.scene("open_box", W, H, 4, 2, True, frames=(5, 3), cam=(0.0137, 0.0071, 1.0)), **_jitter(1))


def all_scenes():
    """name -> scene, every row of the table in DESIGN.md "Random paths"."""
    out = [jitter_sky(1), jitter_sky(3), defocus_sky(), jitter_defocus_ramp(), diffuse_floor(2), diffuse_floor(3),
           specular_mix(), texture_floor(), checker_floor(), glass_tinted(), edge_after_scatter(), open_box(),
           draw_is_one(), mirror_floor(PROBABILITY_IS_ONE, "probability_is_one"),
           mirror_floor(ROULETTE_IS_ONE, "roulette_is_one")]
    return {s["name"]: s for s in out}
