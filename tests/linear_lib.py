"""Linear renders (rt2_render_linear): the accumulation rule of include/rt2.h in
numpy, the yardstick built from the oracle-pinned query chain, and the views
the tests compare.  Host half of tests/test_gpu_linear.py; what it states
without a GPU is checked by tests/test_linear_cpu.py.
"""
import numpy as np

import radiance_scenes as R
import shade_scenes as H
import shading_scenes as ss

F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def accumulate(samples, sums=None, sumsq=None):
    """rt2_render_linear's rule on per-sample values.  samples: float32
    [frames][R][n][3], v_s of every pixel in sample order, frames in increasing
    order.  Per frame and channel: c = q = 0, then c = c + v_s and q = q +
    RN(v_s * v_s) (the product rounded to binary32, then the sum), m = c / R,
    m2 = q / R, sum += m, sumsq += m2.  Returns float32 (sum, sumsq) of shape
    [n][4] with .w = 0, continuing from `sums` / `sumsq` when given."""
    samples = np.asarray(samples, F32)
    frames, rays, n, _ = samples.shape
    total = np.zeros((n, 4), F32) if sums is None else np.array(sums, F32)
    total2 = np.zeros((n, 4), F32) if sumsq is None else np.array(sumsq, F32)
    with np.errstate(all="ignore"):
        for f in range(frames):
            c, q = np.zeros((n, 3), F32), np.zeros((n, 3), F32)
            for s in range(rays):
                v = samples[f, s]
                c = (c + v).astype(F32)
                sq = (v * v).astype(F32)  # numpy float32 arithmetic rounds every operation: no fused multiply-add
                q = (q + sq).astype(F32)
            m, m2 = (c / F32(rays)).astype(F32), (q / F32(rays)).astype(F32)
            total[:, :3] = (total[:, :3] + m).astype(F32)
            total2[:, :3] = (total2[:, :3] + m2).astype(F32)
            total[:, 3] = 0.0
            total2[:, 3] = 0.0
    return total, total2


def chain_samples(rt2mod, scene, u, frame_begin, frame_count, sh=None):
    """v_s of every pixel of the slab from the query chain with
    RT2_TRACE_SCALAR: per frame Scene.path_rays (reseeded on the first sample
    only) and Scene.radiance, numRaysPerPixel times on one stream array.
    Returns (float32 [frames][R][n][3], segments summed)."""
    rays_pp = int(u.numRaysPerPixel)
    out, segs = [], 0
    for f in range(frame_begin, frame_begin + frame_count):
        per, rng = [], None
        for _ in range(rays_pp):
            rays, rng = scene.path_rays(u, f, sh, rng)
            rec, rng = scene.radiance(rays["o"], rays["d"], rng, int(u.maxBounceCount), bool(u.environmentalLight),
                                      rt2mod.TRACE_SCALAR)
            per.append(rec["rgb"].copy())
            segs += int(rec["segments"].sum())
        out.append(per)
    return np.array(out, F32), segs


# ---- views ----------------------------------------------------------------------------------------------------------

SMALL_RAYS = (1, 3, 65)      # 65: one item outlives its wave's other lanes
SMALL_BOUNCES = (1, 8)
# compared through the tonemap: every view of the radiance tests but the 67 x 10 emissive ramp, where more than a
# tenth of the channel values sit at the tonemap's ceiling of 1.0 (test_linear_cpu asserts the cap on the others)
TONEMAP_VIEWS = [(name, w, h) for name in sorted(R.VIEW_SCENES) for w, h in R.VIEW_SIZES
                 if (name, w, h) != ("jitter_defocus_ramp", 67, 10)]
TONEMAP_RAYS = 3
TONEMAP_FRAMES = (5, 3)  # first frame, count


def corridor_view(w=64, h=4, rays=3):
    """The facing mirrors of the radiance tests seen from the axis: pixel
    columns fan out sideways (slope 1 / (3 |px|)), so neighbouring lanes end at
    different bounces: on a patch, the light, the open end or the limit."""
    sc = H.corridor()
    un = dict(width=w, height=h, numTriangles=len(sc["triangles"]), environmentalLight=1, maxBounceCount=8,
              numRaysPerPixel=rays, numTextures=0, cameraPos=(0.0, 0.0, 0.25), viewportFront=(0.0, 0.0, -1.0),
              viewportRight=(3.0, 0.0, 0.0), viewportUp=(0.0, 0.5, 0.0), pixelRight=(0.01, 0.0, 0.0),
              pixelUp=(0.0, 0.01, 0.0), defocusDiskRight=(0.0, 0.0, 0.0), defocusDiskUp=(0.0, 0.0, 0.0))
    return dict(name="lin_corridor", triangles=sc["triangles"], materials=sc["materials"], textures=[], uniforms=un)


CONSTANT_EMISSION = (4.0, 1.0, 0.25)


def constant_view(w=24, h=6, rays=4):
    """One emissive triangle, no sky, no jitter, no defocus: a pixel's samples
    are the same ray, so every path of a pixel returns the same value,
    CONSTANT_EMISSION on the triangle and 0 beside it."""
    b = ss._Builder()
    lit = b.light(CONSTANT_EMISSION, 1.0)
    b.quad((-0.5, -0.4, -1.0), (1.1, 0.0, 0.0), (0.0, 0.9, 0.0), lit)
    b.tris = b.tris[:1]
    return dict(b.scene("lin_constant", w, h, 4, rays, False), name="lin_constant")
