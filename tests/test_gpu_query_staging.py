"""The staging set that a scene's seven blocking ray entry points share
(DESIGN.md "The query frame"): rays, RNG words and output bytes, each grown on
demand and reused by whichever call comes next.

One Scene runs a sequence of blocking calls of every family whose sizes grow
and shrink, so every buffer is both regrown and reused with another family's
bytes still in it, and whose counts cross the 64-ray chunk and the 32-lane
block.  Each result must equal, bit for bit, the same call on a fresh Scene of
the same data (whose buffers hold nothing else), the returned RNG words and
the segment counter included, and the last call must repeat the first.
"""
import numpy as np
import pytest

import closest_hit_scenes as S
import shade_scenes as H

pytestmark = pytest.mark.gpu

ARMS = ("auto", "scalar", "bvh")


def _make(rt2mod, sc, arm):
    if arm == "bvh":
        scene = rt2mod.Scene(S.scene_data(sc["triangles"], sc["materials"]))
        scene.set_traversal("bvh")
    else:
        scene = rt2mod.Scene(triangles=sc["triangles"], materials=sc["materials"])
    scene.set_textures(sc["textures"])
    return scene


def _view(rt2mod, sc):
    """A 9 x 7 view from the scene's first ray, with a defocus disk: path_rays draws for the origin too."""
    u = rt2mod.Uniforms()
    u.width, u.height = 9, 7
    u.numRaysPerPixel, u.environmentalLight, u.maxBounceCount = 1, 1, 4
    u.numTriangles, u.numTextures = len(sc["triangles"]), len(sc["textures"])
    o, f = sc["o"][0], sc["f"][0]
    right = np.cross(f, (0.0, 1.0, 0.0))
    up = np.cross(right, f)
    for name, v in (("cameraPos", o), ("viewportFront", f), ("viewportRight", 0.6 * right), ("viewportUp", 0.6 * up),
                    ("pixelRight", 1.2 / 9 * right), ("pixelUp", 1.2 / 7 * up), ("defocusDiskRight", 0.01 * right),
                    ("defocusDiskUp", 0.01 * up)):
        setattr(u, name, rt2mod.Vec4(float(v[0]), float(v[1]), float(v[2]), 0.0))
    return u


def _bits(result):
    """The call's arrays as bytes."""
    parts = result if isinstance(result, tuple) else (result,)
    return [np.ascontiguousarray(a).tobytes() for a in parts]


@pytest.mark.parametrize("arm", ARMS)
def test_shared_staging_across_families(rt2mod, arm):
    sc = H.soup(33)  # every material type: shade and radiance bounce
    assert len(np.unique(sc["materials"]["materialType"])) > 1
    flags = rt2mod.TRACE_SCALAR if arm == "scalar" else rt2mod.TRACE_AUTO
    o, d = sc["o"], sc["f"]
    tmax = np.where(np.arange(len(o)) % 3 == 0, 2.5, 0.0).astype(np.float32)  # bounded and unbounded rays
    seeds = (np.arange(65, dtype=np.uint32) * np.uint32(2654435761) + np.uint32(12345)).astype(np.uint32)
    u = _view(rt2mod, sc)
    steps = [
        ("trace_rays 130", lambda s: s.trace_rays(o[:130], d[:130], tmax[:130], flags)),
        ("radiance 65", lambda s: s.radiance(o[:65], d[:65], seeds, 8, True, flags)),
        ("occluded 1", lambda s: s.occluded(o[:1], d[:1], tmax[:1], flags)),
        ("surface 200", lambda s: s.surface(o[:200], d[:200], tmax[:200], flags)),
        ("shade_rays 64", lambda s: s.shade_rays(o[:64], d[:64], sc["light"], True, 3, flags)),
        ("camera_rays 9x7", lambda s: s.camera_rays(u)),
        ("path_rays 9x7", lambda s: s.path_rays(u, 5)),
        ("trace_rays 130 again", lambda s: s.trace_rays(o[:130], d[:130], tmax[:130], flags)),
    ]
    shared = _make(rt2mod, sc, arm)
    shared.stats(reset=True)
    got = []
    for name, call in steps:
        fresh = _make(rt2mod, sc, arm)
        fresh.stats(reset=True)
        want = call(fresh)
        want_kernel, want_segments = fresh.last_kernel(), fresh.stats(reset=True).segments
        have = call(shared)
        assert _bits(have) == _bits(want), name
        if "9x7" not in name:  # a ray generator is no query: it leaves the last query's code
            assert shared.last_kernel() == want_kernel, name
        assert shared.stats(reset=True).segments == want_segments, name
        got.append(have)
    assert _bits(got[7]) == _bits(got[0])
    # the calls did what their names say: hits and misses, paths of more than one segment, advanced streams
    dst, tri = got[0]
    assert (tri >= 0).any() and (tri < 0).any()
    assert (got[1][0]["segments"] > 1).any() and not np.array_equal(got[1][1], seeds)
    assert (got[4]["segments"] > 1).any()
    assert len(got[5]) == 63 and len(got[6][0]) == 63 and len(got[6][1]) == 63
