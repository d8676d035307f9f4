"""The resident kernel's exact tests per ray (MfmaSpec::exact_lanes,
rt2_k5_resident.h exact_window_lanes) against the CPU oracle: image bits,
decoded winners, segment counts, and which kernel ran.

Every case runs on the shipped kernels that take the knob (SHIPPED) and, in
the experiment build, on every arm whose name ends in /xl.  A case is skipped
on a variant that cannot hold its scene.  tests/test_exact_lanes_model.py
checks without a GPU what the scenes are built to give.

  a. fans in which every ray hits all n triangles (k = n: the per-lane loop
     runs long), n at the round edges 1, 31, 32, 33, 64, 65, and n = 32 ng - 13
     with the last group hot (padding cut at the compaction), ng up to 38 and
     39 (the L2 loop's window and the Y rebuild);
  b. 32 and 33 triangles each hit by one ray of its own, in scrambled order
     (the bit <-> row map and the block swap), at 8x4 and 11x3;
  c. exact ties between slots 31 and 32 of a sweep (two rounds), between bits
     15 and 16 of a round and across groups: the lower index wins;
  d. one ray with 40 pairs while the other 63 have none, and 63 rays with 40
     pairs each while one has none;
  e. 8x3 and 10x4 images of the 1,216-triangle soup (one block; compaction of
     the live rays to the low lanes; upper = false);
  f. the soups and tie scenes of 1,216 and 1,217 triangles (38 and 39 groups);
  g. incoherent rays (the mixed soup, 4 rays, 4 bounces);
  h. a camera outside the filter's range (the cooperative fallback);
  i. trace_rays with a finite tmax on the resident path (a bound from the
     sweep's start), experiment build only (query arm 3).
"""
import ctypes as C
import re

import numpy as np
import pytest

import closest_hit_scenes as S
import exact_lanes_scenes as X
from conftest import EXPERIMENTS, require_variant
from test_gpu_closest_hit import _ran, _ref, _render, _same_bits, _same_winners
from test_gpu_exact_window import _fan

gpu = pytest.mark.gpu

SHIPPED = (353, 354)  # rt2_render.hip: the automatic kernels built with exact_lanes
RES_GROUPS = 38
RES_L2_GROUPS = 256


def _variants():
    import rt2
    out = list(SHIPPED)
    for v in range(130, 500):
        name = rt2.lib().rt2_variant_name(v)
        if name and name.decode().endswith("/xl") and v not in out:
            out.append(v)
    return out


VARIANTS = _variants()
by_variant = pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: f"v{v}")


def _fits(rt2mod, variant, n):
    require_variant(rt2mod, variant)
    name = rt2mod.lib().rt2_variant_name(variant).decode()
    limit = RES_GROUPS if name.startswith("mfmar/") else RES_L2_GROUPS
    if S.n_groups(n) > limit:
        pytest.skip(f"variant {variant} holds scenes of <= {limit} groups")


def _check(rt2mod, oraclemod, key, tris, mats, u, variant, what, segs_are=None):
    _fits(rt2mod, variant, len(tris))
    ref, segs = _ref(oraclemod, key, tris, mats, u, "brute")
    img, gsegs, ran = _render(rt2mod, key, tris, mats, u, variant)
    _ran(rt2mod, ran, variant)
    _same_winners(img, ref, f"{what}, variant {variant}")
    assert gsegs == segs
    if segs_are is not None:
        assert segs == segs_are
    return ref


# ---- a. fans ---------------------------------------------------------------------

_small_fans = {}


def _small_fan(n, order):
    if (n, order) not in _small_fans:
        t, m = S.fan(n, S.FAN_SEED, order), S.code_materials(n)
        t.setflags(write=False)
        m.setflags(write=False)
        _small_fans[(n, order)] = (t, m)
    return _small_fans[(n, order)]


@gpu
@by_variant
@pytest.mark.parametrize("order", ["far_first", "near_first", "shuffled"])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 64, 65])
def test_fans_round_edges(rt2mod, oraclemod, n, order, variant):
    tris, mats = _small_fan(n, order)
    _check(rt2mod, oraclemod, ("xl-fan", n, order), tris, mats, S.coded_uniforms(64, 36, n), variant,
           f"fan {order}, {n} triangles", 64 * 36)


@gpu
@by_variant
@pytest.mark.parametrize("order", ["far_first", "shuffled"])
@pytest.mark.parametrize("ng", [1, 2, 3, 38, 39])
def test_fans_ragged_last_group(rt2mod, oraclemod, ng, order, variant):
    tris, mats = _fan(ng, order)  # 32 ng - 13 triangles, the window tests' scenes and references
    _check(rt2mod, oraclemod, ("xw-fan", ng, order), tris, mats, S.coded_uniforms(64, 36, len(tris)), variant,
           f"fan {order}, {ng} groups", 64 * 36)


# ---- b. one ray per triangle -----------------------------------------------------

@gpu
@by_variant
@pytest.mark.parametrize("w,h", [(8, 4), (11, 3)])
def test_one_ray_per_triangle(rt2mod, oraclemod, w, h, variant):
    tris, mats, u, order = X.one_ray_each(w, h)
    ref = _check(rt2mod, oraclemod, ("xl-one", w, h), tris, mats, u, variant, f"one ray per triangle, {w}x{h}", w * h)
    assert np.array_equal(S.decode(ref).ravel(), order)  # the premise, on the oracle's image


# ---- c. ties ---------------------------------------------------------------------

@gpu
@by_variant
def test_ties_between_rounds_halves_and_groups(rt2mod, oraclemod, variant):
    tris, mats = X.plane_fan(X.TIE_N, X.TIE_FAMILIES)
    ref = _check(rt2mod, oraclemod, ("xl-ties",), tris, mats, S.coded_uniforms(64, 36, X.TIE_N), variant, "ties",
                 64 * 36)
    won = set(S.decode(ref).ravel().tolist())
    for (lo, hi), _ in X.TIE_FAMILIES:
        assert lo in won and hi not in won  # the premise: every family wins somewhere, by its lower index


# ---- d. one ray against 63 -------------------------------------------------------

@gpu
@by_variant
def test_one_ray_with_many_pairs(rt2mod, oraclemod, variant):
    tris, mats, u = X.one_ray_many(8, 8, 40, 5, 3)
    ref = _check(rt2mod, oraclemod, ("xl-one-many",), tris, mats, u, variant, "one ray with 40 pairs", 64)
    idx = S.decode(ref)
    assert idx[3, 5] == 39 and (idx >= 0).sum() == 1


@gpu
@by_variant
def test_all_rays_but_one_with_many_pairs(rt2mod, oraclemod, variant):
    tris, mats, u = X.all_rays_but_one(8, 8, 40)
    ref = _check(rt2mod, oraclemod, ("xl-but-one",), tris, mats, u, variant, "63 rays with 40 pairs", 64)
    idx = S.decode(ref)
    assert idx[0, 0] == -1 and (idx == 39).sum() == 63


# ---- e. small images; f. 38 and 39 groups -----------------------------------------

@gpu
@by_variant
@pytest.mark.parametrize("w,h", [(8, 3), (10, 4)])
def test_small_images(rt2mod, oraclemod, w, h, variant):
    tris, mats = S.coded_scene("soup", 1216)
    _check(rt2mod, oraclemod, ("soup", 1216), tris, mats, S.coded_uniforms(w, h, 1216), variant, f"soup, {w}x{h}",
           w * h)


@gpu
@by_variant
@pytest.mark.parametrize("kind", ["soup", "ties"])
@pytest.mark.parametrize("n", [1216, 1217])
def test_resident_edge(rt2mod, oraclemod, n, kind, variant):
    tris, mats = S.coded_scene(kind, n)
    _check(rt2mod, oraclemod, (kind, n), tris, mats, S.coded_uniforms(64, 36, n), variant, f"{kind}, {n} triangles",
           64 * 36)


# ---- g. incoherent rays ------------------------------------------------------------

@gpu
@by_variant
@pytest.mark.parametrize("n", [1216, 1217])
def test_incoherent_rays(rt2mod, oraclemod, n, variant):
    _fits(rt2mod, variant, n)
    tris, mats = S.mixed_scene(n)
    u = rt2mod.offline_uniforms(64, 36, 4, 4, n)
    ref, segs = _ref(oraclemod, ("mixed", n), tris, mats, u, "brute")
    img, gsegs, ran = _render(rt2mod, ("mixed", n), tris, mats, u, variant)
    _ran(rt2mod, ran, variant)
    _same_bits(img, ref, f"mixed soup, {n} triangles, 4 rays, 4 bounces, variant {variant}")
    assert gsegs == segs > 64 * 36 * 4


# ---- h. outside the filter's range -----------------------------------------------

@gpu
@by_variant
def test_camera_outside_the_filters_range(rt2mod, oraclemod, variant):
    n = 300
    _fits(rt2mod, variant, n)
    tris, mats = S.mixed_scene(n)
    u = rt2mod.offline_uniforms(40, 30, 4, 2, n)
    u.cameraPos.z = float(2 ** 21)
    ref, segs = _ref(oraclemod, ("mixed-far", n), tris, mats, u, "brute")
    img, gsegs, ran = _render(rt2mod, ("mixed-far", n), tris, mats, u, variant)
    _ran(rt2mod, ran, variant)
    _same_bits(img, ref, f"camera 2^21 away, variant {variant}")
    assert gsegs == segs


# ---- i. ray queries with a bound ----------------------------------------------------

@gpu
@pytest.mark.skipif(not EXPERIMENTS, reason="the query kernel's exact_lanes arm is in the experiment build")
@pytest.mark.parametrize("k", [1, 32, 33, 64, 193])
def test_trace_rays_with_tmax(rt2mod, oraclemod, k):
    import trace_rays_lib as T
    n = 1216
    o, d = T.scene_rays("soup", n, 193)
    dst, tri, _ = T.scene_ref(oraclemod, "soup", n, 193)
    o, d, dst, tri = o[:k], d[:k], dst[:k], tri[:k]
    scene = rt2mod.Scene(triangles=T.scene_tris("soup", n), materials=S.code_materials(n))
    f = rt2mod.lib().rt2_scene_set_query_arm
    f.argtypes = [C.c_void_p, C.c_int]
    assert f(scene._p, 3) == 0
    hit = tri >= 0
    # just above every hit: the same hits, with a bound from the first product on; at the hit: strict, a miss
    for scale, want_tri in ((np.float32(1.5), tri), (np.float32(1.0), np.full(k, -1, np.int32))):
        tmax = np.where(hit, dst * scale, np.float32(7.0)).astype(np.float32)
        gd, gt = scene.trace_rays(o, d, tmax)
        assert scene.last_kernel() == rt2mod.QUERY_RES
        want_dst = np.where(want_tri >= 0, dst, tmax).astype(np.float32)
        bad = (gd.view(np.uint32) != want_dst.view(np.uint32)) | (gt != want_tri)
        assert not bad.any(), f"{int(bad.sum())} of {k} rays differ (tmax = {scale} dst), first {np.flatnonzero(bad)[:4]}"
