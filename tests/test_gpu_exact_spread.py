"""MfmaSpec::exact_spread on the GPU (rt2_k5_resident.h exact_window_lanes;
DESIGN.md "Leftover pairs on all lanes"): 353 / 354, which take the knob, and
in the experiment build their arms with the per-lane loop alone (420, 421) and
the diagnostic build (422), against the CPU oracle: image bits and segment
counts.  422's three counters are the numbers tests/exact_spread_scenes.py's
model predicts from the scenes' descriptions.  The scenes are one wave each
(tests/test_exact_spread_model.py checks what they are built to give):

  - a stack of 1, 2, 3, 33 and 40 triangles on one pixel, on a lane below 32
    and on one above, the nearest last (among the leftovers) and first (the
    lane's own first pair); a few other rays with one pair, the rest with none;
  - 62 .. 65 leftovers in one round (65: the per-lane loop), and 0 .. 3 over
    several stacked rays;
  - at most 32 live rays (20 x 1: lanes 32..63 hold no ray);
  - equal distances whose lower index sits in the later slot: first pair
    against leftover both ways, and two leftovers;
  - config B at 64 x 16, 4 rays, 8 bounces under the upload's slot order;
  - the negative control (423: a spread round's last entry is not tested):
    exactly the pixel the model names changes, to the colour it names."""
import ctypes as C

import numpy as np
import pytest

import closest_hit_scenes as S
import exact_spread_scenes as E
from conftest import EXPERIMENTS, require_variant

pytestmark = pytest.mark.gpu

RES, RES_SLAB, LOOP, LOOP_SLAB, DIAG, DROP = 353, 354, 420, 421, 422, 423
VARIANTS = (RES, RES_SLAB, LOOP, LOOP_SLAB, DIAG)
by_variant = pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: f"v{v}")

_ref = {}


def reference(oraclemod, key, tris, mats, u):
    """(the oracle's image, its segments), once per key, left unchanged."""
    if key not in _ref:
        acc, _, segs, _ = oraclemod.render(tris, mats, u, np.arange(u.height, dtype=np.int32), 0, 1, "brute")
        img = acc[..., :3]
        img.setflags(write=False)
        _ref[key] = (img, segs)
    return _ref[key]


def spread_counts(rt2mod, scene):
    """(leftovers summed, spread rounds, rounds that fell back on Rw > 64) of the diagnostic build's last render."""
    c = (C.c_ulonglong * 32)()
    rt2mod.lib().rt2_scene_diag_ex(scene._p, c, 32)
    return int(c[5]), int(c[12]) & ((1 << 40) - 1), int(c[12]) >> 40


def run(rt2mod, oraclemod, key, sc, variant, slot_tri=None, counters=True):
    """Renders scene `sc` on `variant` under slot_tri (default: the identity); the oracle's bits and segments; on
    the diagnostic build the model's counters.  -> (image, reference)."""
    import slot_order_scenes as sos
    require_variant(rt2mod, variant)
    tris, mats, u = sc["triangles"], sc["materials"], sc["uniforms"]
    st = np.arange(len(tris), dtype=np.int32) if slot_tri is None else slot_tri
    ref, segs = reference(oraclemod, key, tris, mats, u)
    scene = rt2mod.Scene(triangles=tris, materials=mats, device=0)
    scene.set_slot_order(st, sos.chunk_table(tris, st))
    scene.set_variant(variant)
    scene.stats(reset=True)
    img = scene.render_host(u, 0, 1)
    stats = scene.stats(reset=False)
    assert scene.last_kernel() == variant
    got = spread_counts(rt2mod, scene)
    scene.close()
    if variant != DROP:
        bad = (img[..., :3] != ref).any(-1)
        assert not bad.any(), f"variant {variant}, {key}: {bad.sum()} pixels differ, first at {np.argwhere(bad)[0]}"
        assert stats.segments == segs
    if variant == DIAG and counters:
        model, cnt = E.episode(E.pairs_of(sc, st), st)
        assert [m[1] for m in model] == S.decode(ref)[0].tolist()  # the model's winners are the oracle's
        print(f"{key}: leftovers, spread rounds, Rw > 64 rounds = {got}")
        assert got == (cnt["leftovers"], cnt["spread"], cnt["big"])
    return img, ref


@by_variant
@pytest.mark.parametrize("near_last", [True, False], ids=["near_last", "near_first"])
@pytest.mark.parametrize("px", [5, 40])
@pytest.mark.parametrize("n", [1, 2, 3, 33, 40])
def test_stacks(rt2mod, oraclemod, n, px, near_last, variant):
    sc = E.stack_scene(n, px, [0, 9, 33, 63], near_last)
    _, ref = run(rt2mod, oraclemod, ("stack", n, px, near_last), sc, variant)
    assert S.decode(ref)[0, px] == (n - 1 if near_last else 0)


@by_variant
@pytest.mark.parametrize("extra", [0, 1, 2, 3])
def test_leftovers_62_to_65(rt2mod, oraclemod, extra, variant):
    run(rt2mod, oraclemod, ("leftovers", extra), E.leftover_scene(extra), variant)


@by_variant
@pytest.mark.parametrize("left", sorted(E.FEW_LEFTOVERS))
def test_few_leftovers_from_several_rays(rt2mod, oraclemod, left, variant):
    """0, 1 and 2 leftovers over several stacked rays, no lane with two (the per-lane loop), and 3 with two on one
    lane (spread)."""
    run(rt2mod, oraclemod, ("few", left), E.stacks_scene(E.FEW_LEFTOVERS[left]), variant)


@by_variant
def test_at_most_32_live_rays(rt2mod, oraclemod, variant):
    """20 x 1: the wave sweeps one block, lanes 32..63 get a zero mask and only work for the others (the lanes
    without a ray carry the first live lane's, so the counters are not the scene's)."""
    sc = E.stack_scene(9, 13, [0, 2, 19], width=20)
    run(rt2mod, oraclemod, ("narrow",), sc, variant, counters=False)


@by_variant
@pytest.mark.parametrize("kind", ["first_loses", "first_wins", "workers"])
def test_ties_across_the_spread(rt2mod, oraclemod, kind, variant):
    sc, st = E.tie_scene(kind)
    _, ref = run(rt2mod, oraclemod, ("tie", kind), sc, variant, st)
    idx = S.decode(ref)[0]
    assert (idx[7], idx[50]) == ((1, 4) if kind == "workers" else (0, 3))  # the lower index of the duplicates


@by_variant
def test_config_B_small(rt2mod, oraclemod, config_scene, variant):
    require_variant(rt2mod, variant)
    sd, spec = config_scene("B")
    u = rt2mod.offline_uniforms(64, 16, 8, 4, sd.num_triangles)
    ref, segs = reference(oraclemod, "B", sd.triangles(), sd.materials(), u)
    scene = rt2mod.Scene(sd, 0)
    scene.set_variant(variant)
    scene.stats(reset=True)
    img = scene.render_host(u, 0, 1)
    stats = scene.stats(reset=False)
    assert scene.last_kernel() == variant
    left, spread, big = spread_counts(rt2mod, scene)
    scene.close()
    bad = (img[..., :3] != ref).any(-1)
    assert not bad.any(), f"variant {variant}, config B: {bad.sum()} pixels differ, first at {np.argwhere(bad)[0]}"
    assert stats.segments == segs
    if variant == DIAG:
        print(f"config B 64 x 16: leftovers, spread rounds, Rw > 64 rounds = {left, spread, big}")
        assert spread > 0 and left >= 2 * spread  # the path under test ran


@pytest.mark.skipif(not EXPERIMENTS, reason="the arm that drops an entry is in the experiment build")
def test_negative_control(rt2mod, oraclemod):
    """423 leaves a spread round's last list entry untested.  A stack of 3 with the nearest last: the entry is the
    nearest triangle's, so pixel 20 shows the second nearest and no other pixel changes."""
    sc = E.stack_scene(3, 20, [3, 41])
    st = np.arange(5, dtype=np.int32)
    model, _ = E.episode(E.pairs_of(sc, st), st, drop=True)
    img, ref = run(rt2mod, oraclemod, ("control",), sc, DROP)
    diff = (img[..., :3] != ref).any(-1)
    assert np.argwhere(diff).tolist() == [[0, 20]]
    assert S.decode(img)[0, 20] == model[20][1] == 1 and S.decode(ref)[0, 20] == 2
    run(rt2mod, oraclemod, ("control",), sc, RES)  # the same scene on the shipped kernel: the oracle's image
