"""The resident kernel's exact phase per window of groups (rt2_k5_resident.h
exact_window) against the CPU oracle, as decoded winners.

Inside a window the filter works with the bound the window started with, so
triangles pass it that the per-group form would have rejected; the exact phase
must still give every pixel to the sequential strict `dst < best` scan's
winner.  Every case runs on each resident variant of the loaded library: the
automatic kernels 353-356 and, in the experiment build, every A/B arm whose
name carries /xw (window) or /xb (batched loads).  A case is skipped on a
variant that cannot hold its scene.

  a. fans (every triangle covers every pixel: every mask of every window is
     full) in the three orders, n = 32 ng - 13 with ng at the window edges of
     the default window and of the largest one built, at the resident limit
     (38) and one past it (39: the L2 loop);
  b. exact ties whose copies lie in two groups of one window, in the last
     group of a window and the first of the next, and in groups 37 and 38;
     test_tie_families_tie checks on the oracle alone (no GPU) that every
     family ties and that its lowest index wins;
  c. an 8x3 and a 10x4 image of the 1,216-triangle soup (24 live rays: only
     the lower 32-ray block from the first segment on; 40: compaction once
     lanes finish);
  d. incoherent rays: the mixed soup of 1,216 triangles, 4 rays, 4 bounces.
"""
import re

import numpy as np
import pytest

import closest_hit_scenes as S
from conftest import require_variant
from test_gpu_closest_hit import _ran, _ref, _render, _same_bits, _same_winners

gpu = pytest.mark.gpu

DEFAULT_W = 38   # rt2_render.hip kResWin: the window of 353 and 355
LARGEST_W = 38   # the largest window among the A/B arms (the whole resident sweep)
ARM_WS = (2, 4, 8, 19, 38)  # the windows of the A/B arms: the tie families cover each
RES_GROUPS = 38  # rt2_k5_resident.h kResGroups
RES_L2_GROUPS = 256


def _resident_variants():
    """353-356 and every /xw, /xb arm of the loaded library, with the groups each holds."""
    import rt2
    out = []
    for v in range(130, 400):
        name = rt2.lib().rt2_variant_name(v)
        if not name:
            continue
        name = name.decode()
        if v in (353, 354, 355, 356) or (name.startswith(("mfmar/", "mfmarl2/")) and re.search(r"/x[wb]\d", name)):
            out.append(v)
    return out


VARIANTS = _resident_variants()


def _fits(rt2mod, variant, n):
    require_variant(rt2mod, variant)
    name = rt2mod.lib().rt2_variant_name(variant).decode()
    limit = RES_GROUPS if name.startswith("mfmar/") else RES_L2_GROUPS
    if S.n_groups(n) > limit:
        pytest.skip(f"variant {variant} holds scenes of <= {limit} groups")


def _check_coded(rt2mod, oraclemod, key, tris, mats, w, h, variant, what):
    n = len(tris)
    _fits(rt2mod, variant, n)
    u = S.coded_uniforms(w, h, n)
    ref, segs = _ref(oraclemod, key, tris, mats, u, "brute")
    img, gsegs, ran = _render(rt2mod, key, tris, mats, u, variant)
    _ran(rt2mod, ran, variant)
    _same_winners(img, ref, f"{what}, variant {variant}")
    assert gsegs == segs == w * h


# ---- a. fans -------------------------------------------------------------------

def _edge_groups(w):
    return {1, w - 1, w, w + 1, 2 * w, 2 * w + 1, RES_GROUPS, RES_GROUPS + 1} - {0}


FAN_GROUPS = sorted(_edge_groups(DEFAULT_W) | _edge_groups(LARGEST_W))
_fans = {}


def _fan(ng, order):
    if (ng, order) not in _fans:
        n = 32 * ng - 13
        t, m = S.fan(n, S.FAN_SEED, order), S.code_materials(n)
        t.setflags(write=False)
        m.setflags(write=False)
        _fans[(ng, order)] = (t, m)
    return _fans[(ng, order)]


@gpu
@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: f"v{v}")
@pytest.mark.parametrize("order", ["near_first", "far_first", "shuffled"])
@pytest.mark.parametrize("ng", FAN_GROUPS)
def test_fans(rt2mod, oraclemod, ng, order, variant):
    tris, mats = _fan(ng, order)
    _check_coded(rt2mod, oraclemod, ("xw-fan", ng, order), tris, mats, 64, 36, variant, f"fan {order}, {ng} groups")


# ---- b. ties -------------------------------------------------------------------

TIE_SIZES = (1216, 32 * 44 - 13)  # 38 full groups (every variant); 44 groups, the last ragged (the L2 loop's)


def _copy_slot(g, k, n):
    """A slot of group g other than its champion's (window_tie_families asserts it)."""
    return 32 * g + (7 * g + 13 + 5 * k) % min(32, n - 32 * g)


def window_tie_families(n):
    """For every pair of groups (g1 < g2) below, two families: group g1's
    champion copied into g2 (the copy passes the filter on the window's stale
    bound and must lose the strict <) and group g2's champion copied into g1
    (the copy, the lower index, must win).  The pairs, for each window W of
    ARM_WS and DEFAULT_W: two groups inside one window; the last group of a
    window and the first of the next.  Scenes past 38 groups add groups 37 and
    38 (the resident loop's last and the L2 loop's first), 39 and 40 (the L2
    loop's windows start again at 38: an edge for W = 2) and 42 and 43 (one
    window there for every W)."""
    pairs = [(16, 17), (21, 22),   # W = 2: window [16, 17]; windows [20, 21] | [22, 23]
             (4, 6), (11, 12),     # W = 4: window [4, 7]; [8, 11] | [12, 15]
             (24, 29), (31, 32),   # W = 8: window [24, 31]; [24, 31] | [32, 37]
             (18, 19),             # W = 19: [0, 18] | [19, 37] (one window there: the pairs above)
             (2, 35)]              # W = 38: the whole resident sweep
    if DEFAULT_W > 1 and DEFAULT_W not in ARM_WS:
        raise ValueError("add the default window's pairs")
    ng = S.n_groups(n)
    if ng > RES_GROUPS:
        pairs += [(37, 38), (39, 40), (42, 43)]
    fams = []
    for g1, g2 in pairs:
        fams.append([S.champ(g1, n), _copy_slot(g2, 0, n)])
        fams.append([S.champ(g2, n), _copy_slot(g1, 1, n)])
    used = [i for f in fams for i in f]
    assert len(set(used)) == len(used) and max(used) < n
    champs = {S.champ(g, n) for g in range(ng)}
    assert all(f[1] not in champs for f in fams)
    return fams


_ties = {}


def _tie_scene(n):
    if n not in _ties:
        t, m = S.with_ties(S.soup(n, S.SOUP_SEED), window_tie_families(n)), S.code_materials(n)
        t.setflags(write=False)
        m.setflags(write=False)
        _ties[n] = (t, m)
    return _ties[n]


@pytest.mark.parametrize("n", TIE_SIZES)
def test_tie_families_tie(rt2mod, oraclemod, n):
    """On the oracle alone: every family's members are the same triangle bit
    for bit, the family's lowest index is the closest hit of some pixels and no
    other member wins any."""
    tris, mats = _tie_scene(n)
    ref, _ = _ref(oraclemod, ("xw-ties", n), tris, mats, S.coded_uniforms(64, 36, n), "brute")
    idx = S.decode(ref)
    for fam in window_tie_families(n):
        assert all(np.array_equal(tris[k][fam[1]], tris[k][fam[0]]) for k in "abc")
        own = {i: int((idx == i).sum()) for i in fam}
        low = min(fam)
        assert own[low] >= 3, f"family {fam}: {own}"
        assert own[max(fam)] == 0, f"family {fam}: {own}"


@gpu
@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: f"v{v}")
@pytest.mark.parametrize("n", TIE_SIZES)
def test_ties(rt2mod, oraclemod, n, variant):
    tris, mats = _tie_scene(n)
    _check_coded(rt2mod, oraclemod, ("xw-ties", n), tris, mats, 64, 36, variant, f"ties, {n} triangles")


# ---- c. small images -------------------------------------------------------------

@gpu
@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: f"v{v}")
@pytest.mark.parametrize("w,h", [(8, 3), (10, 4)])
def test_small_images(rt2mod, oraclemod, w, h, variant):
    tris, mats = S.coded_scene("soup", 1216)
    _check_coded(rt2mod, oraclemod, ("soup", 1216), tris, mats, w, h, variant, f"soup, {w}x{h}")


# ---- d. incoherent rays ------------------------------------------------------------

@gpu
@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: f"v{v}")
def test_incoherent_rays(rt2mod, oraclemod, variant):
    n = 1216
    _fits(rt2mod, variant, n)
    tris, mats = S.mixed_scene(n)
    u = rt2mod.offline_uniforms(64, 36, 4, 4, n)
    ref, segs = _ref(oraclemod, ("mixed", n), tris, mats, u, "brute")
    img, gsegs, ran = _render(rt2mod, ("mixed", n), tris, mats, u, variant)
    _ran(rt2mod, ran, variant)
    _same_bits(img, ref, f"mixed soup, 4 rays, 4 bounces, variant {variant}")
    assert gsegs == segs > 64 * 36 * 4
