"""The resident kernel's first window without the Y product (rt2_mfma.h
kt_group<false>, MfmaSpec::y_first) against the CPU oracle, as decoded winners.

While no ray of a sweep has a distance bound, the Y product is only the
det > 0 test, which U, -V and X imply; the first window of every sweep leaves
it out and the Y fragment is first built after that window.  What can go wrong:
a back face passing where it did not before and winning; a later window
running on a Y fragment that was never built (whether or not the first window
found anything); padding slots, which now pass for every ray, being tested.

Every case runs on 353-356 and, in the experiment build, on each arm that
keeps Y in the first window (names ending in /yw).  A case is skipped on a
variant that cannot hold its scene.  The premises of scenes a and b are checked
on the oracle alone (no GPU) by the tests without the gpu mark.

  a. back faces: 608 soup triangles and, at lower indices, their copies with
     reversed winding (1,216), and the same with 13 cut from the end;
  b. 39 and 44 groups (the last ragged) with nothing to find in groups 0-37
     (behind the camera: masks are set, every exact test rejects; off to the
     side: no mask is set) and a fan behind them; and a fan in groups 0-37 with
     one nearer triangle per later group, the rest farther;
  c. the window tie families of test_gpu_exact_window at both sizes;
  d. fans of 1, 19, 32*38 - 13, 32*38 and 32*39 - 13 triangles (padding);
  e. an 8x3 and a 10x4 image of the 1,216-triangle soup (24 live rays: only
     the lower 32-ray block; 40: compaction once lanes finish);
  f. incoherent rays: the mixed soups of 1,216 and 1,217 triangles, 4 rays,
     4 bounces, bit for bit.
"""
import numpy as np
import pytest

import closest_hit_scenes as S
from test_gpu_closest_hit import _ran, _ref, _render, _same_bits
from test_gpu_exact_window import TIE_SIZES, _check_coded, _fits, _tie_scene

gpu = pytest.mark.gpu

RES_TRIS = 32 * 38  # rt2_k5_resident.h kResGroups groups: the first window of 353-356
W, H = 64, 36


def _variants():
    """353-356 and every /yw arm of the loaded library."""
    import rt2
    out = []
    for v in range(130, 400):
        name = rt2.lib().rt2_variant_name(v)
        if name and (v in (353, 354, 355, 356) or name.decode().endswith("/yw")):
            out.append(v)
    return out


VARIANTS = _variants()
on_variants = pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: f"v{v}")

_built = {}


def _scene(key, make):
    """(triangles, materials) of an index-coded scene, built once and read-only."""
    if key not in _built:
        t = make()
        t["materialIndex"] = np.arange(len(t))
        m = S.code_materials(len(t))
        t.setflags(write=False)
        m.setflags(write=False)
        _built[key] = (t, m)
    return _built[key]


def _oracle_winners(oraclemod, key, tris, mats):
    ref, _ = _ref(oraclemod, key, tris, mats, S.coded_uniforms(W, H, len(tris)), "brute")
    return S.decode(ref)


# ---- a. back faces ---------------------------------------------------------------

BACK_SIZES = (1216, 1216 - 13)
N_FRONT = 608


def _back_faces(n):
    def make():
        front = S.soup(N_FRONT, S.SOUP_SEED)
        # soup() winds for n.z > 0; seen from the camera a few of those are still
        # back faces: wind every front face towards the camera itself
        a, b, c = (front[k][:, :3].astype(np.float64) for k in "abc")
        back = (np.cross(b - a, c - a) * (np.array(S.CAMERA) - a)).sum(1) < 0
        front["b"][back], front["c"][back] = front["c"][back].copy(), front["b"][back].copy()
        rev = front.copy()
        rev["b"], rev["c"] = front["c"], front["b"]
        return np.concatenate([rev, front])[:n]
    return _scene(("back", n), make)


@pytest.mark.parametrize("n", BACK_SIZES)
def test_back_faces_premise(rt2mod, oraclemod, n):
    """On the oracle alone: no reversed triangle wins, and every winner has its
    reversed twin (the same three vertices) at a lower index."""
    tris, mats = _back_faces(n)
    idx = _oracle_winners(oraclemod, ("back", n), tris, mats)
    won = np.unique(idx[idx >= 0])
    assert len(won) >= 19  # the champions of the 19 front groups at least
    assert won.min() >= N_FRONT
    twin = won - N_FRONT
    assert np.array_equal(tris["a"][twin], tris["a"][won])
    assert np.array_equal(tris["b"][twin], tris["c"][won]) and np.array_equal(tris["c"][twin], tris["b"][won])


@gpu
@on_variants
@pytest.mark.parametrize("n", BACK_SIZES)
def test_back_faces(rt2mod, oraclemod, n, variant):
    tris, mats = _back_faces(n)
    _check_coded(rt2mod, oraclemod, ("back", n), tris, mats, W, H, variant, f"back faces, {n} triangles")


# ---- b. a first window with nothing to find, and its opposite -------------------------

LATE_GROUPS = (39, 44)  # n = 32 ng - 13: one ragged group after the first window; six, the last ragged


def _moved(tris, dx, dz):
    t = tris.copy()
    for k in "abc":
        t[k][:, 0] += np.float32(dx)
        t[k][:, 2] += np.float32(dz)
    return t


def _empty_first_window(ng, where):
    """Groups 0-37: the soup moved behind the camera (every line of sight still
    pierces some of them, at a negative distance) or 60 units to the side (no
    line of sight meets any); groups 38 and up: a fan."""
    def make():
        soup = S.soup(RES_TRIS, S.SOUP_SEED)
        away = _moved(soup, 0.0, 20.0) if where == "behind" else _moved(soup, 60.0, 0.0)
        return np.concatenate([away, S.fan(32 * ng - 13 - RES_TRIS, S.FAN_SEED, "shuffled")])
    return _scene(("late-fan", ng, where), make)


def _late_champions(ng):
    """Indices of the one nearer triangle of every group from 38 on."""
    m = 32 * ng - 13 - RES_TRIS
    return [RES_TRIS + S.champ(g, m) for g in range(S.n_groups(m))]


def _near_after_fan(ng):
    """Groups 0-37: a fan (around z = 0); groups 38 and up: a soup 6 units
    farther than the index-coded one (z <= -2: behind the fan) whose champions
    stay in the plane z = 5, in front of the fan."""
    def make():
        m = 32 * ng - 13 - RES_TRIS
        late = _moved(S.soup(m, S.SOUP_SEED), 0.0, -6.0)
        for i in _late_champions(ng):
            for k in "abc":
                late[k][i - RES_TRIS, 2] = S.CHAMP_Z
        return np.concatenate([S.fan(RES_TRIS, S.FAN_SEED, "shuffled"), late])
    return _scene(("late-near", ng), make)


@pytest.mark.parametrize("where", ["behind", "aside"])
@pytest.mark.parametrize("ng", LATE_GROUPS)
def test_empty_first_window_premise(rt2mod, oraclemod, ng, where):
    """On the oracle alone: every pixel's winner is in group 38 or later."""
    tris, mats = _empty_first_window(ng, where)
    idx = _oracle_winners(oraclemod, ("late-fan", ng, where), tris, mats)
    assert idx.min() >= RES_TRIS


@pytest.mark.parametrize("ng", LATE_GROUPS)
def test_near_after_fan_premise(rt2mod, oraclemod, ng):
    """On the oracle alone: every pixel has a winner; the winners from group 38
    on are exactly the nearer triangles, one per group, and the fan wins the
    rest."""
    tris, mats = _near_after_fan(ng)
    idx = _oracle_winners(oraclemod, ("late-near", ng), tris, mats)
    assert idx.min() >= 0
    late = np.unique(idx[idx >= RES_TRIS])
    assert list(late) == sorted(_late_champions(ng))
    assert (idx < RES_TRIS).sum() > idx.size // 2


@gpu
@on_variants
@pytest.mark.parametrize("where", ["behind", "aside"])
@pytest.mark.parametrize("ng", LATE_GROUPS)
def test_empty_first_window(rt2mod, oraclemod, ng, where, variant):
    tris, mats = _empty_first_window(ng, where)
    _check_coded(rt2mod, oraclemod, ("late-fan", ng, where), tris, mats, W, H, variant,
                 f"soup {where}, then a fan, {ng} groups")


@gpu
@on_variants
@pytest.mark.parametrize("ng", LATE_GROUPS)
def test_near_after_fan(rt2mod, oraclemod, ng, variant):
    tris, mats = _near_after_fan(ng)
    _check_coded(rt2mod, oraclemod, ("late-near", ng), tris, mats, W, H, variant,
                 f"a fan, then nearer and farther triangles, {ng} groups")


# ---- c. ties ---------------------------------------------------------------------

@gpu
@on_variants
@pytest.mark.parametrize("n", TIE_SIZES)
def test_ties(rt2mod, oraclemod, n, variant):
    tris, mats = _tie_scene(n)
    _check_coded(rt2mod, oraclemod, ("xw-ties", n), tris, mats, W, H, variant, f"ties, {n} triangles")


# ---- d. padding ------------------------------------------------------------------

PAD_SIZES = (1, 19, 32 * 38 - 13, 32 * 38, 32 * 39 - 13)


@gpu
@on_variants
@pytest.mark.parametrize("n", PAD_SIZES)
def test_padding(rt2mod, oraclemod, n, variant):
    tris, mats = _scene(("pad-fan", n), lambda: S.fan(n, S.FAN_SEED, "shuffled"))
    _check_coded(rt2mod, oraclemod, ("pad-fan", n), tris, mats, W, H, variant, f"fan of {n}")


# ---- e. half-block forms ---------------------------------------------------------

@gpu
@on_variants
@pytest.mark.parametrize("w,h", [(8, 3), (10, 4)])
def test_small_images(rt2mod, oraclemod, w, h, variant):
    tris, mats = S.coded_scene("soup", 1216)
    _check_coded(rt2mod, oraclemod, ("soup", 1216), tris, mats, w, h, variant, f"soup, {w}x{h}")


# ---- f. incoherent rays ----------------------------------------------------------

@gpu
@on_variants
@pytest.mark.parametrize("n", [1216, 1217])
def test_incoherent_rays(rt2mod, oraclemod, n, variant):
    _fits(rt2mod, variant, n)
    tris, mats = S.mixed_scene(n)
    u = rt2mod.offline_uniforms(W, H, 4, 4, n)
    ref, segs = _ref(oraclemod, ("mixed", n), tris, mats, u, "brute")
    img, gsegs, ran = _render(rt2mod, ("mixed", n), tris, mats, u, variant)
    _ran(rt2mod, ran, variant)
    _same_bits(img, ref, f"mixed soup of {n}, 4 rays, 4 bounces, variant {variant}")
    assert gsegs == segs > W * H * 4
