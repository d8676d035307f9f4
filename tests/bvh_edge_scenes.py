"""Hand-built BVHs whose image, per-ray result or leaf-test count reads out one
decision of the BVH walk (calculateRayCollisionBVH, compute.glsl:382-460).

Host half of tests/test_gpu_bvh_edges.py (needs the GPU); its premises are
checked on the CPU oracle alone by tests/test_bvh_edge_scenes.py.  Only numpy
here: triangle, material and node arrays (rt2.TRI_DTYPE, MAT_DTYPE, NODE_DTYPE).

rt2_scene_create checks only the shape of a node array and the oracle walks
whatever nodes it is given, so the boxes here need not bound their triangles:
a box that is wrongly visited or wrongly pruned then changes which triangle
wins (index-coded lights, closest_hit_scenes.py) or how many leaf tests a
segment makes.  The reference's corners these scenes sit on:
  * an axis with |d_i| < 1e-6 is skipped: the box's extent there is ignored,
    so a box the ray never enters is admitted;
  * a box flat on an unskipped axis (bmin == bmax) is always missed
    (tMin >= tMax);
  * tMax = -0.0 is not < 0: a box whose far face passes through the origin of
    the ray is admitted.

Every scene is built in one frame (camera at (0, 0, 10) looking down -z, the
triangles facing it around z = 5, the view there +-2 x +-2) and then rotated by
a cyclic permutation of the coordinates (`shift`: x -> y -> z -> x, which keeps
the triangles' winding), uniforms and query rays with it.
"""
from typing import NamedTuple

import numpy as np

import closest_hit_scenes as S
import rt2

F32 = np.float32
SKIP = F32(1e-6)            # rayBoundsIntersect's threshold, compute.glsl:388
CAM = (0.0, 0.0, 10.0)
PLANE_Z = 5.0
HALF = 0.4                  # viewportRight / viewportUp length for |front| = 1: +-2 at z = 5
JITTER = 4e-6               # pixelRight on a jitter-decided axis: |d_i| up to 2e-6
BIG = ((-40.0, -20.0), (40.0, -20.0), (0.0, 50.0))  # a footprint that covers the whole view

CHAIN_DEPTHS = (2, 3, 33, 61, 62)
MAX_DEPTH = 62              # the deepest tree rt2_scene_create accepts


class Scene(NamedTuple):
    name: str
    tris: np.ndarray        # as uploaded (rotated by shift)
    mats: np.ndarray
    nodes: np.ndarray
    shift: int
    canon_tris: np.ndarray  # the same in the building frame
    canon_nodes: np.ndarray
    targets: np.ndarray     # (k, 3) points on the triangles, building frame


def _roll(v, shift):
    return np.roll(np.asarray(v)[..., :3], shift, axis=-1)


def _finish(name, tris, nodes, shift=0, mats=None, targets=None):
    t, n = tris.copy(), nodes.copy()
    for k in "abc":
        t[k][:, :3] = _roll(tris[k], shift)
    n["bmin"], n["bmax"] = _roll(nodes["bmin"], shift), _roll(nodes["bmax"], shift)
    m = S.code_materials(len(tris)) if mats is None else mats
    if targets is None:
        targets = (tris["a"][:, :3] + tris["b"][:, :3] + tris["c"][:, :3]).astype(np.float64) / 3.0
    for a in (t, n, m, tris, nodes):
        a.setflags(write=False)
    return Scene(name, t, m, n, shift, tris, nodes, np.asarray(targets, np.float64))


def _frontal(pts, z):
    """Triangles facing +z: pts (n, 3, 2) the (x, y) of a, b, c (counter-clockwise), z scalar or (n,)."""
    pts = np.asarray(pts, np.float64).reshape(-1, 3, 2)
    zz = np.broadcast_to(np.asarray(z, np.float64), (len(pts),))
    v = [np.concatenate([pts[:, k], zz[:, None]], 1).astype(F32) for k in range(3)]
    return S._triangles(*v)


def tile_triangles(n, cols, rows, fill=0.8):
    """n small upright triangles in the plane z = 5, triangle i in cell i of a
    cols x rows grid over the view (row-major from the bottom left)."""
    assert n <= cols * rows
    i = np.arange(n)
    cw, ch = 4.0 / cols, 4.0 / rows
    cx, cy = -2.0 + (i % cols + 0.5) * cw, -2.0 + (i // cols + 0.5) * ch
    hw, hh = 0.5 * fill * cw, 0.5 * fill * ch
    pts = np.stack([np.stack([cx - hw, cy - hh], 1), np.stack([cx + hw, cy - hh], 1), np.stack([cx, cy + hh], 1)], 1)
    return _frontal(pts, PLANE_Z)


def _node_array(n):
    nodes = np.zeros(n, dtype=rt2.NODE_DTYPE)
    nodes["childIndex"] = -1
    return nodes


def _set(nodes, i, lo, hi, tri_index=0, tri_count=0, child=-1):
    nodes["bmin"][i], nodes["bmax"][i] = lo, hi
    nodes["triangleIndex"][i], nodes["triangleCount"][i], nodes["childIndex"][i] = tri_index, tri_count, child


def uniforms(width, height, n_tris, skip="none", axes="x", shift=0, cam=CAM, bounces=1, basic=False,
             half=(HALF, HALF)):
    """Every rt2.Uniforms field by hand: a pinhole camera at `cam` looking down
    -z with |front| = 1 (no defocus), environment light off, 1 ray per pixel.
    skip = "none": ordinary viewport vectors (no lane skips an axis, but for the
    centre column or row of a preview).  "jitter": on each axis of `axes` ("x":
    right, "y": up) the viewport vector is 0 and the pixel vector 4e-6, so the
    pixel jitter alone decides |d_axis| < 1e-6 lane by lane.  "zero": viewport
    and pixel vector both 0 there: d_axis is exactly +-0 in every lane.  All
    vectors are rotated by `shift` like the scene."""
    assert skip in ("none", "jitter", "zero") and set(axes) <= set("xy")
    right = np.array([half[0], 0.0, 0.0])
    up = np.array([0.0, half[1], 0.0])
    pr, pu = right * 2.0 / width, up * 2.0 / height
    if skip != "none":
        if "x" in axes:
            right, pr = right * 0.0, np.array([JITTER if skip == "jitter" else 0.0, 0.0, 0.0])
        if "y" in axes:
            up, pu = up * 0.0, np.array([0.0, JITTER if skip == "jitter" else 0.0, 0.0])
    u = rt2.Uniforms()
    u.pad, u.numTextures, u.width, u.height = 0, 0, width, height
    u.numSpheres, u.numTriangles = 0, n_tris
    u.basicShading, u.basicShadingShadow = int(basic), 0
    u.environmentalLight, u.maxBounceCount, u.numRaysPerPixel, u.frameIndex = 0, bounces, 1, 0

    def put(v4, v):
        v4.x, v4.y, v4.z, v4.w = (*(float(c) for c in _roll(np.asarray(v, np.float64), shift)), 0.0)

    put(u.basicShadingLightPosition, (0.0, 0.0, 0.0))
    put(u.cameraPos, cam)
    put(u.viewportFront, (0.0, 0.0, -1.0))
    put(u.viewportRight, right)
    put(u.viewportUp, up)
    put(u.pixelRight, pr)
    put(u.pixelUp, pu)
    put(u.defocusDiskRight, (0.0, 0.0, 0.0))
    put(u.defocusDiskUp, (0.0, 0.0, 0.0))
    return u


# ---- chain ---------------------------------------------------------------------

def chain(depth, near="interior", leaf_slot=0):
    """A chain of `depth` levels: every interior node has one leaf child and one
    interior child (the last one two leaves), the leaf in child slot leaf_slot.
    All boxes are (-3, -3, 4) .. (3, 3, front) and overlap; the front face (6.5
    against 6) makes the interior child ("interior") or the leaf ("leaf") the
    near one for every ray.  Leaf k holds triangle k alone, in cell k of an
    8 x 8 grid: every box is entered before any triangle is reached (4 / |d.z|
    against 5 / |d.z|), so every segment tests all `depth` leaves, and with the
    interior child near the reference's stack holds every leaf of the chain at
    once before the first is tested."""
    assert depth >= 2 and near in ("interior", "leaf") and leaf_slot in (0, 1)
    tris = tile_triangles(depth, 8, 8)
    nodes = _node_array(2 * depth - 1)
    lo = (-3.0, -3.0, 4.0)
    near_z, far_z = 6.5, 6.0
    _set(nodes, 0, lo, (3.0, 3.0, 7.0), child=1)
    at = 0
    for k in range(depth - 1):
        c = 2 * k + 1
        nodes["childIndex"][at] = c
        if k == depth - 2:
            _set(nodes, c, lo, (3.0, 3.0, near_z if leaf_slot == 0 else far_z), k, 1)
            _set(nodes, c + 1, lo, (3.0, 3.0, far_z if leaf_slot == 0 else near_z), k + 1, 1)
        else:
            li, ii = (c, c + 1) if leaf_slot == 0 else (c + 1, c)
            _set(nodes, li, lo, (3.0, 3.0, far_z if near == "interior" else near_z), k, 1)
            _set(nodes, ii, lo, (3.0, 3.0, near_z if near == "interior" else far_z), child=0)
            at = ii
    return _finish(f"chain{depth}-{near}-{leaf_slot}", tris, nodes)


# ---- displaced -------------------------------------------------------------------

def _view_targets(z_values, k=5):
    g = np.linspace(-1.7, 1.7, k)
    return np.array([(x, y, z) for z in z_values for y in g for x in g])


def displaced(axes):
    """Two leaves: triangle 0 (z = 5) in front of triangle 1 (z = 4), both over
    the whole view.  Leaf 1's box holds triangle 1; leaf 0's box is displaced to
    100..101 on the axis (for "xy": on both), far from triangle 0 and from every
    ray: only a ray that skips the axis (both axes) is admitted, tests triangle
    0 and hits it.  axes: "x", "y", "z" (the x scene rotated) or "xy"."""
    assert axes in ("x", "y", "z", "xy")
    tris = _frontal([BIG, BIG], [PLANE_Z, PLANE_Z - 1.0])
    nodes = _node_array(3)
    _set(nodes, 0, (-50.0, -50.0, 3.0), (101.0, 101.0, 6.0), child=1)
    y = (100.0, 101.0) if axes == "xy" else (-50.0, 60.0)
    _set(nodes, 1, (100.0, y[0], 4.5), (101.0, y[1], 5.5), 0, 1)
    _set(nodes, 2, (-50.0, -50.0, 3.5), (50.0, 60.0, 4.5), 1, 1)
    shift = {"x": 0, "y": 1, "z": 2, "xy": 0}[axes]
    return _finish(f"displaced-{axes}", tris, nodes, shift, targets=_view_targets((PLANE_Z, PLANE_Z - 1.0)))


def skip_axes(axes):
    """The uniforms' `axes` of a displaced / flat scene (the rotation carries x to y or z)."""
    return "xy" if axes == "xy" else "x"


# ---- flat --------------------------------------------------------------------------

def flat(axis):
    """Four leaves under two interior nodes.  Leaf 0: a hand-set box flat on x
    (x = 0..0) around triangle 0, which covers the view at z = 5.5: admitted
    only by a ray that skips x.  Leaf 1: the tight box of triangle 1, which
    lies in the plane z = 5 (left half of the view): flat on z, missed by every
    ray that does not skip z.  Leaves 2 and 3: ordinary boxes around triangle 2
    (z = 4.5, upper half) and triangle 3 (z = 4, whole view).  axis "y" / "z":
    the scene rotated."""
    assert axis in ("x", "y", "z")
    left = ((0.0, -6.0), (0.0, 6.0), (-12.0, 0.0))
    upper = ((-12.0, 0.0), (12.0, 0.0), (0.0, 12.0))
    tris = _frontal([BIG, left, upper, BIG], [5.5, 5.0, 4.5, 4.0])
    nodes = _node_array(7)
    _set(nodes, 0, (-50.0, -50.0, 3.0), (50.0, 60.0, 7.0), child=1)
    _set(nodes, 1, (-50.0, -50.0, 4.75), (50.0, 60.0, 7.0), child=3)
    _set(nodes, 2, (-50.0, -50.0, 3.0), (50.0, 60.0, 4.75), child=5)
    _set(nodes, 3, (0.0, -50.0, 5.0), (0.0, 60.0, 6.0), 0, 1)
    _set(nodes, 4, (-12.0, -6.0, 5.0), (0.0, 6.0, 5.0), 1, 1)
    _set(nodes, 5, (-12.0, 0.0, 4.25), (12.0, 12.0, 4.75), 2, 1)
    _set(nodes, 6, (-50.0, -50.0, 3.5), (50.0, 60.0, 4.5), 3, 1)
    shift = {"x": 0, "y": 1, "z": 2}[axis]
    return _finish(f"flat-{axis}", tris, nodes, shift, targets=_view_targets((5.5, 5.0, 4.5, 4.0), 4))


# ---- eight leaves under a balanced tree ------------------------------------------------

def _balanced8(leaves, interior_hi=(4.0, 4.0, 7.0)):
    """Nodes 0..6 interior (0 -> 1, 2; 1 -> 3, 4; 2 -> 5, 6; 3..6 -> the leaf
    pairs 7.. 14), each with the box (-4, -4, 3) .. interior_hi; leaves: (lo,
    hi, triangleIndex, triangleCount)."""
    assert len(leaves) == 8
    nodes = _node_array(15)
    for i in range(7):
        _set(nodes, i, (-4.0, -4.0, 3.0), interior_hi, child=2 * i + 1)
    for k, (lo, hi, ti, tc) in enumerate(leaves):
        _set(nodes, 7 + k, lo, hi, ti, tc)
    return nodes


TOUCHING_BANDS = (0, 1, 2, 4, 3, 5, 6, 6)  # leaf -> band of its triangle (band 4 straddles y = 0)


def touching():
    """Eight leaves, triangle k in leaf k: a wide triangle in the plane z = 5 in
    its own horizontal band of the view (triangles 6 and 7 coincide).  The
    camera stands at (0, 0, 10), so the numerators of the faces through it are
    exactly 0 and t = +-0:
      0  a face at the camera (z up to 10): admitted, tMin = -0;
      1  the far face at the camera (z from 10 to 12): tMax = -0, not < 0: admitted;
      2  an edge through the camera (x from 0, z up to 10): admitted by d.x > 0
         only (or by a ray that skips x);
      3  a corner at the camera (x from 0, y from 0, z up to 10): d.x > 0 and d.y > 0;
      4  wholly behind the camera (z 11..12, tMax < 0): never admitted;
      5  beside the view (x -3..-1): admitted where the ray reaches it inside the z slab;
      6, 7  identical boxes, identical triangles: dA < dB is false, so the
            second child is the near one and triangle 7 keeps every tie.
    Interior node 1's box ends at the camera plane too (z up to 10)."""
    band_y = -2.25 + 0.5 * np.asarray(TOUCHING_BANDS)
    pts = [((-2.4, y + 0.04), (2.4, y + 0.04), (0.0, y + 0.46)) for y in band_y]
    tris = _frontal(pts, PLANE_Z)
    lo, hi = (-3.0, -3.0, 4.0), (3.0, 3.0, 6.0)
    leaves = [(lo, (3.0, 3.0, 10.0), 0, 1),
              ((-3.0, -3.0, 10.0), (3.0, 3.0, 12.0), 1, 1),
              ((0.0, -3.0, 4.0), (3.0, 3.0, 10.0), 2, 1),
              ((0.0, 0.0, 4.0), (3.0, 3.0, 10.0), 3, 1),
              ((-3.0, -3.0, 11.0), (3.0, 3.0, 12.0), 4, 1),
              ((-3.0, -3.0, 4.0), (-1.0, 3.0, 6.0), 5, 1),
              (lo, hi, 6, 1),
              (lo, hi, 7, 1)]
    nodes = _balanced8(leaves)
    nodes["bmax"][1] = (4.0, 4.0, 10.0)
    return _finish("touching", tris, nodes)


LEAF_COUNTS = (0, 1, 30, 31, 32, 33, -1, 0)


def leaf_sizes():
    """Eight leaves of 0, 1, 30, 31, 32 and 33 triangles (bvh_records packs up
    to 30 into the stack entry and sends larger leaves through the node array),
    one with triangleCount = -1 and one empty leaf whose range starts at the
    array's end; 127 triangles, triangle i in cell i of a 16 x 8 grid.  All
    boxes overlap and are entered before any triangle; the empty leaf 0 is the
    near child of its pair (front face 6.5 against 6)."""
    n = sum(c for c in LEAF_COUNTS if c > 0)
    tris = tile_triangles(n, 16, 8)
    lo = (-3.0, -3.0, 4.0)
    leaves, at = [], 0
    for k, c in enumerate(LEAF_COUNTS):
        hi = (3.0, 3.0, 6.5 if k == 0 else 6.0)
        if c == -1:
            leaves.append((lo, hi, 5, -1))
        else:
            leaves.append((lo, hi, at, c))
            at += c
    assert at == n == 127 and leaves[7][2] == n
    return _finish("leaf_sizes", tris, _balanced8(leaves))


def root_leaf():
    """The smallest tree: node 0 is a leaf of three triangles (no child-pair
    record at all; the walk starts at a leaf, whose box is never looked at)."""
    nodes = _node_array(1)
    _set(nodes, 0, (100.0, 100.0, 100.0), (101.0, 101.0, 101.0), 0, 3)
    return _finish("root_leaf", tile_triangles(3, 8, 8), nodes)


# ---- slab-path switch ----------------------------------------------------------------

SLAB_N = 257
SLAB_SIZE = (64, 36)
SLAB_HALF = (0.46, 0.256)       # the soups' view: +-2.3 x +-1.28 at z = 5 from (0, 5, 10)
SLAB_FRAMES = (3, 2)            # first frame, frames


def slab_switch(which):
    """The mixed soup (diffuse, mirrors, a light every 8th triangle) of 257
    triangles on its build_bvh tree, for 6 bounces and 2 frames.  Returns
    (scene, uniforms).
      "a"  a camera component of 2^-40: primary rays fail render_bvh4's
           mk_coord_ok (not 0 and below 2^-37), scattered rays from surface
           points pass it, and a wave's lanes are at different bounces: both
           kinds in one wave, which must then take the IEEE slab;
      "b"  one box coordinate of 1e-30 and one of 2^60: recs_ok = 0, every wave
           takes the IEEE slab;
      "c"  as "a" with the jitter-decided skip on x for the primary rays."""
    assert which in ("a", "b", "c")
    t, m = S.mixed_scene(SLAB_N)
    sd = S.scene_data(t, m)
    tris, mats, nodes = sd.triangles().copy(), sd.materials().copy(), sd.nodes().copy()
    cam = (2.0 ** -40, 5.0, 10.0)
    if which == "b":
        cam = (0.0, 5.0, 10.0)
        nodes["bmax"][1, 0] = 2.0 ** 60
        nodes["bmin"][2, 1] = 1e-30
    w, h = SLAB_SIZE
    u = uniforms(w, h, len(tris), "jitter" if which == "c" else "none", "x", cam=cam, bounces=6, half=SLAB_HALF)
    return _finish(f"slab_switch-{which}", tris, nodes, mats=mats), u


# ---- query rays ----------------------------------------------------------------------------

ORDINARY, THRESHOLD, TINY, LONG, BOX_ORIGIN, EXTREME_ORIGIN, NONFINITE_BLOCK = range(7)
CLASS_NAMES = ("ordinary", "threshold", "tiny", "long", "box_origin", "extreme_origin", "nonfinite_block")
_CYCLE = (THRESHOLD, BOX_ORIGIN, TINY, THRESHOLD, EXTREME_ORIGIN, LONG, ORDINARY)
BLOCK = (64, 128)               # the rays of the non-finite block
NAN_RAY, INF_RAY = 64 + 41, 64 + 50
RAY_COUNTS = (193, 257)

_up, _dn = np.nextafter(SKIP, F32(1)), np.nextafter(SKIP, F32(0))
THRESHOLD_VALUES = np.array([0.0, -0.0, SKIP, -SKIP, _up, -_up, _dn, -_dn, F32(9.99e-7), -F32(9.99e-7)], F32)
TINY_DIRECTIONS = np.array([(3e-7, -2e-7, -9e-7), (-9e-7, 9.9e-7, -5e-7), (0.0, 0.0, 0.0), (-0.0, 0.0, -0.0),
                            (1e-7, 1e-7, 9e-7), (-9.99e-7, -9.99e-7, -9.99e-7)], F32)
EXTREME_VALUES = np.array([2.0 ** -40, 2.0 ** 60, 1e-40, -(2.0 ** -40)], F32)  # 1e-40: a binary32 subnormal


def _unit(v):
    n = np.linalg.norm(v)
    return v / n if n > 0 else np.array([0.0, 0.0, -1.0])


def query_rays(scene, n, seed=11):
    """(origins, directions, class) of n rays for `scene`, float32.  Rays 64..127
    are the non-finite block: ordinary rays with a NaN origin component in ray
    105 and an infinite direction component in ray 114.  The others take the
    classes of _CYCLE by turns:
      threshold       one direction component (x, y, z by turns) set to +0, -0,
                      +-1e-6f, its two float32 neighbours, +-9.99e-7, the ray
                      otherwise aimed at a triangle;
      tiny            all three components below 1e-6 (aimed so that the far
                      hit lands on a triangle), d = 0, d = (-0, 0, -0);
      long            an ordinary direction times 3;
      box_origin      origins at corners, on edges and on faces of the nodes'
                      boxes (bmin / bmax coordinates as they are);
      extreme_origin  an origin component of 2^-40, 2^60 or a subnormal;
      ordinary        from around the camera toward a triangle or just beside
                      it, every fifth past all of them.
    The special components are float32 values assigned after every other
    computation: they reach the kernel bit for bit."""
    rng = np.random.default_rng(seed)
    tg, nodes = scene.targets, scene.canon_nodes
    o = np.zeros((n, 3), F32)
    d = np.zeros((n, 3), F32)
    cls = np.zeros(n, np.int32)
    count = [0] * len(CLASS_NAMES)

    def ordinary(k):
        org = np.asarray(CAM) + np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), 0.0])
        t = tg[k % len(tg)] + np.array([rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), 0.0])
        if k % 5 == 4:  # past every triangle
            t = np.array([60.0, -45.0, t[2]])
        org = org.astype(F32)
        return org, _unit(t - org.astype(np.float64)).astype(F32)

    j = 0
    for i in range(n):
        if BLOCK[0] <= i < BLOCK[1]:
            c = NONFINITE_BLOCK
        else:
            c = _CYCLE[j % len(_CYCLE)]
            j += 1
        k = count[c]
        count[c] += 1
        cls[i] = c
        t = tg[(k * 7 + c) % len(tg)]
        if c in (ORDINARY, NONFINITE_BLOCK):
            o[i], d[i] = ordinary(k)
        elif c == LONG:
            oo, dd = ordinary(k)
            o[i], d[i] = oo, dd * F32(3)
        elif c == THRESHOLD:
            axis, v = k % 3, THRESHOLD_VALUES[(k // 3) % len(THRESHOLD_VALUES)]
            if axis < 2:  # straight above the target on that axis
                org = np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), CAM[2]])
                org[axis] = t[axis]
            else:  # along x in the target's own z plane
                org = np.array([t[0] - 3.0, t[1], t[2]])
            org = org.astype(F32)
            dd = t - org.astype(np.float64)
            dd[axis] = 0.0
            o[i], d[i] = org, _unit(dd).astype(F32)
            d[i, axis] = v
        elif c == TINY:
            dd = TINY_DIRECTIONS[k % len(TINY_DIRECTIONS)]
            org = np.array([t[0], t[1], CAM[2]])
            if dd[2] < 0:  # back along the direction from the target
                s = (CAM[2] - t[2]) / -np.float64(dd[2])
                org = t - dd.astype(np.float64) * s
            o[i], d[i] = org.astype(F32), dd
        elif c == BOX_ORIGIN:
            nd = nodes[(k * 11) % len(nodes)]
            lo, hi = nd["bmin"].astype(np.float64), nd["bmax"].astype(np.float64)
            kind, bits = k % 3, k * 5 + 3  # corner, edge, face by turns
            org = np.where([(bits >> a) & 1 for a in range(3)], hi, lo)
            mid = 0.5 * (lo + hi)
            if kind >= 1:  # an edge: one coordinate between the bounds
                org[k % 3] = mid[k % 3]
            if kind == 2:  # a face: two
                org[(k + 1) % 3] = mid[(k + 1) % 3]
            org = org.astype(F32)
            o[i], d[i] = org, _unit(t - org.astype(np.float64)).astype(F32)
        else:  # EXTREME_ORIGIN
            v, axis = EXTREME_VALUES[k % len(EXTREME_VALUES)], (k // len(EXTREME_VALUES)) % 2
            org = np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), CAM[2]])
            org[axis] = 0.0
            t = tg[np.argmin(np.abs(tg[:, axis]) + 1e-3 * ((np.arange(len(tg)) * 7 + k) % len(tg)))]
            o[i], d[i] = org.astype(F32), _unit(t - org).astype(F32)
            o[i, axis] = v
    if n > NAN_RAY:
        o[NAN_RAY, 0] = np.nan
    if n > INF_RAY:
        d[INF_RAY, 1] = np.inf
    o, d = np.ascontiguousarray(_roll(o, scene.shift)), np.ascontiguousarray(_roll(d, scene.shift))
    for a in (o, d, cls):
        a.setflags(write=False)
    return o, d, cls


def ray_bounds32(o, d, bmin, bmax):
    """rayBoundsIntersect (compute.glsl:382-408) in numpy float32: the entry
    distance, 1e38 for a miss."""
    o, d, bmin, bmax = (np.asarray(v, F32) for v in (o, d, bmin, bmax))
    t_min, t_max = F32(-1e32), F32(1e32)
    with np.errstate(all="ignore"):
        for i in range(3):
            if not (d[i] < SKIP and d[i] > -SKIP):
                t0, t1 = (bmin[i] - o[i]) / d[i], (bmax[i] - o[i]) / d[i]
                if t0 > t1:
                    t0, t1 = t1, t0
                if t_min < t0:
                    t_min = t0
                if t_max > t1:
                    t_max = t1
                if t_min >= t_max or t_max < F32(0):
                    return F32(1e38)
    return t_min


def walk(oraclemod, tris, nodes, o, d, bound=1e38):
    """The reference's walk (compute.glsl:410-460) restated in Python on one
    ray, with float32 box distances and the oracle's own triangle test.
    Returns (dst, tri, leaf tests, interior visits, the stack's highest fill,
    the node index of the leaf that gave the hit or -1)."""
    import ctypes as C
    f = oraclemod.lib().oracle_ray_triangle
    tris = np.ascontiguousarray(tris)
    o, d = np.ascontiguousarray(o, F32), np.ascontiguousarray(d, F32)
    out = C.c_float()
    best, bi, tests, visits, leaf = F32(bound), -1, 0, 0, -1
    stack, high = [0], 1
    while stack:
        ni = stack.pop()
        nd = nodes[ni]
        if nd["childIndex"] == -1:
            for t in range(int(nd["triangleIndex"]), int(nd["triangleIndex"]) + int(nd["triangleCount"])):
                tests += 1
                if f(o.ctypes.data, d.ctypes.data, tris.ctypes.data + 80 * t, C.addressof(out)) and \
                        F32(out.value) < best:
                    best, bi, leaf = F32(out.value), t, ni
        else:
            visits += 1
            ia, ib = int(nd["childIndex"]), int(nd["childIndex"]) + 1
            da = ray_bounds32(o, d, nodes["bmin"][ia], nodes["bmax"][ia])
            db = ray_bounds32(o, d, nodes["bmin"][ib], nodes["bmax"][ib])
            near_a = da < db
            d_near, d_far = (da, db) if near_a else (db, da)
            i_near, i_far = (ia, ib) if near_a else (ib, ia)
            if d_far < best and len(stack) < 64:
                stack.append(i_far)
            if d_near < best and len(stack) < 64:
                stack.append(i_near)
            high = max(high, len(stack))
    return best, bi, tests, visits, high, leaf


def leaf_of_triangle(nodes):
    """Triangle index -> the leaf whose range holds it (the first such leaf), -1 where none does."""
    n = int(max((nd["triangleIndex"] + nd["triangleCount"] for nd in nodes if nd["childIndex"] == -1), default=0))
    out = np.full(max(n, 1), -1, np.int64)
    for i, nd in enumerate(nodes):
        if nd["childIndex"] == -1 and nd["triangleCount"] > 0:
            r = slice(int(nd["triangleIndex"]), int(nd["triangleIndex"] + nd["triangleCount"]))
            out[r] = np.where(out[r] < 0, i, out[r])
    return out


def bounded_tmax(scene, o, d, dst, tri):
    """One bound per ray from its unbounded result, by turns (ray index mod 4):
    none; one ulp above the hit distance (the same hit); half the hit distance
    (a miss); the float32 entry distance of the hit leaf's own box, where that
    is positive (`dstChild < dst` is strict: the leaf is not pushed, its
    triangle cannot be the hit).  A ray that misses has no bound."""
    leaf = leaf_of_triangle(scene.nodes)
    tmax = np.zeros(len(o), F32)
    for i in np.flatnonzero(np.asarray(tri) >= 0):
        k = i % 4
        if k == 1:
            tmax[i] = np.nextafter(dst[i], F32(np.inf))
        elif k == 2:
            tmax[i] = dst[i] * F32(0.5)
        elif k == 3:
            nd = scene.nodes[leaf[tri[i]]]
            e = ray_bounds32(o[i], d[i], nd["bmin"], nd["bmax"])
            tmax[i] = e if 0 < e < F32(1e38) else F32(0)
    return tmax


# ---- the scenes of the tests, built once ------------------------------------------------

_built = {}


def get(kind, *args):
    """chain / displaced / flat / touching / leaf_sizes scenes, built once and read-only."""
    if (kind, args) not in _built:
        _built[(kind, args)] = {"chain": chain, "displaced": displaced, "flat": flat, "touching": touching,
                                "leaf_sizes": leaf_sizes, "root_leaf": root_leaf}[kind](*args)
    return _built[(kind, args)]


def render_cases():
    """(id, scene, uniforms, first frame, frames) of every render the GPU tests
    compare with the oracle; images of at most 64 x 64."""
    cases = []
    for depth in CHAIN_DEPTHS:
        for near in ("interior", "leaf"):
            for slot in (0, 1):
                sc = get("chain", depth, near, slot)
                cases.append((sc.name, sc, uniforms(64, 64, len(sc.tris)), 0, 1))
    for axes in ("x", "y", "z", "xy"):
        sc = get("displaced", axes)
        for skip in ("jitter", "zero", "none"):
            cases.append((f"{sc.name}-{skip}", sc, uniforms(64, 16, 2, skip, skip_axes(axes), sc.shift), 0, 1))
    for axis in ("x", "y", "z"):
        sc = get("flat", axis)
        for skip in ("jitter", "none"):
            cases.append((f"{sc.name}-{skip}", sc, uniforms(64, 16, 4, skip, "x", sc.shift), 0, 1))
    sc = get("touching")
    cases.append((sc.name, sc, uniforms(64, 64, len(sc.tris)), 0, 1))
    cases.append((sc.name + "-jitter", sc, uniforms(64, 64, len(sc.tris), "jitter", "x"), 0, 1))
    for kind in ("leaf_sizes", "root_leaf"):
        sc = get(kind)
        cases.append((sc.name, sc, uniforms(64, 64, len(sc.tris)), 0, 1))
    for which in "abc":
        if ("slab", which) not in _built:
            _built[("slab", which)] = slab_switch(which)
        sc, u = _built[("slab", which)]
        cases.append((sc.name, sc, u, *SLAB_FRAMES))
    return cases


def query_scenes():
    return [get("displaced", "x"), get("displaced", "xy"), get("flat", "x"), get("flat", "z"), get("touching"),
            get("chain", MAX_DEPTH, "interior", 0), get("leaf_sizes")]
