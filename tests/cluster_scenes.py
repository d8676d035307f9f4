"""Hand-built scenes and tables for the compact-cluster tests
(tests/test_cluster_need.py on the CPU, tests/test_gpu_cluster_rows.py on the
GPU).  Only numpy and the rt2 package's host half.

The strips scene, seen by the default camera (at (0, 5, 10), looking down -z;
at z = 5 a 16:9 view spans x in +-2.3 and y in 5 +- 1.28): parts in index
order, each a whole number of 32-triangle groups except the last:

    part      groups  what                                         table
    one       1       strip over 1 of 64 pixel columns, band 0     compact (first)
    wall      2       large triangles behind and below everything  full
    half      2       strip over 32 columns, band 1, planar z = 5  compact (flat box)
    half1     3       strip over 33 columns, band 2                compact
    all       1       strip over all 64 columns, band 3            compact
    none      2       a blob behind the camera (no primary ray)    compact
    most      1.x     strip over 31 columns, band 4; ragged group  compact (last)

so a wave of 64 adjacent pixels of one image row meets a cluster that 0, 1,
about 31 / 32 / 33 (the pixel jitter moves the edge columns) and 64 of its
primary rays need, clusters of 1, 2 and 3 groups, a compact cluster first,
last and next to a full one, a flat box and a ragged last group.  Two exact
distance ties cross the compact / full border, one won by each side."""
import numpy as np

import rt2
from closest_hit_scenes import VIEW_X, VIEW_Y, CAMERA, CHAMP_Z, _triangles, mixed_materials, with_ties

PARTS = (("one", 32, True), ("wall", 64, False), ("half", 64, True), ("half1", 96, True), ("all", 32, True),
         ("none", 64, True), ("most", 37, True))
BANDS = 5


def _wind(a, b, c):
    nz = (b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0])
    flip = nz < 0  # n.z > 0: facing the camera
    b[flip], c[flip] = c[flip].copy(), b[flip].copy()
    return a, b, c


def _strip(rng, n, cols, band, flat):
    """n small triangles over the first `cols` pixel columns of a 64-column 16:9 image, in band `band`."""
    x0, x1 = -VIEW_X, -VIEW_X + 2 * VIEW_X * cols / 64
    y0 = CAMERA[1] - VIEW_Y + 2 * VIEW_Y * band / BANDS
    y1 = y0 + 2 * VIEW_Y / BANDS
    lo, hi = np.array([x0, y0, CHAMP_Z - 0.2]), np.array([x1, y1, CHAMP_Z + 0.2])
    if flat:
        lo[2] = hi[2] = CHAMP_Z
    size = (hi - lo) * np.array([0.5 if cols == 1 else 0.15, 0.5, 1.0])
    ctr = rng.uniform(lo, hi - size, (n, 3))
    a, b, c = ctr, ctr + rng.uniform(0, 1, (n, 3)) * size, ctr + rng.uniform(0, 1, (n, 3)) * size
    # two triangles reach the strip's corners, so its box is the strip
    a[0], b[0], c[0] = lo, (hi[0], lo[1], lo[2]), (lo[0], hi[1], hi[2])
    a[1], b[1], c[1] = hi, (lo[0], hi[1], hi[2]), (hi[0], lo[1], lo[2])
    return _wind(*(v.astype(np.float32) for v in (a, b, c)))


def _wall(rng, n):
    """n large triangles: a back wall at z = -4 and a floor at y = 2, each covered several times over."""
    a, b, c = (np.zeros((n, 3), np.float32) for _ in range(3))
    for i in range(n):
        s = rng.uniform(-1.0, 1.0, 2)
        if i % 2 == 0:  # back wall, facing +z
            a[i], b[i], c[i] = (-9 + s[0], 0 + s[1], -4), (9 + s[0], 0 + s[1], -4), (s[0], 12 + s[1], -4)
        else:  # floor, facing +y
            a[i], b[i], c[i] = (-9 + s[0], 2, 9 + s[1]), (9 + s[0], 2, 9 + s[1]), (s[0], 2, -9 + s[1])
    return a, b, c


def _blob(rng, n, lo, hi, size):
    ctr = rng.uniform(lo, hi, (n, 3))
    a = ctr
    b = np.clip(ctr + rng.uniform(-size, size, (n, 3)), lo, hi)
    c = np.clip(ctr + rng.uniform(-size, size, (n, 3)), lo, hi)
    return tuple(v.astype(np.float32) for v in (a, b, c))


_cache = {}


def strips_scene():
    """(triangles, materials, ranges): ranges = [(first group, end group, compact)] of the parts."""
    if "strips" in _cache:
        return _cache["strips"]
    rng = np.random.default_rng(20)
    geo = {"one": _strip(rng, 32, 1, 0, False), "wall": _wall(rng, 64), "half": _strip(rng, 64, 32, 1, True),
           "half1": _strip(rng, 96, 33, 2, False), "all": _strip(rng, 32, 64, 3, False),
           "none": _blob(rng, 64, np.array([-1.0, 4.0, 12.0]), np.array([1.0, 6.0, 13.0]), 0.3),
           "most": _strip(rng, 37, 31, 4, False)}
    a, b, c = (np.concatenate([geo[name][k] for name, _, _ in PARTS]) for k in range(3))
    tris = _triangles(a, b, c)
    n = len(tris)
    # ties across the compact / full border: wall triangle 40 becomes a copy of `half`'s triangle 100 (the full
    # cluster's lower index wins), wall triangle 41 a copy of `one`'s triangle 5 (the compact cluster's wins)
    tris = with_ties(tris, [[100, 40], [5, 41]])
    mats = mixed_materials(n)
    ranges, g = [], 0
    for _, cnt, compact in PARTS:
        g1 = g + (cnt + 31) // 32
        ranges.append((g, g1, compact))
        g = g1
    assert g == (n + 31) // 32 and n % 32 != 0
    _cache["strips"] = (tris, mats, ranges)
    return _cache["strips"]


def group_boxes(tris):
    """(lo, hi) float64 [groups, 3] of the vertices of every 32-triangle group."""
    v = np.stack([tris["a"][:, :3], tris["b"][:, :3], tris["c"][:, :3]], 1).astype(np.float64)  # [n, 3 vertices, 3]
    ng = (len(tris) + 31) // 32
    lo = np.stack([v[32 * g:32 * g + 32].min((0, 1)) for g in range(ng)])
    hi = np.stack([v[32 * g:32 * g + 32].max((0, 1)) for g in range(ng)])
    return lo, hi


def explicit_table(tris, ranges, pad=None, far_o=None):
    """A CLUSTER_TABLE_DTYPE record with the given ranges, every box the
    vertices' box padded like the library's (its pad_abs and far_o, taken from
    the library's own table of the same triangles, unless given)."""
    own = rt2.cluster_table(tris)
    pad = np.float32(own["pad_abs"] if pad is None else pad)
    t = np.zeros(1, dtype=rt2.CLUSTER_TABLE_DTYPE)[0]
    t["far_o"] = own["far_o"] if far_o is None else far_o
    t["pad_abs"] = pad
    t["n"] = len(ranges)
    glo, ghi = group_boxes(tris)
    for k, (g0, g1, compact) in enumerate(ranges):
        t["c"][k]["g0"] = g0
        t["c"][k]["g1_flags"] = g1 | (rt2.CLUSTER_COMPACT if compact else 0)
        t["c"][k]["lo"] = glo[g0:g1].min(0).astype(np.float32) - pad
        t["c"][k]["hi"] = ghi[g0:g1].max(0).astype(np.float32) + pad
    return t


def check_table(t, tris):
    """The invariants of a table: contiguous ranges that cover the groups, at
    most MAX_CLUSTERS of them, every vertex inside its compact cluster's box
    with room to spare.  n = 0 (no compact cluster) has nothing to check."""
    n = int(t["n"])
    assert 0 <= n <= rt2.MAX_CLUSTERS
    if n == 0:
        return
    ng = (len(tris) + 31) // 32
    glo, ghi = group_boxes(tris)
    g = 0
    compact = 0
    for c in t["c"][:n]:
        g0, g1 = int(c["g0"]), int(c["g1_flags"]) & 0xffff
        assert g0 == g and g1 > g0
        assert int(c["g1_flags"]) & ~(0xffff | rt2.CLUSTER_COMPACT) == 0
        if int(c["g1_flags"]) & rt2.CLUSTER_COMPACT:
            compact += 1
            assert np.all(c["lo"].astype(np.float64) < glo[g0:g1].min(0))
            assert np.all(c["hi"].astype(np.float64) > ghi[g0:g1].max(0))
        g = g1
    assert g == ng
    assert compact >= 1, "a table without a compact cluster is the empty table"
    assert t["pad_abs"] > 0 and t["far_o"] > 0


def cluster_of_triangle(t, idx):
    """For triangle indices idx (>= 0): the cluster each lies in."""
    g = np.asarray(idx) >> 5
    ends = np.array([int(c["g1_flags"]) & 0xffff for c in t["c"][:int(t["n"])]])
    return np.searchsorted(ends, g, side="right")


def compact_mask(t):
    m = 0
    for k, c in enumerate(t["c"][:int(t["n"])]):
        if int(c["g1_flags"]) & rt2.CLUSTER_COMPACT:
            m |= 1 << k
    return m
