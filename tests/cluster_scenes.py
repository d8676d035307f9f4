"""Hand-built scenes and tables for the compact-cluster tests
(tests/test_cluster_need.py on the CPU, tests/test_gpu_cluster_rows.py and
tests/test_gpu_cluster_private.py on the GPU).  Only numpy and the rt2
package's host half.  The strips scene first; the comb scenes, whose triangles
each belong to one ray, and the row model of cluster_rows_frag further down.

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
from closest_hit_scenes import (VIEW_X, VIEW_Y, CAMERA, CHAMP_Z, _triangles, code_materials, mixed_materials,
                                with_ties)

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


# ------------------------------------------------------------- comb scenes
#
# Scenes in which a ray that was wrongly left out of a compact cluster's sweep
# cannot be rescued by its neighbours (tests/test_gpu_cluster_private.py).
# The camera sits at the origin and looks down -z through a 64-column viewport
# that is tilted a little (COMB_FRONT), so that no primary ray has a zero
# direction component (such a ray needs every cluster).  Pixel jitter and
# defocus are zero: the ray of pixel (x, y) has the direction
# (fx + hx px, fy + hy py, -1), px = (2 x - 64) / 64, py = (2 y - H) / H.
#
# Cluster 0 is a full "wall" group at z = -9 .. -9.16 (wall triangle 0 is the
# nearest everywhere).  Every other cluster is compact, owns one image row (its
# band) and is a comb: for every COMB_PITCH-th column of its interval
# [x0, x1) one small triangle at depth 5 centred on that column's ray (the
# evidence), and behind each of them, on the same ray, copies scaled from the
# origin by 1 + COMB_LAYER per layer, which fill the cluster's 32 g slots and
# are never the closest hit.  The evidence of owned column number q lies in
# group q % g of the cluster, so every group of a 2- or 3-group cluster holds
# hits.  The boxes' y and z extents are the vertices' plus COMB_PAD; the x
# extent is chosen so that exactly the columns of [x0, x1) meet the box: each
# edge halfway between the neighbouring columns' rays over the box's depth
# range (asserted to be apart).

COMB_W = 64
COMB_PITCH = 2            # owned columns: every second one of the interval
COMB_Z = 5.0
COMB_FRONT = (0.0171, 0.0123, -1.0)
COMB_HX = 0.64            # viewportRight.x: columns are 0.1 apart at depth 5
COMB_ROW = 0.01           # viewportUp.y per image row: rows are 0.1 apart at depth 5
COMB_HALF = 0.012         # half-width of a comb triangle at depth 5 (12 % of the pixel pitch)
COMB_LAYER = 2.0e-4
COMB_PAD = 2.0 ** -8
WALL_Z = 9.0

# (x0, x1, groups): the needing sets (c0, c1) the one-block form must see ...
COMB_CASES_ONE = ((0, 32, 1), (32, 64, 2), (16, 48, 3), (31, 63, 1), (1, 33, 2), (9, 10, 3), (40, 41, 1),
                  (33, 64, 2), (20, 45, 3), (24, 56, 1), (8, 40, 2), (3, 34, 3))
# ... and the two-block side of the threshold, with a few more one-block ones
COMB_CASES_TWO = ((0, 33, 1), (31, 64, 2), (15, 48, 3), (0, 64, 1), (30, 34, 2), (20, 45, 1), (40, 50, 3))
COMB_SCENES = {"one": COMB_CASES_ONE, "two": COMB_CASES_TWO}
COMB_REQUIRED = ((32, 0), (0, 32), (16, 16), (1, 31), (31, 1), (1, 0), (0, 1), (0, 31), (12, 13), (8, 24),
                 (32, 1), (1, 32), (17, 16), (0, 0))


# The negative controls: (scene, band, the interval its box is shrunk to, victim column).  The victim owns a
# triangle of the cluster and its ray no longer needs the box.
COMB_CONTROLS = (("one", 0, (1, 32), 0),     # (32, 0) -> (31, 0)
                 ("one", 8, (21, 45), 20),   # the straddle (12, 13) -> (11, 13)
                 ("one", 2, (17, 48), 16),   # (16, 16), c0 + c1 = 32 -> (15, 16)
                 ("one", 9, (25, 56), 24),   # (8, 24), c0 + c1 = 32 -> (7, 24)
                 ("two", 0, (1, 33), 0),     # (32, 1), two blocks -> (31, 1), one block
                 ("two", 3, (1, 64), 0),     # (32, 32) -> (31, 32): still two blocks, every ray is swept
                 ("one", 8, (20, 44), 44))   # victim in lanes 32..63, c = 24 < 32: the first filler row


def comb_height(n_bands):
    return 8 * ((n_bands + 7) // 8)


def comb_uniforms(H, n_tris, bounces=1, rays=1, env=0, jitter=False, front=COMB_FRONT, right=None, up=None):
    """The comb scenes' view: camera at the origin, W = 64, deterministic primary rays unless jitter."""
    u = rt2.offline_uniforms(COMB_W, H, bounces, rays, n_tris)
    u.environmentalLight = int(env)
    right = (COMB_HX, 0.0, 0.0) if right is None else right
    up = (0.0, COMB_ROW * H, 0.0) if up is None else up
    for name, v in (("cameraPos", (0.0, 0.0, 0.0)), ("viewportFront", front), ("viewportRight", right),
                    ("viewportUp", up), ("pixelRight", (0.0, 0.0, 0.0)), ("pixelUp", (0.0, 0.0, 0.0)),
                    ("defocusDiskRight", (0.0, 0.0, 0.0)), ("defocusDiskUp", (0.0, 0.0, 0.0))):
        f = getattr(u, name)
        f.x, f.y, f.z, f.w = float(v[0]), float(v[1]), float(v[2]), 0.0
    if jitter:
        u.pixelRight.x = 2.0 * right[0] / COMB_W
        u.pixelUp.y = 2.0 * up[1] / H
    return u


def camera_rays_model(u):
    """The deterministic primary rays of the view u in numpy float32, as
    advance() forms them (rt2_path.h: end point, origin, normalize; the dot
    product's two fmaf through binary64).  -> (o, d), [H * W, 3], row-major."""
    f = np.float32
    W, H = int(u.width), int(u.height)
    v3 = lambda v: np.array([v.x, v.y, v.z], f)
    cam, right, up, front = v3(u.cameraPos), v3(u.viewportRight), v3(u.viewportUp), v3(u.viewportFront)
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    px = ((x.ravel() * 2 - W).astype(f) / f(W))[:, None]
    py = ((y.ravel() * 2 - H).astype(f) / f(H))[:, None]
    end = ((cam + front)[None, :] + right[None, :] * px) + up[None, :] * py
    o = np.broadcast_to(cam, end.shape).copy()
    v = end - o
    v64 = v.astype(np.float64)
    s = (v[:, 0] * v[:, 0]).astype(np.float64)
    s = (v64[:, 1] * v64[:, 1] + s).astype(f).astype(np.float64)
    s = (v64[:, 2] * v64[:, 2] + s).astype(f)
    with np.errstate(all="ignore"):
        return o, (v / np.sqrt(s)[:, None]).astype(f)


def _comb_dirs(H):
    """Per column and per row: the ray's x / depth and y / depth (float64 of the float32 view)."""
    f = np.float32
    dx = np.float64(f(COMB_FRONT[0])) + np.float64(f(COMB_HX)) * ((np.arange(COMB_W) * 2 - COMB_W) / COMB_W)
    dy = np.float64(f(COMB_FRONT[1])) + np.float64(f(COMB_ROW * H)) * ((np.arange(H) * 2 - H) / H)
    return dx, dy


def _box_x(dx, c_lo, c_hi, zn, zf):
    """The x extent that the rays of columns [c_lo, c_hi), and no others, meet between the depths zn and zf."""
    span = lambda c: (min(zn * dx[c], zf * dx[c]), max(zn * dx[c], zf * dx[c]))
    gap = 0.25 * COMB_HALF  # at least this much between a box edge and either neighbour's ray
    if c_lo == 0:
        x0 = span(0)[0] - 0.05
    else:
        out, inn = span(c_lo - 1)[1], span(c_lo)[0]
        assert inn - out > 2 * gap, "the columns' rays are not apart over the box's depth"
        x0 = 0.5 * (out + inn)
    if c_hi == COMB_W:
        x1 = span(COMB_W - 1)[1] + 0.05
    else:
        inn, out = span(c_hi - 1)[1], span(c_hi)[0]
        assert out - inn > 2 * gap, "the columns' rays are not apart over the box's depth"
        x1 = 0.5 * (inn + out)
    assert x0 < x1
    return np.float32(x0), np.float32(x1)


def comb_scene(cases, pitch=COMB_PITCH, last=32):
    """cases: the clusters in index order, (x0, x1, groups) for a comb and
    ("wall", groups) for a full cluster; a list of combs alone gets a one-group
    wall in front of it (cluster 0).  last: triangles of the scene's last
    group (a ragged one loses its last slots).  Returns a dict: triangles,
    materials (a light per triangle, coded by its index), ranges, H, bands (per
    comb: its cluster k, image row, x0, x1, groups, owned columns and the index
    of each one's evidence triangle), column and band_of per triangle (-1: a
    wall), wall_tri (the wall triangle in front of all others) and
    table(shrink=None): the explicit table; shrink = {band: (x0', x1')} gives
    those clusters the box of another interval (the negative controls: a
    well-formed box that leaves out a ray whose triangle is still in the
    cluster)."""
    cases = tuple(tuple(c) for c in cases)
    if all(c[0] != "wall" for c in cases):
        cases = (("wall", 1),) + cases
    key = ("comb", cases, pitch, last)
    if key in _cache:
        return _cache[key]
    assert 2 <= len(cases) <= rt2.MAX_CLUSTERS and 1 <= last <= 32
    H = comb_height(sum(c[0] != "wall" for c in cases))
    dx, dy = _comb_dirs(H)
    n_wall = 32 * sum(c[1] for c in cases if c[0] == "wall")
    star = (n_wall // 2 + 3) % n_wall if n_wall > 32 else 0  # the wall triangle in front, by its number among the walls
    va, vb, vc = [], [], []
    ranges, bands, g, walls, wall_tri = [], [], 0, 0, -1
    column, band_of = [], []  # per triangle: the column of the ray it is centred on, and its band
    for k, case in enumerate(cases):
        if case[0] == "wall":  # every triangle covers the whole view, each at its own depth
            groups = case[1]
            for i in range(32 * groups):
                z = -(WALL_Z + 0.005 * ((walls - star) * 37 % n_wall))
                if walls == star:
                    wall_tri = len(va)
                va.append((-40.0, -30.0, z)), vb.append((40.0, -30.0, z)), vc.append((0.0, 50.0, z))
                column.append(-1), band_of.append(-1)
                walls += 1
            ranges.append((g, g + groups, False))
            g += groups
            continue
        x0, x1, groups = case
        band = len(bands)
        owned = np.arange(x0, x1, pitch)
        slots = 32 * groups - (32 - last if k == len(cases) - 1 else 0)
        assert len(owned) <= 32 and 0 <= x0 < x1 <= COMB_W
        slot_of = [None] * slots  # (layer, owned column number)
        evidence = []
        for q in range(len(owned)):
            s = 32 * (q % groups) + q // groups
            slot_of[s] = (0, q)
            evidence.append(32 * g + s)
        layer, q = 1, 0
        for s in range(slots):
            if slot_of[s] is None:
                slot_of[s] = (layer, q)
                q += 1
                if q == len(owned):
                    layer, q = layer + 1, 0
        for lay, q in slot_of:
            t = COMB_Z * (1.0 + COMB_LAYER * lay)
            w = COMB_HALF * t / COMB_Z
            p = np.array([t * dx[owned[q]], t * dy[band], -t])
            va.append(p + (-w, -w, 0)), vb.append(p + (w, -w, 0)), vc.append(p + (0, w, 0))
            column.append(int(owned[q])), band_of.append(band)
        bands.append(dict(k=k, row=band, x0=x0, x1=x1, groups=groups, owned=owned, evidence=np.array(evidence)))
        ranges.append((g, g + groups, True))
        g += groups
    a, b, c = _wind(*(np.array(v, np.float64).astype(np.float32) for v in (va, vb, vc)))
    tris = _triangles(a, b, c)
    assert len(tris) == 32 * (g - 1) + (last if cases[-1][0] != "wall" else 32)
    mats = code_materials(len(tris))
    base = explicit_table(tris, ranges, pad=COMB_PAD)

    def table(shrink=None):
        t = base.copy()
        for band, bd in enumerate(bands):
            lo_c, hi_c = (shrink or {}).get(band, (bd["x0"], bd["x1"]))
            k = bd["k"]
            zn, zf = -float(t["c"][k]["hi"][2]), -float(t["c"][k]["lo"][2])
            t["c"][k]["lo"][0], t["c"][k]["hi"][0] = _box_x(dx, lo_c, hi_c, zn, zf)
        return t

    tris.setflags(write=False)
    mats.setflags(write=False)
    _cache[key] = dict(triangles=tris, materials=mats, ranges=ranges, H=H, bands=bands, table=table, pitch=pitch,
                       column=np.array(column), band_of=np.array(band_of), wall_tri=wall_tri)
    return _cache[key]


# The full table: 38 groups in 13 clusters, compact and full in turn, single-group clusters of both kinds, and
# group 37 in a compact cluster that only its own row needs.
FULL_CASES = ((0, 32, 1), ("wall", 3), (20, 45, 4), ("wall", 2), (0, 33, 5), ("wall", 1), (31, 64, 3), ("wall", 2),
              (9, 10, 4), ("wall", 3), (16, 48, 1), ("wall", 5), (40, 64, 4))
FULL_RAGGED_LAST = 7


def named_comb_scene(name):
    """"one", "two" (COMB_SCENES), "full" (38 whole groups: 1,216 triangles) or "ragged" (its last group cut to 7)."""
    if name in COMB_SCENES:
        return comb_scene(COMB_SCENES[name])
    sc = comb_scene(FULL_CASES, last=32 if name == "full" else FULL_RAGGED_LAST)
    assert len(sc["ranges"]) == rt2.MAX_CLUSTERS and sc["ranges"][-1][1] == 38
    return sc


def need_counts(t, o, d, k):
    """(c0, c1) of every 64-ray row for cluster k, and the rows' need masks (Python ints)."""
    bits = ((rt2.cluster_need(t, o, d) >> np.uint32(k)) & 1).reshape(-1, 64)
    masks = [sum(1 << int(l) for l in np.flatnonzero(r)) for r in bits]
    return bits[:, :32].sum(1).astype(int), bits[:, 32:].sum(1).astype(int), masks


def row_model(need):
    """cluster_rows_frag (rt2_k5_resident.h) for a 64-bit need mask of at most
    32 bits, restated: per lane the row it gives its ray (rk for a needing
    lane, `rest` for another), per block; then the result's rows by the
    `first` select.  -> (rows of block 0's lanes [32], of block 1's [32], the
    source lane of each result row [32], -1 where a block's rows are not a
    permutation)."""
    need = int(need)
    bit = [(need >> l) & 1 for l in range(64)]
    c0, c1 = sum(bit[:32]), sum(bit[32:])
    assert c0 + c1 <= 32
    row = []
    for l in range(64):
        rk = sum(bit[:l])  # lanes_below(need)
        rest = ((l - rk) + (c0 if l < 32 else c1 + 2 * c0)) & 31
        row.append(rk if bit[l] else rest)
    rows0, rows1 = row[:32], row[32:]
    src = []
    for j in range(32):  # ds_permute: lane j receives from the lane that names it
        from0 = [l for l in range(32) if rows0[l] == j]
        from1 = [32 + l for l in range(32) if rows1[l] == j]
        pick = from0 if j < c0 else from1  # `first`
        src.append(pick[0] if len(pick) == 1 else -1)
    return rows0, rows1, src


def swept_lanes(need):
    """The lanes whose rays a compact cluster's sweep holds, in a wave of 64 live rays with this need mask."""
    need = int(need)
    c = bin(need).count("1")
    if c == 0:
        return set()
    if c > 32:
        return set(range(64))
    return set(row_model(need)[2])
