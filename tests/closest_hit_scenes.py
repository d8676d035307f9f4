"""Scenes whose image says which triangle won the closest-hit scan.

Host half of tests/test_gpu_closest_hit.py (needs the GPU); its premises are
checked on the CPU oracle alone by tests/test_closest_hit_scenes.py.  Only
numpy here: triangle and material arrays (rt2.TRI_DTYPE, rt2.MAT_DTYPE).

Index-coded lights: material i is a LIGHT of strength 1 whose emission colour
spells i in base 21, and triangle i uses material i.  With 1 ray per pixel,
1 frame and the environment light off, trace() returns at the first hit of a
LIGHT, so a pixel is exactly the tone-mapped emission of the triangle hit (or
0 on a miss) and decode() reads the winner's index back from the float bits.
"""
import numpy as np

import rt2

LEVELS = 21
# LEV[k] = float32(k + 1) / float32(21): no level is 0, so a miss (0, 0, 0) is not a code
LEV = np.arange(1, LEVELS + 1, dtype=np.float32) / np.float32(LEVELS)
MAX_CODES = LEVELS ** 3  # 9,261 > 8,193

CAMERA = (0.0, 5.0, 10.0)  # rt2.default_camera: at (0, 5, 10) looking down -z
CHAMP_Z = 5.0              # the champions' plane; the view there is +-2.3 x +-1.28 around (0, 5)
VIEW_X, VIEW_Y = 2.3, 1.28


def tone_levels():
    """The 21 levels after tonemapACES + toSRGB (the oracle's own function), as float32."""
    import oracle
    f = oracle.lib().oracle_tonemap_srgb
    t = np.array([f(float(v)) for v in LEV], dtype=np.float32)
    assert len(np.unique(t)) == LEVELS and np.all(np.diff(t) > 0)
    return t


def code_materials(n):
    """n LIGHT materials; material i's emission colour is i in base 21 (r = lowest digit)."""
    assert 0 < n <= MAX_CODES
    i = np.arange(n)
    m = np.zeros(n, dtype=rt2.MAT_DTYPE)
    m["color"][:, :3] = 1.0
    m["textureIndex"] = -1
    m["materialType"] = rt2.LIGHT
    m["emissionStrength"] = 1.0
    m["emissionColor"][:, 0] = LEV[i % LEVELS]
    m["emissionColor"][:, 1] = LEV[i // LEVELS % LEVELS]
    m["emissionColor"][:, 2] = LEV[i // (LEVELS * LEVELS) % LEVELS]
    return m


def mixed_materials(n, light_every=8):
    """code_materials with only every light_every-th triangle left a light; the
    others alternate between diffuse grey and a perfect mirror, so paths go on
    in incoherent directions for several segments."""
    m = code_materials(n)
    i = np.arange(n)
    other = i % light_every != 0
    mirror = other & (i % 2 == 1)
    m["materialType"][other] = rt2.DIFFUSE
    m["emissionStrength"][other] = 0.0
    m["emissionColor"][other] = 0.0
    m["color"][other, :3] = 0.9
    m["materialType"][mirror] = rt2.SPECULAR
    m["color"][mirror, :3] = 1.0
    m["specularColor"][mirror, :3] = 1.0
    m["smoothness"][mirror] = 1.0
    m["specularProbability"][mirror] = 1.0
    return m


def encode(idx, levels=None):
    """The image (..., 3) float32 that index-coded lights give for winners idx (-1 = miss)."""
    t = tone_levels() if levels is None else levels
    idx = np.asarray(idx)
    hit = idx >= 0
    j = np.where(hit, idx, 0)
    img = np.stack([t[j % LEVELS], t[j // LEVELS % LEVELS], t[j // (LEVELS * LEVELS) % LEVELS]], -1)
    img[~hit] = 0.0
    return img.astype(np.float32)


def decode(img, levels=None):
    """Per-pixel triangle index of an index-coded image (..., >= 3), -1 for a
    miss.  Raises ValueError on any channel whose bits are not a level."""
    t = tone_levels() if levels is None else levels
    bits = np.ascontiguousarray(img[..., :3], dtype=np.float32).view(np.uint32)
    tb = t.view(np.uint32)  # increasing (positive floats order like their bits)
    k = np.searchsorted(tb, bits)
    k = np.minimum(k, LEVELS - 1)
    is_level = tb[k] == bits
    miss = (bits == 0).all(-1)
    bad = ~(is_level.all(-1) | miss)
    if bad.any():
        where = np.argwhere(bad)[0]
        raise ValueError(f"{int(bad.sum())} pixels are not index codes, first at {tuple(int(v) for v in where)}: "
                         f"{img[tuple(where)][:3]}")
    idx = k[..., 0] + LEVELS * k[..., 1] + LEVELS * LEVELS * k[..., 2]
    return np.where(miss, -1, idx).astype(np.int64)


def _triangles(a, b, c):
    n = len(a)
    t = np.zeros(n, dtype=rt2.TRI_DTYPE)
    t["a"][:, :3], t["b"][:, :3], t["c"][:, :3] = a, b, c
    t["materialIndex"] = np.arange(n)
    return t


def n_groups(n):
    return (n + 31) // 32


def champ(g, n):
    """Group g's champion: a different slot of each 32-triangle group."""
    return min(32 * g + 7 * g % 32, n - 1)


def soup(n, seed, extent=0.45):
    """n small random triangles (the other two vertices within +-extent of the
    first) facing the camera in the box x [-4.6, 4.6],
    y [2.4, 7.6], z [-4, 4]; in each 32-triangle group the champion is replaced
    by a small upright triangle in the plane z = 5 (in front of all the others),
    in its own cell of a cols x rows grid over the view, half-width 0.35 of the
    cell: every group owns pixels where its champion is the closest hit, and the
    rest of the image is a random competition."""
    rng = np.random.default_rng(seed)
    ctr = np.stack([rng.uniform(-4.6, 4.6, n), rng.uniform(2.4, 7.6, n), rng.uniform(-4.0, 4.0, n)], 1)
    b = ctr + rng.uniform(-extent, extent, (n, 3))
    c = ctr + rng.uniform(-extent, extent, (n, 3))
    a, b, c = (v.astype(np.float32) for v in (ctr, b, c))
    nz = (b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0])
    flip = nz < 0  # wind so that n.z > 0: the test culls back faces
    b[flip], c[flip] = c[flip].copy(), b[flip].copy()
    ng = n_groups(n)
    cols = int(np.ceil(np.sqrt(16 * ng / 9)))
    rows = -(-ng // cols)
    cw, ch = 2 * VIEW_X / cols, 2 * VIEW_Y / rows
    for g in range(ng):
        i = champ(g, n)
        cx = -VIEW_X + (g % cols + 0.5) * cw
        cy = CAMERA[1] - VIEW_Y + (g // cols + 0.5) * ch
        hw, hh = 0.35 * cw, 0.35 * ch
        a[i] = (cx - hw, cy - hh, CHAMP_Z)
        b[i] = (cx + hw, cy - hh, CHAMP_Z)
        c[i] = (cx, cy + hh, CHAMP_Z)
    return _triangles(a, b, c)


def with_ties(tris, families):
    """A copy of tris in which, for each family (source, copy, copy, ...), the
    three vertices of the source triangle (not its material) are written onto
    the other indices: exact distance ties at every ray that hits them.  The
    sequential strict `dst < best` scan gives every such pixel to the family's
    lowest index."""
    t = tris.copy()
    for fam in families:
        src = fam[0]
        for i in fam[1:]:
            for k in "abc":
                t[k][i] = t[k][src]
    return t


def tie_families(n):
    """The families of the tie scenes at the sizes the tests use: copies across
    the first group's end, the tile edge at 19 x 32, the resident/L2 edge at
    38 x 32, the last full group and a one-triangle ragged group (where the
    size has them), and a copy far below its original.  Every source is a
    champion, so the family is the closest hit of some pixels."""
    fams = [[champ(0, n), 31, 32], [champ(18, n), 607, 608]]
    if n == 1216:
        fams += [[champ(37, n), 1214, 1215], [champ(30, n), 5]]
    elif n == 1217:
        fams += [[champ(37, n), 1215, 1216], [champ(30, n), 5]]
    elif n == 8192:
        fams += [[champ(37, n), 1215, 1216], [champ(100, n), 8190, 8191], [champ(200, n), 5]]
    elif n == 8193:
        fams += [[champ(37, n), 1215, 1216], [champ(100, n), 8191, 8192], [champ(200, n), 5]]
    else:
        raise ValueError(f"no tie families for {n} triangles")
    for f in fams:
        assert len(set(f)) == len(f) and max(f) < n
    return fams


def fan(n, seed, order):
    """n triangles over the same (x, y) footprint (-40, -20), (40, -20), (0, 50),
    each on its own plane z = a x + b (y - 5) + c with a, b in +-0.05 and c in
    +-0.2: every triangle covers every pixel, so every ray has n true hits at
    nearly equal distances.  order sorts by c: "far_first" (the bound improves
    along the whole scan and the winner is in the last groups), "near_first" (an
    early index wins and all that follow must lose the strict <) or "shuffled"."""
    rng = np.random.default_rng(seed)
    ca, cb, cc = rng.uniform(-0.05, 0.05, n), rng.uniform(-0.05, 0.05, n), rng.uniform(-0.2, 0.2, n)
    if order == "far_first":
        o = np.argsort(cc, kind="stable")
    elif order == "near_first":
        o = np.argsort(-cc, kind="stable")
    elif order == "shuffled":
        o = np.arange(n)
    else:
        raise ValueError(order)
    ca, cb, cc = ca[o], cb[o], cc[o]
    out = []
    for x, y in ((-40.0, -20.0), (40.0, -20.0), (0.0, 50.0)):  # (b - a) x (c - a) has z > 0
        out.append(np.stack([np.full(n, x), np.full(n, y), ca * x + cb * (y - 5.0) + cc], 1).astype(np.float32))
    return _triangles(*out)


def scene_data(tris, mats, bvh=True):
    """The arrays as an rt2.SceneData (add_material, add_triangles, build_bvh).
    build_bvh reorders the triangles, each keeping its material: a decoded
    index is still the index in `tris`."""
    sd = rt2.SceneData()
    M = rt2.Material
    for rec in mats:
        m = M.from_buffer_copy(rec.tobytes())
        sd.add_material(m)
    sd.add_triangles(tris)
    if bvh:
        sd.build_bvh()
    return sd


def coded_uniforms(width, height, n):
    """1 ray, 1 frame's settings, bounce limit 1, environment light off."""
    u = rt2.offline_uniforms(width, height, 1, 1, n)
    u.environmentalLight = 0
    return u


# The scenes of the tests: triangle count -> image size; the seeds of the
# recipes (tests/test_closest_hit_scenes.py asserts what they must give).
SIZES = {1216: (64, 36), 1217: (64, 36), 8192: (128, 72), 8193: (128, 72)}
KINDS = ("soup", "ties", "fan_far_first", "fan_near_first", "fan_shuffled")
SOUP_SEED, FAN_SEED = 41, 5
TILE_SHAPE_GROUPS = (1, 9, 10, 19, 20, 28, 29, 39, 57)  # n = 32 ng - 13 triangles each
ROW_RUN_TRIS = 2400

_scenes = {}


def coded_scene(kind, n):
    """(triangles, materials) of an index-coded scene, built once and read-only."""
    if (kind, n) not in _scenes:
        if kind == "soup":
            t = soup(n, SOUP_SEED)
        elif kind == "ties":
            t = with_ties(soup(n, SOUP_SEED), tie_families(n))
        elif kind.startswith("fan_"):
            t = fan(n, FAN_SEED, kind[4:])
        else:
            raise ValueError(kind)
        m = code_materials(n)
        t.setflags(write=False)
        m.setflags(write=False)
        _scenes[(kind, n)] = (t, m)
    return _scenes[(kind, n)]


def mixed_extent(n):
    """The triangles' extent in the mixed soups: the index-coded soup's 0.45 at
    8,192 triangles and up, and below that larger by sqrt(8192 / n), so that the
    triangles' total area stays that of the 8,192-triangle soup: as few primary
    rays miss and as many scattered rays hit again, whatever the count."""
    return 0.45 * max(1.0, (8192 / n) ** 0.5)


def mixed_scene(n):
    """(triangles, materials) of the soup with mixed materials, built once and read-only."""
    if ("mixed", n) not in _scenes:
        t, m = soup(n, SOUP_SEED, mixed_extent(n)), mixed_materials(n)
        t.setflags(write=False)
        m.setflags(write=False)
        _scenes[("mixed", n)] = (t, m)
    return _scenes[("mixed", n)]
