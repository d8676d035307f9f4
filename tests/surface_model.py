"""Scenes, rays and a float64 model for the surface-query tests.

Host half of tests/test_gpu_surface.py (needs the GPU); its premises are
checked on the CPU oracle and this model alone by tests/test_surface_cpu.py.
Only numpy here.

The model restates, in binary64 from the binary32 vertices and rays, what a
surface record holds besides the oracle's (dst, tri):

  unit_normals   normalize(cross(b - a, c - a)) per triangle, and the bound
                 4 * 2^-23 * (|e0||e1| / |cross| + 1) per component: three
                 fused cross products and a normalisation, each rounding at
                 most 2^-24 relative, the products relative to |e0||e1|;
  barycentrics   rayTriangleIntersect's u, v (compute.glsl:322-337: the
                 weights of b and c) and the bound 16 * 2^-24 * (|e||d||ao| /
                 |det| + 1), e the longer edge: about ten roundings of at most
                 2^-24, each relative to the product of norms;
  camera_dirs    main's basicShading ray (compute.glsl:665-676); the device's
                 direction is within 2^-21 per component: at most six
                 roundings on a unit vector.

The bounds come from the formats and the operation counts, not from what any
kernel returns; test_surface_cpu.py asserts that they stay below 1e-4 on every
scene used, which is a condition on the scenes.
"""
import numpy as np

import closest_hit_scenes as S
import shading_scenes as ss
import trace_rays_lib as T

F32 = np.float32
GLASS_HIGHLIGHT, UNKNOWN = 6, 9
TYPES = (ss.DIFFUSE, ss.SPECULAR, ss.LIGHT, ss.CHECKER, ss.GLASS, ss.TEXTURE, GLASS_HIGHLIGHT, UNKNOWN)
PURE_TYPES = (ss.DIFFUSE, ss.SPECULAR, ss.LIGHT, ss.GLASS, GLASS_HIGHLIGHT, UNKNOWN)  # albedo = f(material) alone
CAMERA_TOL = 2.0 ** -21
MAX_TOL = 1e-4


# ---- the float64 model -----------------------------------------------------------------------------------------

def _edges(tris):
    a, b, c = (np.asarray(tris[k][:, :3], np.float64) for k in "abc")
    return a, b - a, c - a


def _norm(v):
    return np.sqrt((v * v).sum(-1))


def unit_normals(tris):
    """(normal float64 [n, 3], bound float64 [n])."""
    _, e0, e1 = _edges(tris)
    n = np.cross(e0, e1)
    ln = _norm(n)
    return n / ln[:, None], 4 * 2.0 ** -23 * (_norm(e0) * _norm(e1) / ln + 1)


def barycentrics(tris, tri, o, d):
    """(u, v, bound), float64 [n], of rays (o, d) on triangles tris[tri]."""
    a, e0, e1 = (x[tri] for x in _edges(tris))
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    n = np.cross(e0, e1)
    det = -(d * n).sum(-1)
    ao = o - a
    q = np.cross(d, ao)
    u = -(e1 * q).sum(-1) / det
    v = (e0 * q).sum(-1) / det
    e = np.maximum(_norm(e0), _norm(e1))
    return u, v, 16 * 2.0 ** -24 * (e * _norm(d) * _norm(ao) / np.abs(det) + 1)


def slab_rows(un, shard=None):
    """The image rows of a shard's slab, (tile_rows, rank, nranks); None: the whole image."""
    h = un["height"]
    if shard is None:
        return np.arange(h)
    tile, rank, nranks = shard
    return np.array([y for y in range(h) if y // tile % nranks == rank])


def camera_dirs(un, shard=None):
    """The slab's primary directions, float64 [rows * W, 3], slab-row order."""
    w, h = un["width"], un["height"]
    rows = slab_rows(un, shard)
    x = (2.0 * np.arange(w) - w) / w
    y = (2.0 * rows - h) / h
    f, r, up = (np.array(un[k], np.float64) for k in ("viewportFront", "viewportRight", "viewportUp"))
    d = f[None, None, :] + r[None, None, :] * x[None, :, None] + up[None, None, :] * y[:, None, None]
    d = d.reshape(-1, 3)
    return d / _norm(d)[:, None]


# ---- materials whose base colour is a function of the material alone -------------------------------------------

def pure_materials(n, seed=11):
    """n materials cycling through PURE_TYPES with random colours; every other
    LIGHT has an emission component above 1 (normalizeColor divides)."""
    rng = np.random.default_rng(seed)
    m = np.zeros(n, ss.MAT_DTYPE)
    i = np.arange(n)
    m["materialType"] = np.array(PURE_TYPES)[i % len(PURE_TYPES)]
    m["color"][:, :3] = rng.uniform(0.05, 1.0, (n, 3))
    m["color"][:, 3] = 1.0
    m["specularColor"][:] = 1.0
    m["emissionColor"][:, :3] = rng.uniform(0.05, 1.0, (n, 3)) * np.where(i // len(PURE_TYPES) % 2 == 1, 3.0, 1.0)[:, None]
    m["emissionStrength"] = 1.0
    m["refractiveIndex"] = 1.5
    m["textureIndex"] = -1
    m["index"] = i
    m.setflags(write=False)
    return m


def pure_albedo(mats):
    """The base colour of each material of PURE_TYPES, float32 [n, 3] (traceBasic, one bounce, no shadow)."""
    t = mats["materialType"]
    assert np.isin(t, PURE_TYPES).all()
    out = np.zeros((len(mats), 3), F32)
    col = np.isin(t, (ss.DIFFUSE, ss.SPECULAR, ss.GLASS))
    out[col] = mats["color"][col, :3]
    lit = t == ss.LIGHT
    e = mats["emissionColor"][lit, :3].astype(F32)
    mx = e.max(1, keepdims=True)
    out[lit] = np.where(mx > 1, e / np.where(mx > 1, mx, F32(1)), e)  # binary32 division, correctly rounded
    out[t == UNKNOWN] = (1.0, 0.0, 1.0)
    return out


# ---- the (dst, tri) scenes: trace_rays_lib's soups with pure materials -----------------------------------------

HIT_SCENES = (("soup", 1), ("far", 33), ("soup", 1216), ("soup", 1217))
RAY_COUNTS = (1, 63, 64, 65, 1025)
_rays = {}


def hit_scene_rays(kind, n):
    """1,025 rays of a (dst, tri) scene; the smaller counts are prefixes.  On
    the 1,217-triangle soup rays 40 .. 47 aim at triangle 1,216, the champion
    of the group read from L2 (in front of everything else in its cell)."""
    if (kind, n) not in _rays:
        tris = T.scene_tris(kind, n)
        o, d = T.make_rays(tris, 1025)
        if n == 1217:
            po, pd = T.rays_at(tris, 1216, 8, 99)
            o, d = o.copy(), d.copy()
            o[40:48], d[40:48] = po, pd
        o.setflags(write=False)
        d.setflags(write=False)
        _rays[(kind, n)] = (o, d)
    return _rays[(kind, n)]


# ---- fat triangles: the barycentrics' bound stays small ---------------------------------------------------------

def fat_triangles(n=40, seed=3):
    """n near-equilateral triangles of circumradius 0.8 .. 1.4, tilted up to 30
    degrees off the camera's axis, in the soups' box: long edges, no slivers,
    no grazing hits from around the camera."""
    rng = np.random.default_rng(seed)
    ctr = np.stack([rng.uniform(-3, 3, n), rng.uniform(3, 7, n), rng.uniform(-3, 3, n)], 1)
    r = rng.uniform(0.8, 1.4, n)
    ph = rng.uniform(0, 2 * np.pi, n)
    tx, ty = rng.uniform(-0.5, 0.5, n), rng.uniform(-0.5, 0.5, n)  # slopes dz/dx, dz/dy
    v = []
    for k in range(3):
        x, y = r * np.cos(ph + 2 * np.pi * k / 3), r * np.sin(ph + 2 * np.pi * k / 3)
        v.append(ctr + np.stack([x, y, tx * x + ty * y], 1))  # counter-clockwise seen from +z: n.z > 0
    t = S._triangles(*(p.astype(F32) for p in v))
    t.setflags(write=False)
    return t


def fat_rays(n=257, seed=5):
    """From around the camera toward uniform points of the box: hits and misses."""
    rng = np.random.default_rng(seed)
    o = np.asarray(S.CAMERA) + rng.uniform(-0.5, 0.5, (n, 3))
    target = rng.uniform((-4.5, 1.5, -3.0), (4.5, 8.5, 3.0), (n, 3))
    d = target - o
    return o.astype(F32), (d / _norm(d)[:, None]).astype(F32)


# ---- the view: every material type in one picture ---------------------------------------------------------------

VIEW_SIZES = ((67, 10), (64, 4))
VIEW_CAMERAS = ((0.0, 0.0, 0.0), (0.11, 0.07, 0.4), (0.06, -0.05, -0.15))
VIEW_TEXTURE_INDICES = (0, 1, 2, 7)  # sampled, sampled, at or above numTextures (a unit with no image), at or above 5
VIEW_NUM_TEXTURES = 2
_views = {}


def view_textures():
    return ss._textures()[:VIEW_NUM_TEXTURES]


def view_scene(width, height, cam, total=0):
    """Nine bands side by side in the plane z = -3, seen from `cam` looking down
    -z through a 0.8 x 0.6 viewport: DIFFUSE, SPECULAR, LIGHT (lower half an
    emission below 1, upper half above), CHECKER, GLASS, TEXTURE (four quads
    above each other, indices VIEW_TEXTURE_INDICES), GLASS_HIGHLIGHT, a type the
    shader does not know (9), and nothing.  Padded to `total` triangles with
    inert ones.  basicShading = 1, one bounce, no shadow ray, the sky on."""
    key = (width, height, cam, total)
    if key in _views:
        return _views[key]
    b = ss._Builder()
    x0, bw, ylo, yhi = -2.4, 4.8 / 9, -2.6, 2.6
    wide = [(-0.7, -0.35), (1.9, -0.35), (1.9, 2.6), (-0.7, 2.6)]

    def band(k, mat, y0=ylo, y1=yhi, uv=None):
        left = x0 + k * bw - (1.0 if k == 0 else 0.0)  # the first band reaches past the view's edge
        b.quad((left, y0, -3.0), (x0 + (k + 1) * bw - left, 0, 0), (0, y1 - y0, 0), mat, uv)

    band(0, b.material(ss.DIFFUSE, color=(0.3, 1.0, 0.6)))
    band(1, b.material(ss.SPECULAR, color=(0.9, 0.7, 0.3), smooth=1.0, prob=1.0))
    band(2, b.light((0.9, 0.5, 0.2), 0.7), ylo, 0.1)  # the splits lie off the pixel centres of both sizes
    band(2, b.light((3.0, 1.5, 0.75), 2.0), 0.1, yhi)
    band(3, b.material(ss.CHECKER, checker=1.7))
    band(4, b.material(ss.GLASS, color=(0.6, 0.8, 1.0), ior=1.5))
    ys = (ylo, -1.1, -0.2, 0.7, yhi)
    for j, index in enumerate(VIEW_TEXTURE_INDICES):
        band(5, b.material(ss.TEXTURE, texture=index), ys[j], ys[j + 1], wide)
    band(6, b.material(GLASS_HIGHLIGHT, color=(0.5, 0.5, 0.5)))
    band(7, b.material(UNKNOWN, color=(0.2, 0.3, 0.4)))
    b.inert(total)
    sc = b.scene(f"surface_view/{width}x{height}/n{len(b.tris)}", width, height, 1, 1, True, textures=view_textures(),
                 num_textures=VIEW_NUM_TEXTURES, cam=cam)
    sc["uniforms"]["basicShading"] = 1
    sc["uniforms"]["basicShadingShadow"] = 0
    for k in ("triangles", "materials"):
        sc[k].setflags(write=False)
    _views[key] = sc
    return sc


def view_rays(un, shard=None):
    """The model's camera rays of a view as binary32 (o, d): for the premises; the GPU tests trace the device's own."""
    d = camera_dirs(un, shard).astype(F32)
    o = np.broadcast_to(np.array(un["cameraPos"], F32), d.shape).copy()
    return o, d
