"""Rays, scenes and the reference of the ray-query tests.

Host half of tests/test_gpu_trace_rays.py (needs the GPU); its premises are
checked on the CPU oracle alone by tests/test_trace_rays_cpu.py.

The reference is computed here from the oracle's own rayTriangleIntersect
(oracle_ray_triangle): per ray, every triangle of the array as uploaded, in
index order, with a strict `dst < best` started at the ray's bound.  No case
samples or skips rays; every case stays at or below 2 M (ray, triangle) pairs
(about 0.8 us each through ctypes).
"""
import ctypes as C

import numpy as np

import closest_hit_scenes as S

F32 = np.float32
UNBOUNDED = F32(1e38)
BOX_LO = np.array([-4.6, 2.4, -4.0])
BOX_HI = np.array([4.6, 7.6, 4.0])
SEED = 7
MAX_PAIRS = 2_000_000


def bound_of(tmax):
    """bound_i of include/rt2.h: tmax when 0 < tmax < 1e38f, otherwise 1e38f."""
    t = np.asarray(tmax, dtype=F32)
    with np.errstate(invalid="ignore"):
        return np.where((t > 0) & (t < UNBOUNDED), t, UNBOUNDED).astype(F32)


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def make_rays(tris, n, seed=SEED):
    """n rays (origins, directions as float32 (n, 3), directions of unit length
    to float32 rounding): half from around the camera toward a random point of
    a random triangle (so also a 1-triangle scene is hit), a quarter from
    around the camera toward a random point of the soup's box, a quarter from
    inside the box in uniformly random directions (those pointing away from
    the camera meet only back faces: misses).  The kinds are interleaved, so
    every prefix and every 64-ray chunk holds all three."""
    rng = np.random.default_rng(seed)
    kind = np.arange(n) % 4  # 0, 1: aimed; 2: box; 3: inside
    cam = np.asarray(S.CAMERA) + rng.uniform(-0.5, 0.5, (n, 3))
    t = rng.integers(0, len(tris), n)
    w = rng.dirichlet((1.0, 1.0, 1.0), n)
    a, b, c = (tris[k][t, :3].astype(np.float64) for k in "abc")
    aimed = w[:, :1] * a + w[:, 1:2] * b + w[:, 2:] * c
    box = rng.uniform(BOX_LO, BOX_HI, (n, 3))
    o = np.where((kind == 3)[:, None], rng.uniform(BOX_LO, BOX_HI, (n, 3)), cam)
    target = np.where((kind <= 1)[:, None], aimed, box)
    d = np.where((kind == 3)[:, None], _unit(rng.normal(size=(n, 3))), _unit(target - o))
    return o.astype(F32), d.astype(F32)


def rays_at(tris, index, k, seed):
    """k rays from around the camera toward interior points of triangle `index`."""
    rng = np.random.default_rng(seed)
    cam = np.asarray(S.CAMERA) + rng.uniform(-0.5, 0.5, (k, 3))
    w = rng.dirichlet((4.0, 4.0, 4.0), k)  # away from the edges
    a, b, c = (tris[x][index, :3].astype(np.float64) for x in "abc")
    target = w[:, :1] * a + w[:, 1:2] * b + w[:, 2:] * c
    return cam.astype(F32), _unit(target - cam).astype(F32)


def tie_rays(tris, families, n):
    """make_rays(n - 8 per family) followed by 8 rays at each family's source."""
    k = 8
    o, d = make_rays(tris, n - k * len(families))
    parts = [(o, d)] + [rays_at(tris, fam[0], k, 100 + i) for i, fam in enumerate(families)]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def reference(oraclemod, tris, o, d, tmax=None):
    """(dst float32[n], tri int32[n], ties int32[n]): the sequential scan of the
    module docstring; ties[i] = triangles whose accepted distance equals the
    winner's (1 = no exact tie, 0 on a miss)."""
    f = oraclemod.lib().oracle_ray_triangle
    tris = np.ascontiguousarray(tris)
    assert tris.dtype.itemsize == 80
    n, nt = len(o), len(tris)
    assert n * nt <= MAX_PAIRS, f"{n} rays x {nt} triangles: more than {MAX_PAIRS} pairs"
    o = np.ascontiguousarray(o, dtype=F32)
    d = np.ascontiguousarray(d, dtype=F32)
    bound = bound_of(np.zeros(n, F32) if tmax is None else np.broadcast_to(np.asarray(tmax, F32), (n,)))
    out = C.c_float()
    pout = C.addressof(out)
    addr = [tris.ctypes.data + 80 * t for t in range(nt)]
    dst = np.empty(n, F32)
    tri = np.empty(n, np.int32)
    ties = np.zeros(n, np.int32)
    for i in range(n):
        po, pd = o.ctypes.data + 12 * i, d.ctypes.data + 12 * i
        best, bi, same = float(bound[i]), -1, 0
        for t in range(nt):
            if f(po, pd, addr[t], pout):
                v = out.value
                if v < best:
                    best, bi, same = v, t, 1
                elif v == best and bi >= 0:
                    same += 1
        dst[i], tri[i], ties[i] = best, bi, same
    for a in (dst, tri, ties):
        a.setflags(write=False)
    return dst, tri, ties


# ---- the scenes of the tests (built once, read-only) ----------------------
SOUP_SIZES = (1, 32, 33, 1216, 1217, 8192, 8193)
RAY_COUNTS = (1, 31, 32, 33, 63, 64, 65, 1025)  # on the 1,217-triangle soup
FAN_ORDERS = ("far_first", "near_first")
FAR = float(2 ** 21)

_tris = {}
_refs = {}


def n_rays_for(n_tris):
    return 193 if n_tris <= 1217 else 97


def scene_tris(kind, n):
    """soup: S.soup(n, SOUP_SEED); ties: the 1,217-triangle soup with its tie
    families; fan_<order>: S.fan(64, FAN_SEED, order); far: the 33-triangle
    soup with vertex a of triangle 5 at x = 2^21, outside the matrix filter's
    range (|a| <= 2^20)."""
    if (kind, n) not in _tris:
        if kind == "soup":
            t = S.soup(n, S.SOUP_SEED)
        elif kind == "ties":
            t = S.with_ties(S.soup(n, S.SOUP_SEED), S.tie_families(n))
        elif kind.startswith("fan_"):
            t = S.fan(n, S.FAN_SEED, kind[4:])
        elif kind == "far":
            t = S.soup(n, S.SOUP_SEED).copy()
            t["a"][5, 0] = FAR
        else:
            raise ValueError(kind)
        t.setflags(write=False)
        _tris[(kind, n)] = t
    return _tris[(kind, n)]


def scene_rays(kind, n, n_rays):
    tris = scene_tris(kind, n)
    if kind == "ties":
        return tie_rays(tris, S.tie_families(n), n_rays)
    return make_rays(tris, n_rays)


def scene_ref(oraclemod, kind, n, n_rays, tris=None, tag="brute"):
    """The unbounded reference of a scene's rays over `tris` (default: the
    scene's own array; the BVH tests pass the array build_bvh reordered),
    computed once per (scene, rays, array) and left unchanged."""
    key = (kind, n, n_rays, tag)
    if key not in _refs:
        o, d = scene_rays(kind, n, n_rays)
        _refs[key] = reference(oraclemod, scene_tris(kind, n) if tris is None else tris, o, d)
    return _refs[key]
