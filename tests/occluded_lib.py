"""Scenes, rays and chunks of the occlusion-query tests.

Host half of tests/test_gpu_occluded.py (needs the GPU); its premises are
checked on the CPU oracle alone by tests/test_occluded_cpu.py.  The soups, fans
and rays are those of tests/trace_rays_lib.py; added here is the *picket*
scene, which puts a ray's only occluder into any chosen 32-triangle group:

pickets(n): n small disjoint triangles in the plane z = 0, one per cell of a
40-column grid, front faces toward +z.  A ray from the eye (in front) through
the centroid of picket k is accepted by picket k and by no other triangle; a
ray through a grid corner (between the pickets) or from behind the plane
through a centroid (det < 0: a back face) is accepted by none.  pickets(m) is
the first m triangles of pickets(n) for m < n.

The reference of every test is oracle.closest_hits(...)[1] >= 0.
"""
import ctypes as C

import numpy as np

import closest_hit_scenes as S
import trace_rays_lib as T

F32 = np.float32
COLS = 40
STEP = 0.2           # cell size
HALF = 0.05          # a picket's half-width: a quarter of the cell
X0, Y0 = -4.0, 2.0   # the grid's lower left corner
EYE = (0.0, 5.0, 8.0)
BEHIND = (0.0, 5.0, -8.0)
PICKETS = (1216, 1217)   # every group resident; the last group (one triangle) from L2
MAX_SCAN_PAIRS = 600_000

_pickets = {}


def _centre(k):
    k = np.asarray(k)
    return np.stack([X0 + (k % COLS + 0.5) * STEP, Y0 + (k // COLS + 0.5) * STEP, np.zeros(k.shape)], -1)


def pickets(n):
    if n not in _pickets:
        c = _centre(np.arange(n))
        a = c + (-HALF, -HALF, 0.0)
        b = c + (HALF, -HALF, 0.0)
        top = c + (0.0, HALF, 0.0)
        t = S._triangles(a.astype(F32), b.astype(F32), top.astype(F32))  # n.z > 0: the front faces +z
        t.setflags(write=False)
        _pickets[n] = t
    return _pickets[n]


def _rays(origin, target):
    target = np.atleast_2d(np.asarray(target, np.float64))
    o = np.broadcast_to(np.asarray(origin, np.float64), target.shape)
    d = target - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o.astype(F32), d.astype(F32)


def centroid(n, k):
    """The centroid of picket k as stored (float32 vertices)."""
    t = pickets(n)
    return (t["a"][k, :3].astype(np.float64) + t["b"][k, :3] + t["c"][k, :3]) / 3.0


def aim(n, k):
    """Rays from the eye through the centroids of pickets k: accepted by k alone."""
    return _rays(EYE, centroid(n, np.asarray(k)))


def gap(i):
    """Rays from the eye through the grid corners i (row-major over COLS + 1 columns): accepted by none."""
    i = np.asarray(i)
    return _rays(EYE, np.stack([X0 + (i % (COLS + 1)) * STEP, Y0 + (i // (COLS + 1)) * STEP, np.zeros(i.shape)], -1))


def behind(n, k):
    """Rays from behind the plane through the centroids of pickets k: back faces, accepted by none."""
    return _rays(BEHIND, centroid(n, np.asarray(k)))


def _put(rays, lane, ray):
    o, d = (a.copy() for a in rays)
    o[lane], d[lane] = ray[0][0], ray[1][0]
    return o, d


def _cat(*parts):
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def _interleave(n, occluded_lanes, count):
    """count rays: the lanes of occluded_lanes aimed at pickets of group 0, the others through gaps."""
    lanes = np.arange(count)
    o, d = gap(lanes + 50)
    ao, ad = aim(n, lanes % 32)
    sel = np.isin(lanes, occluded_lanes)
    o[sel], d[sel] = ao[sel], ad[sel]
    return o, d


def e_group(n, j):
    """Chunk (e): the group of lane j's only occluder."""
    return np.minimum((39 * np.asarray(j)) // 64, S.n_groups(n) - 1)


def chunks(n):
    """{name: (o, d, claim)} of the exit-logic chunks on pickets(n); claim[i] is
    the only triangle that accepts ray i, or -1 for none (what the premises test
    checks by a full scan).  64-ray chunks a, b, c, d, e0, e1 and the ragged
    f33a, f33b (33 rays), f1a, f1b (1 ray)."""
    j = np.arange(64)
    last = n - 1
    out = {}
    a = aim(n, j % 32)
    out["a"] = (*a, j % 32)                                       # all occluded by group 0
    cl = (j % 32).copy()
    cl[17] = last
    out["b"] = (*_put(a, 17, aim(n, [last])), cl)                 # lane 17 only by the scene's last triangle
    cl = (j % 32).copy()
    cl[17] = -1
    out["c"] = (*_put(a, 17, gap([17])), cl)                      # lane 17 unoccluded
    o, d = gap(j)
    bo, bd = behind(n, j * 19 % n)
    o[1::2], d[1::2] = bo[1::2], bd[1::2]
    out["d"] = (o, d, np.full(64, -1))                            # none occluded: gaps and back faces
    g = e_group(n, j)
    out["e0"] = (*aim(n, 32 * g), 32 * g)                         # lane j's only occluder opens its group ...
    k1 = np.minimum(32 * g + 31, last)
    out["e1"] = (*aim(n, k1), k1)                                 # ... or closes it
    # ragged chunks: the first ray (the one padding lanes carry) occluded, by the last triangle, while others are not
    lanes = np.arange(33)
    f = _put(_interleave(n, lanes[lanes % 3 == 1], 33), 0, aim(n, [last]))
    cl = np.where(lanes % 3 == 1, lanes % 32, -1)
    cl[0] = last
    out["f33a"] = (*f, cl)
    f = _interleave(n, lanes[lanes % 3 != 0], 33)                 # ... and the converse: ray 0 is not, others are
    out["f33b"] = (*f, np.where(lanes % 3 != 0, lanes % 32, -1))
    out["f1a"] = (*aim(n, [last]), np.array([last]))
    out["f1b"] = (*gap([7]), np.array([-1]))
    return out


FULL = ("a", "b", "c", "d", "e0", "e1")
RAGGED = ("f33a", "f33b", "f1a", "f1b")


def fan_rays(order):
    """97 rays from around the camera toward random points of the soups' box,
    which every triangle of the fan covers (trace_rays_lib's own fan rays also
    graze the fan or start inside the box and leave without meeting it)."""
    rng = np.random.default_rng(31 + len(order))
    cam = np.asarray(S.CAMERA) + rng.uniform(-0.5, 0.5, (97, 3))
    d = rng.uniform(T.BOX_LO, T.BOX_HI, (97, 3)) - cam
    return cam.astype(F32), (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)


def accepting_sets(oraclemod, tris, o, d):
    """Per ray the list of triangles whose rayTriangleIntersect accepts it (no
    bound), by a full scan with the oracle's own function; equal rays are
    scanned once.  At most MAX_SCAN_PAIRS pairs."""
    f = oraclemod.lib().oracle_ray_triangle
    tris = np.ascontiguousarray(tris)
    rays = np.ascontiguousarray(np.concatenate([o, d], 1), dtype=F32)
    uniq, inv = np.unique(rays.view(np.dtype((np.void, 24))).ravel(), return_inverse=True)
    uniq = np.ascontiguousarray(uniq.view(F32).reshape(-1, 6))
    assert len(uniq) * len(tris) <= MAX_SCAN_PAIRS, f"{len(uniq)} rays x {len(tris)} triangles"
    out = C.c_float()
    pout = C.addressof(out)
    addr = [tris.ctypes.data + 80 * t for t in range(len(tris))]
    sets = []
    for i in range(len(uniq)):
        po = uniq.ctypes.data + 24 * i
        sets.append([t for t in range(len(tris)) if f(po, po + 12, addr[t], pout)])
    return [sets[k] for k in inv.ravel()]


def occluded_ref(oraclemod, tris, o, d, tmax=None, mode="brute", nodes=None):
    """The reference: oracle.closest_hits(...)[1] >= 0, with its dst, tests and visits."""
    bound = None if tmax is None else T.bound_of(np.broadcast_to(np.asarray(tmax, F32), (len(o),)))
    dst, tri, tests, visits = oraclemod.closest_hits(tris, o, d, bound, mode, nodes)
    return tri >= 0, dst, tests, visits


def bound_cases(dst, hit):
    """[(name, tmax, expected)] of the bounded cases on rays whose unbounded
    closest distance is dst (hit: it exists)."""
    n = len(dst)
    none = np.zeros(n, bool)
    cases = [("tmax = dst", np.where(hit, dst, F32(0)).astype(F32), none),
             ("tmax = nextafter(dst)", np.where(hit, np.nextafter(dst, F32(np.inf)), F32(0)).astype(F32), hit),
             ("tmax = dst / 2", np.where(hit, dst * F32(0.5), F32(0)).astype(F32), none)]
    for v in (0.0, -1.0, np.nan, np.inf, 2e38):
        with np.errstate(over="ignore"):
            cases.append((f"tmax = {v}", np.full(n, v).astype(F32), hit))  # the unbounded encodings
    return cases
