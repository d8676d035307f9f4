"""Scenes, rays and references for the preview shading query tests.

Host half of tests/test_gpu_shade.py (needs the GPU); its premises are checked
on the CPU oracle alone by tests/test_shade_cpu.py.  numpy, the oracle and the
package's host-side scene builders only.

The reference of a ray is the oracle's traceBasic through a one-pixel camera:
width = height = 2, basicShading = 1, cameraPos = o, viewportFront = f,
viewportRight = viewportUp = 0.  Pixel (1, 1) has px = py = 0, so
oracle.render_pixels(..., [1], [1]) returns traceBasic's colour and segment
count for Ray(o, normalize(f)).  A ray set is therefore a list of (o, f); the
GPU tests take d from rt2_camera_rays_host for the same uniforms.

walk() follows the same rays segment by segment with oracle.closest_hits and
binary32 numpy arithmetic and names what happened on the way (the branch of
traceBasic's switch at every hit and how the ray ended).  It is used for the
coverage conditions only, never as a reference for colours; that it follows
the oracle's paths is itself asserted (its segment counts are the oracle's).
"""
import numpy as np

import closest_hit_scenes as S
import shading_scenes as ss
import surface_model as M
import trace_rays_lib as T

F32 = np.float32
GLASS_HIGHLIGHT, UNKNOWN = 6, 9
RAY_COUNTS = (1, 63, 64, 65, 1025)
SETTINGS = [(shadow, mb) for shadow in (0, 1) for mb in (1, 3, 8)]

BRANCHES = ("sky after 1 segment", "sky after 2 or more segments", "diffuse", "checker white", "checker black",
            "texture", "light above 1", "light at most 1", "glass entered and left", "glass total internal reflection",
            "highlight pass-through", "unknown type", "bounce limit inside a mirror pair", "diffuse end, shadow ray occluded",
            "diffuse end, shadow ray free")


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


# ---- the oracle through one-pixel cameras ----------------------------------------------------------------------

def one_pixel_uniforms(rt2mod, o, f, n_tris, light, shadow, max_bounce, num_textures):
    u = rt2mod.Uniforms()
    u.width = u.height = 2
    u.basicShading, u.numRaysPerPixel, u.environmentalLight = 1, 1, 1
    u.numTriangles, u.numTextures = int(n_tris), int(num_textures)
    u.basicShadingShadow, u.maxBounceCount = int(shadow), int(max_bounce)
    u.basicShadingLightPosition = rt2mod.Vec4(float(light[0]), float(light[1]), float(light[2]), 1.0)
    u.cameraPos = rt2mod.Vec4(float(o[0]), float(o[1]), float(o[2]), 0.0)
    u.viewportFront = rt2mod.Vec4(float(f[0]), float(f[1]), float(f[2]), 0.0)
    return u


_refs = {}


def oracle_shade(oraclemod, rt2mod, sc, shadow, max_bounce, mode="brute", tris=None, nodes=None):
    """(rgb float32 [n, 3], segments int32 [n]) of the scene's rays, once per
    scene, setting and array; read-only.  tris / nodes: the BVH's arrays."""
    key = (sc["name"], int(shadow), int(max_bounce), mode)
    if key not in _refs:
        tri = sc["triangles"] if tris is None else tris
        n = len(sc["o"])
        rgb, segs = np.zeros((n, 3), F32), np.zeros(n, np.int32)
        oraclemod.set_textures(sc["textures"])
        try:
            for i in range(n):
                u = one_pixel_uniforms(rt2mod, sc["o"][i], sc["f"][i], len(tri), sc["light"], shadow, max_bounce,
                                       len(sc["textures"]))
                acc, _, s, _ = oraclemod.render_pixels(tri, sc["materials"], u, [1], [1], 0, 1, mode, nodes, threads=1)
                rgb[i], segs[i] = acc[0, :3], s
        finally:
            oraclemod.set_textures([])
        rgb.setflags(write=False)
        segs.setflags(write=False)
        _refs[key] = (rgb, segs)
    return _refs[key]


def oracle_shade_rays(oraclemod, rt2mod, sc, o, f, shadow, max_bounce):
    """The same for rays that are not the scene's own (not kept)."""
    tmp = dict(sc, o=np.asarray(o, F32), f=np.asarray(f, F32), name=None)
    key = (None, int(shadow), int(max_bounce), "brute")
    _refs.pop(key, None)
    out = oracle_shade(oraclemod, rt2mod, tmp, shadow, max_bounce)
    _refs.pop(key, None)
    return out


# ---- the walk: which branches a ray takes ----------------------------------------------------------------------

def walk(oraclemod, sc, max_bounce, shadow=1):
    """Per ray: (events, segments).  events is a list of branch names in the
    order traceBasic meets them."""
    tris, mats = sc["triangles"], sc["materials"]
    n = len(sc["o"])
    o = sc["o"].astype(F32).copy()
    d = _unit(sc["f"]).astype(F32)
    events = [[] for _ in range(n)]
    segs = np.zeros(n, np.int64)
    inside = np.zeros(n, bool)
    entered = np.zeros(n, bool)
    mirrors = np.zeros(n, np.int64)  # consecutive mirror hits
    live = np.ones(n, bool)
    light = np.asarray(sc["light"], F32)
    for bounce in range(1, max_bounce + 1):
        idx = np.flatnonzero(live)
        if not len(idx):
            break
        dst, tri, _, _ = oraclemod.closest_hits(tris, o[idx], d[idx])
        for k, i in enumerate(idx):
            segs[i] += 1
            t = int(tri[k])
            if t < 0:
                events[i].append(BRANCHES[0] if bounce == 1 else BRANCHES[1])
                live[i] = False
                continue
            a, b, c = (tris[x][t, :3].astype(F32) for x in "abc")
            nrm = np.cross(b - a, c - a).astype(F32)
            nrm = (nrm / np.sqrt((nrm * nrm).sum(dtype=F32))).astype(F32)
            hit = (o[i] + d[i] * dst[k]).astype(F32)
            m = mats[tris["materialIndex"][t]]
            kind = int(m["materialType"])
            o[i] = (hit - nrm * F32(1e-4)).astype(F32)
            if kind != ss.SPECULAR:
                mirrors[i] = 0
            if kind == ss.SPECULAR:
                mirrors[i] += 1
                d[i] = (d[i] - nrm * (F32(2) * (nrm * d[i]).sum(dtype=F32))).astype(F32)
                if bounce == max_bounce and mirrors[i] >= 2:
                    events[i].append(BRANCHES[12])
            elif kind in (ss.DIFFUSE, ss.CHECKER, ss.TEXTURE):
                if kind == ss.DIFFUSE:
                    events[i].append("diffuse")
                elif kind == ss.TEXTURE:
                    events[i].append("texture")
                else:
                    s = F32(m["checkerScale"])
                    black = False
                    if s > 0:
                        q = np.floor(o[i] * s).sum(dtype=F32)
                        black = q - F32(2) * np.floor(q / F32(2)) == 0
                    events[i].append("checker black" if black else "checker white")
                if shadow:
                    segs[i] += 1
                    to_light = _unit(light - hit).astype(F32)
                    _, st, _, _ = oraclemod.closest_hits(tris, o[i][None], to_light[None])
                    if kind == ss.DIFFUSE:
                        events[i].append(BRANCHES[13] if st[0] >= 0 else BRANCHES[14])
                live[i] = False
            elif kind == ss.LIGHT:
                events[i].append("light above 1" if m["emissionColor"][:3].max() > 1 else "light at most 1")
                live[i] = False
            elif kind == ss.GLASS:
                eta = F32(m["refractiveIndex"]) if inside[i] else F32(1) / F32(m["refractiveIndex"])
                ni = (nrm * d[i]).sum(dtype=F32)
                kk = F32(1) - eta * eta * (F32(1) - ni * ni)
                if kk < 0:
                    d[i] = (d[i] - nrm * (F32(2) * ni)).astype(F32)
                    if inside[i]:
                        events[i].append(BRANCHES[9])
                else:
                    d[i] = (eta * d[i] - (eta * ni + np.sqrt(kk, dtype=F32)) * nrm).astype(F32)
                    if inside[i] and entered[i]:
                        events[i].append(BRANCHES[8])
                    entered[i] = True
                    inside[i] = not inside[i]
            elif kind == GLASS_HIGHLIGHT:
                events[i].append(BRANCHES[10])
            else:
                events[i].append(BRANCHES[11])
                live[i] = False
    return events, segs


# ---- materials of every kind ------------------------------------------------------------------------------------

def every_material(n, seed=23):
    """n materials cycling through every branch of traceBasic's switch."""
    rng = np.random.default_rng(seed)
    kinds = (ss.DIFFUSE, ss.SPECULAR, ss.LIGHT, ss.CHECKER, ss.GLASS, ss.TEXTURE, GLASS_HIGHLIGHT, UNKNOWN, ss.DIFFUSE,
             ss.LIGHT, ss.SPECULAR)
    m = np.zeros(n, ss.MAT_DTYPE)
    i = np.arange(n)
    m["materialType"] = np.array(kinds)[i % len(kinds)]
    m["color"][:, :3] = rng.uniform(0.05, 1.0, (n, 3))
    m["color"][:, 3] = 1.0
    m["specularColor"][:] = 1.0
    m["emissionColor"][:, :3] = rng.uniform(0.05, 1.0, (n, 3)) * np.where(i % len(kinds) == 9, 3.0, 1.0)[:, None]
    m["emissionStrength"] = 1.0
    m["smoothness"] = m["specularProbability"] = 1.0
    m["checkerScale"] = 1.7
    m["refractiveIndex"] = 1.5
    m["textureIndex"] = i // len(kinds) % 3  # 0, 1: the two images; 2: a unit without one
    m["index"] = i
    return m


def textures():
    """A 3-channel and a 1-channel image."""
    rng = np.random.default_rng(5)
    return [ss._textures()[0], rng.integers(30, 256, (4, 5, 1), dtype=np.uint8)]


def _finish(name, tris, mats, o, f, light, tex=()):
    sc = dict(name=name, triangles=np.ascontiguousarray(tris), materials=np.ascontiguousarray(mats),
              o=np.ascontiguousarray(o, F32), f=np.ascontiguousarray(f, F32), light=tuple(map(float, light)),
              textures=list(tex))
    assert len(sc["o"]) == len(sc["f"])
    for k in ("triangles", "materials", "o", "f"):
        sc[k].setflags(write=False)
    return sc


_scenes = {}


def _cached(fn):
    def get(*a):
        key = (fn.__name__,) + a
        if key not in _scenes:
            _scenes[key] = fn(*a)
        return _scenes[key]
    return get


# ---- 1 triangle, and the soups with hits in the group read from L2 --------------------------------------------

@_cached
def soup(n):
    """trace_rays_lib's soup of n triangles, each with a material of its own
    cycling through every type, with the rays of surface_model.hit_scene_rays
    (on 1,217 triangles rays 40 .. 47 aim at triangle 1,216, in the group read
    from L2).  Texture coordinates are a function of the index."""
    tris = T.scene_tris("soup", n).copy()
    k = np.arange(n)
    tris["aTex"] = np.stack([0.1 * (k % 7), 0.2 * (k % 3)], 1)
    tris["bTex"] = tris["aTex"] + (1.3, 0.1)
    tris["cTex"] = tris["aTex"] + (0.2, 0.9)
    o, d = M.hit_scene_rays("soup", n)
    return _finish(f"soup{n}", tris, every_material(n), o, d, (0.5, 9.0, 12.0), textures())


# ---- the diverse Cornell box with a checker floor, textures, a highlight sheet and an unknown type -----------

def _facing_quad(b, centre, towards, half, mat, uv=None):
    """A square of half-width `half` about `centre`, its front towards the point `towards`."""
    centre, towards = np.asarray(centre, np.float64), np.asarray(towards, np.float64)
    nrm = _unit(towards - centre)
    t1 = _unit(np.cross(nrm, (0.31, 0.87, 0.38)))
    t2 = np.cross(nrm, t1)
    b.quad(centre - half * (t1 + t2), 2 * half * t1, 2 * half * t2, mat, uv)


@_cached
def cornell(rt2mod_id=None):
    import rt2
    Mt = rt2.Material
    sd = rt2.SceneData()
    ids = [sd.add_material(m) for m in (Mt.diffuse((1, 0, 0)), Mt.diffuse((0, 1, 0)), Mt.diffuse((1, 1, 1)),
                                        Mt.light((2, 1.5, 1), 15.0), Mt.glass((0.9, 0.95, 1.0), 1.5),
                                        Mt.specular((1, 1, 1), (1, 1, 1), 1.0, 1.0), Mt.checker(8.0),
                                        Mt.specular((0.8, 0.6, 0.3), (1, 1, 1), 0.7, 0.4))]
    sd.create_diverse_cornell_box(10.0, *ids)
    box_t, box_m = sd.triangles().copy(), sd.materials().copy()
    lo = np.minimum.reduce([box_t[k][:, :3].min(0) for k in "abc"]).astype(np.float64)
    hi = np.maximum.reduce([box_t[k][:, :3].max(0) for k in "abc"]).astype(np.float64)
    ctr, ext = (lo + hi) / 2, (hi - lo).min()
    eye = ctr + np.array((0.013, 0.007, 0.011)) * ext
    b = ss._Builder()
    b.mats = [box_m[i].copy() for i in range(len(box_m))]
    r, h = 0.22 * ext, 0.07 * ext
    wide = [(-0.7, -0.35), (1.9, -0.35), (1.9, 2.6), (-0.7, 2.6)]
    extras = [(b.material(ss.CHECKER, checker=1.7), (0.1, -1.0, 0.2)),           # the checker floor
              (b.material(ss.TEXTURE, texture=0), (1.0, 0.3, 0.2)),             # 3-channel image
              (b.material(ss.TEXTURE, texture=1), (-1.0, 0.3, -0.2)),           # 1-channel image
              (b.material(GLASS_HIGHLIGHT, color=(0.5, 0.5, 0.5)), (0.2, 0.3, 1.0)),
              (b.material(UNKNOWN, color=(0.2, 0.3, 0.4)), (-0.3, 0.9, -0.4)),
              (b.light((0.9, 0.5, 0.2), 0.7), (0.4, 0.2, -1.0))]                # a light with no component above 1
    targets = []
    for mat, direction in extras:
        c = eye + r * _unit(direction)
        _facing_quad(b, c, eye, h, mat, wide)
        targets.append(c)
    tris = np.concatenate([box_t, np.array(b.tris, ss.TRI_DTYPE)])
    mats = np.array(b.mats, ss.MAT_DTYPE)
    rng = np.random.default_rng(17)
    n = 1025
    o = eye + rng.uniform(-0.01, 0.01, (n, 3)) * ext
    f = rng.normal(size=(n, 3))
    aim = np.arange(n) % 3 == 0  # every third ray at one of the added quads
    tg = np.array(targets)[rng.integers(0, len(targets), n)] + rng.uniform(-0.8, 0.8, (n, 3)) * h
    f[aim] = (tg - o)[aim]
    f *= rng.uniform(0.5, 2.0, (n, 1))  # viewportFront need not be of unit length
    light = ctr + np.array((0.0, 0.4, 0.0)) * (hi - lo)
    return _finish("cornell", tris, mats, o, f, light, textures())


# ---- two facing mirrors with diffuse patches at staggered depths ---------------------------------------------

@_cached
def corridor():
    """Mirrors in the planes x = -1 and x = 1 facing each other, y in [-1, 1],
    z from 1 down to -14; on each of them, a hair in front, diffuse patches
    from z = -3 (lower half, y < 0) or z = -4.5 (upper half) down to z = -7,
    and a light patch between z = -9 and -10.  A ray from the axis with
    direction (+-1, y', -s) meets the walls at z = -s (2 k - 1): it ends on a
    patch at a bounce between 1 and 8 that its slope s decides, on the light,
    in the sky beyond the open end, or at the bounce limit between the mirrors.
    The preview light hangs far above the open top; a roof over z in [-5.2, -3.6]
    hides it from the patches below it."""
    b = ss._Builder()
    mirror = b.mirror()
    dif = [b.material(ss.DIFFUSE, color=c) for c in ((0.9, 0.4, 0.2), (0.2, 0.5, 0.9))]
    lit = b.light((2.0, 1.0, 0.5), 3.0)
    roof = b.material(ss.DIFFUSE, color=(0.3, 0.3, 0.3))
    for sx in (-1.0, 1.0):
        def wall(x, y0, y1, z0, z1, mat):
            # front towards the axis: normal (-sx, 0, 0)
            if sx < 0:
                b.quad((x, y0, z0), (0, y1 - y0, 0), (0, 0, z1 - z0), mat)
            else:
                b.quad((x, y0, z0), (0, 0, z1 - z0), (0, y1 - y0, 0), mat)
        wall(sx, -1.0, 1.0, -14.0, 1.0, mirror)
        e = sx * 0.999
        wall(e, -1.0, 0.0, -7.0, -3.0, dif[0])
        wall(e, 0.0, 1.0, -7.0, -4.5, dif[1])
        wall(e, -1.0, 1.0, -10.0, -9.0, lit)
    b.quad((-1.5, 1.5, -5.2), (3.0, 0, 0), (0, 0, 1.6), roof)  # normal (0, -1, 0): faces down
    rng = np.random.default_rng(29)
    n = 4096
    s = np.exp(rng.uniform(np.log(0.15), np.log(6.0), n))
    o = np.stack([rng.uniform(-0.2, 0.2, n), rng.uniform(-0.6, 0.6, n), rng.uniform(0.0, 0.5, n)], 1)
    f = np.stack([rng.choice((-1.0, 1.0), n), rng.uniform(-0.03, 0.03, n), -s], 1)
    sc = b.scene("corridor", 2, 2, 8, 1, True)
    return _finish("corridor", sc["triangles"], sc["materials"], o, f, (0.0, 60.0, -5.0))


def corridor_1025():
    sc = corridor()
    return dict(sc, name="corridor/1025", o=sc["o"][:1025], f=sc["f"][:1025])


ORACLE_SCENES = {"one": lambda: soup(1), "cornell": cornell, "corridor": corridor_1025,
                 "soup1216": lambda: soup(1216), "soup1217": lambda: soup(1217)}


# ---- chunks picked by what the oracle says of the corridor's rays -----------------------------------------------

def corridor_classes(oraclemod, rt2mod, max_bounce=8):
    """Of the corridor's 4,096 rays, by the oracle alone: `ends`, the bounce at
    which a ray ended on a patch (its segment count grows by one with the
    shadow ray on), 0 otherwise; `occluded`, the shadow ray found something
    (the colour is a fifth); `early`, the ray ended on the light or in the sky
    before the bounce limit."""
    sc = corridor()
    rgb0, seg0 = oracle_shade(oraclemod, rt2mod, sc, 0, max_bounce)
    rgb1, seg1 = oracle_shade(oraclemod, rt2mod, sc, 1, max_bounce)
    patch = seg1 == seg0 + 1
    assert ((seg1 == seg0) | patch).all()
    ends = np.where(patch, seg0, 0)
    occluded = patch & (rgb1.view(np.uint32) != rgb0.view(np.uint32)).any(1)
    early = ~patch & (seg0 < max_bounce)
    return ends, occluded, early, seg0


def _take(mask, k, what):
    idx = np.flatnonzero(mask)
    assert len(idx) >= k, f"{what}: {len(idx)} rays, {k} needed"
    return idx[:k]


def shadow_chunks(oraclemod, rt2mod):
    """Indices into the corridor's rays, three chunks of 64: patch ends at
    bounces 1, 2 and 3 with both shadow outcomes in each class, interleaved;
    exactly one ray that ends on a patch; none."""
    ends, occ, early, _ = corridor_classes(oraclemod, rt2mod)
    first = np.concatenate([_take((ends == k) & (occ == bool(v)), 10, f"bounce {k} occluded {v}")
                            for k in (1, 2, 3) for v in (0, 1)] + [_take(early, 4, "early")])
    first = first[np.random.default_rng(3).permutation(64)]
    second = _take(early, 64, "early").copy()
    second[37] = _take(ends == 2, 1, "one patch end")[0]
    third = _take(early, 64, "early")
    return first, second, third


def compaction_chunk(oraclemod, rt2mod):
    """40 rays that end at bounce 1 in lanes 0 .. 39, then 24 that go on."""
    _, _, _, seg0 = corridor_classes(oraclemod, rt2mod)
    return np.concatenate([_take(seg0 == 1, 40, "one segment"), _take(seg0 >= 3, 24, "three or more segments")])
