"""Scenes, rays, seeds and references for the radiance query tests.

Host half of tests/test_gpu_radiance.py (needs the GPU); its premises are
checked on the CPU oracle alone by tests/test_radiance_cpu.py.  numpy, the
oracle and the package's host-side scene builders only.

The reference of a ray is the oracle's trace() through the one-pixel camera of
tests/shade_scenes.py turned to the path tracer: width = height = 2,
basicShading = 0, numRaysPerPixel = R, cameraPos = o, viewportFront = f and the
other six camera vectors zero.  All four pixels then get the same ray (the
defocus disk, the jitter and the viewport's extent are zero), with seeds
p + frame * 968824447 for p = 0 .. 3 (p = x + 2 y).  The multiplier is odd, so
any 32-bit seed is some frame's: frame_for().  oracle.render_pixels(..., frame,
1) returns toSRGB(tonemapACES(sum / R)) and the segment count; the GPU tests
apply oracle_tonemap_srgb to the query's linear colour and compare bits.  A
ray set is therefore a list of (o, f, p, frame).

walk() follows the same rays segment by segment with oracle.closest_hits,
binary32 numpy arithmetic and the generator in Python integers, and names what
happened on the way.  It is used for the coverage conditions only, never as a
reference for colours; that it follows the oracle's paths is itself asserted
(only rays whose segment count is the oracle's are counted).
"""
import ctypes as C

import numpy as np

import random_scenes as rs
import shade_scenes as H
import shading_model as sm
import shading_scenes as ss
import surface_model as M

F32 = np.float32
MULT = 968824447
MULT_INV = pow(MULT, -1, 2 ** 32)
MASK = 0xFFFFFFFF
RAY_COUNTS = (1, 63, 64, 65, 1025)
SETTINGS = [(env, mb) for env in (0, 1) for mb in (1, 3, 8)]
TIE_FREE = ("one", "soup1216", "soup1217")  # random triangles: no two at one distance along a ray

BRANCHES = ("diffuse", "texture", "specular bounce", "specular declined", "checker", "glass refracted",
            "glass total internal reflection", "light", "unknown type", "glass highlight type", "sky",
            "black sky", "pass-through", "roulette kill at bounce 1", "roulette kill at a later bounce",
            "survival below one", "cut at the limit")


# ---- seeds -------------------------------------------------------------------------------------------------------

def frame_for(seed, p):
    """The frame at which pixel p (= x + 2 y) of the one-pixel camera starts from `seed`."""
    return ((int(seed) - int(p)) * MULT_INV) & MASK


def seed_of(p, frame):
    return (np.asarray(p, np.uint64) + np.asarray(frame, np.uint64) * np.uint64(MULT)).astype(np.uint64) & np.uint64(MASK)


def pcg_next(state):
    """random(), compute.glsl:148-154, on Python integers -> (state, binary32 value)."""
    state = (state * 747796405 + 2891336453) & MASK
    r = (((state >> ((state >> 28) + 4)) ^ state) * 277803737) & MASK
    r = (r >> 22) ^ r
    return state, F32(r) / F32(4294967296.0)


def advance(seed, draws):
    s = int(seed)
    for _ in range(int(draws)):
        s = (s * 747796405 + 2891336453) & MASK
    return s


def default_seeds(n, key):
    """(p, frame) of n rays: pixel i % 4; the first four are seed 0, seed
    0xFFFFFFFF, frame 5 (5 * 968824447 is past 2^32) and the last frame; the
    others random 32-bit frames, nearly all of which wrap."""
    rng = np.random.default_rng(key)
    p = np.arange(n) % 4
    frame = rng.integers(0, 2 ** 32, n, dtype=np.uint64)
    special = [frame_for(0, 0), frame_for(0xFFFFFFFF, 1), 5, 0xFFFFFFFF]
    frame[:min(n, 4)] = special[:n]
    return p.astype(np.int64), frame


# ---- the oracle through one-pixel cameras -----------------------------------------------------------------------

def one_pixel_uniforms(rt2mod, o, f, n_tris, env, max_bounce, num_textures, rays=1):
    u = rt2mod.Uniforms()
    u.width = u.height = 2
    u.basicShading, u.numRaysPerPixel, u.environmentalLight = 0, int(rays), int(env)
    u.numTriangles, u.numTextures = int(n_tris), int(num_textures)
    u.maxBounceCount = int(max_bounce)
    u.cameraPos = rt2mod.Vec4(float(o[0]), float(o[1]), float(o[2]), 0.0)
    u.viewportFront = rt2mod.Vec4(float(f[0]), float(f[1]), float(f[2]), 0.0)
    return u


def tonemap(oraclemod, linear):
    """oracle_tonemap_srgb per channel of a float32 array."""
    fn = oraclemod.lib().oracle_tonemap_srgb
    flat = np.ascontiguousarray(linear, F32).reshape(-1)
    return np.array([fn(C.c_float(float(x))) for x in flat], F32).reshape(np.shape(linear))


_refs = {}


def oracle_radiance(oraclemod, rt2mod, sc, env, max_bounce, mode="brute", tris=None, nodes=None, rays=1):
    """(toSRGB(tonemapACES(sum / rays)) float32 [n, 3], segments int32 [n]) of
    the scene's rays, once per scene, setting and array; read-only.  tris /
    nodes: the BVH's arrays."""
    key = (sc["name"], int(env), int(max_bounce), mode, int(rays))
    if key not in _refs:
        tri = sc["triangles"] if tris is None else tris
        n = len(sc["o"])
        rgb, segs = np.zeros((n, 3), F32), np.zeros(n, np.int32)
        oraclemod.set_textures(sc["textures"])
        try:
            for i in range(n):
                u = one_pixel_uniforms(rt2mod, sc["o"][i], sc["f"][i], len(tri), env, max_bounce, len(sc["textures"]),
                                       rays)
                p = int(sc["p"][i])
                acc, _, s, _ = oraclemod.render_pixels(tri, sc["materials"], u, [p % 2], [p // 2], int(sc["frame"][i]),
                                                       1, mode, nodes, threads=1)
                rgb[i], segs[i] = acc[0, :3], s
        finally:
            oraclemod.set_textures([])
        rgb.setflags(write=False)
        segs.setflags(write=False)
        _refs[key] = (rgb, segs)
    return _refs[key]


# ---- scenes -------------------------------------------------------------------------------------------------------

_scenes = {}


def _rays_of(sc, name, key, mats=None):
    n = len(sc["o"])
    p, frame = default_seeds(n, key)
    out = dict(sc, name=name, p=p, frame=frame)
    if mats is not None:
        out["materials"] = mats
    for k in ("p", "frame", "materials"):
        out[k].setflags(write=False)
    return out


def soup(n):
    if ("soup", n) not in _scenes:
        _scenes["soup", n] = _rays_of(H.soup(n), f"rad_soup{n}", 100 + n)
    return _scenes["soup", n]


def cornell():
    """shade_scenes' diverse Cornell box (every material type, a 3-channel and
    a 1-channel texture, a highlight-type sheet, an unknown type and a dim
    light) with its ceiling light dimmed to strength 2, so that a path that
    ends on it stays below the tonemap's ceiling in two channels, and the green
    wall marked isEdgeHighlight: a path that meets it after its first bounce
    passes through to the sky."""
    if "cornell" not in _scenes:
        sc = H.cornell()
        mats = sc["materials"].copy()
        assert mats["materialType"][3] == ss.LIGHT and mats["materialType"][1] == ss.DIFFUSE
        mats["emissionStrength"][3] = 2.0
        mats["isEdgeHighlight"][1] = 1
        _scenes["cornell"] = _rays_of(sc, "rad_cornell", 7, mats)
    return _scenes["cornell"]


def corridor():
    """The facing mirrors: lanes end at different bounces (a patch's roulette, the light, the open end)."""
    if "corridor" not in _scenes:
        _scenes["corridor"] = _rays_of(H.corridor_1025(), "rad_corridor", 11)
    return _scenes["corridor"]


ORACLE_SCENES = {"one": lambda: soup(1), "cornell": cornell, "corridor": corridor, "soup1216": lambda: soup(1216),
                 "soup1217": lambda: soup(1217)}


def picked(sc, idx, name):
    idx = np.asarray(idx)
    return dict(sc, name=name, o=sc["o"][idx], f=sc["f"][idx], p=sc["p"][idx], frame=sc["frame"][idx])


# ---- the frames at which a draw is exactly 1.0, on their scenes ---------------------------------------------------

def draw_is_one_rays():
    """name -> (scene, which): the pixel of random_scenes' DRAW_IS_ONE,
    PROBABILITY_IS_ONE and ROULETTE_IS_ONE frames as a ray of the one-pixel
    camera with that pixel's seed: o = cameraPos, f = the pixel's end point
    less cameraPos, in binary32."""
    out = {}
    for name, which, scene in (("draw_is_one", rs.DRAW_IS_ONE, rs.draw_is_one()),
                               ("probability_is_one", rs.PROBABILITY_IS_ONE,
                                rs.mirror_floor(rs.PROBABILITY_IS_ONE, "probability_is_one")),
                               ("roulette_is_one", rs.ROULETTE_IS_ONE,
                                rs.mirror_floor(rs.ROULETTE_IS_ONE, "roulette_is_one"))):
        un = scene["uniforms"]
        W, Hh = un["width"], un["height"]
        v = {k: np.array(un[k], F32) for k in ("cameraPos", "viewportFront", "viewportRight", "viewportUp")}
        px, py = F32(which["x"] * 2 - W) / F32(W), F32(which["y"] * 2 - Hh) / F32(Hh)
        f = (v["viewportFront"] + v["viewportRight"] * px + v["viewportUp"] * py).astype(F32)
        seed = (which["x"] + which["y"] * W + which["frame"] * MULT) & MASK
        p = 2
        out[name] = (dict(name=f"rad_{name}", triangles=scene["triangles"], materials=scene["materials"],
                          o=v["cameraPos"][None].astype(F32), f=f[None], p=np.array([p]),
                          frame=np.array([frame_for(seed, p)], np.uint64), textures=[],
                          max_bounce=un["maxBounceCount"], seed=seed), which)
    return out


# ---- the walk: which branches a path takes -------------------------------------------------------------------------

def _unit32(v):
    v = np.asarray(v, F32)
    return (v / np.sqrt((v * v).sum(dtype=F32))).astype(F32)


def _rnd_dir(state):
    for _ in range(100):
        state, x = pcg_next(state)
        state, y = pcg_next(state)
        state, z = pcg_next(state)
        v = np.array([x * F32(2) - F32(1), y * F32(2) - F32(1), z * F32(2) - F32(1)], F32)
        s = (v * v).sum(dtype=F32)
        if s < 1:
            return state, (v / np.sqrt(s)).astype(F32)
    return state, np.zeros(3, F32)


def _texture(sc, texels, m, t, o, d):
    k = int(m["textureIndex"])
    if k < 0 or k >= len(texels):
        return np.zeros(3, F32)
    if k > 4:
        return np.array([1, 0, 1], F32)
    u, v, _ = M.barycentrics(sc["triangles"], np.array([t]), o[None], d[None])
    w = 1.0 - u - v
    tri = sc["triangles"]
    uv = tri["aTex"][t] * u + tri["bTex"][t] * v + tri["cTex"][t] * w
    rgb = sm.sample_linear_repeat(texels[k], uv[:1], uv[1:])[0]
    return rgb[0].astype(F32)


def walk(oraclemod, sc, env, max_bounce):
    """Per ray: (events, segments, state after the last draw).  The ray and the
    state after the camera's three draws are those of the one-pixel camera."""
    tris, mats = sc["triangles"], sc["materials"]
    texels = [sm.gl_texels(t) for t in sc["textures"]]
    n = len(sc["o"])
    o = sc["o"].astype(F32).copy()
    d = np.stack([_unit32((sc["o"][i] + sc["f"][i]).astype(F32) - sc["o"][i]) for i in range(n)])
    state = [advance(s, 3) for s in seed_of(sc["p"], sc["frame"])]
    colour = np.ones((n, 3), F32)
    inside = np.zeros(n, bool)
    events = [[] for _ in range(n)]
    segs = np.zeros(n, np.int64)
    live = np.ones(n, bool)
    nrm_all = np.stack([_unit32(np.cross((tris["b"][t, :3] - tris["a"][t, :3]).astype(F32),
                                         (tris["c"][t, :3] - tris["a"][t, :3]).astype(F32)).astype(F32))
                        for t in range(len(tris))]) if len(tris) else np.zeros((0, 3), F32)
    for bounce in range(1, max_bounce + 1):
        idx = np.flatnonzero(live)
        if not len(idx):
            break
        with np.errstate(all="ignore"):
            dst, tri, _, _ = oraclemod.closest_hits(tris, o[idx], d[idx])
        for k, i in enumerate(idx):
            segs[i] += 1
            t = int(tri[k])
            if t < 0:
                events[i].append("sky" if env else "black sky")
                live[i] = False
                continue
            nrm = nrm_all[t]
            step = (d[i] * dst[k]).astype(F32)
            hit = (o[i] + step).astype(F32)
            m = mats[tris["materialIndex"][t]]
            kind = int(m["materialType"])
            tex = _texture(sc, texels, m, t, o[i], d[i]) if kind == ss.TEXTURE else None
            back = (step * F32(-1e-3)).astype(F32)
            o[i] = (hit + back if kind == ss.GLASS else hit - back).astype(F32)
            prev = d[i].copy()
            if kind in (ss.DIFFUSE, ss.TEXTURE, ss.CHECKER):
                state[i], r = _rnd_dir(state[i])
                d[i] = _unit32(nrm + r)
                if kind == ss.DIFFUSE:
                    atten = m["color"][:3].astype(F32)
                    events[i].append("diffuse")
                elif kind == ss.TEXTURE:
                    atten = tex
                    events[i].append("texture")
                else:
                    s = F32(m["checkerScale"])
                    black = False
                    if s > 0:
                        q = np.floor(o[i] * s).sum(dtype=F32)
                        black = q - F32(2) * np.floor(q / F32(2)) == 0
                    atten = np.zeros(3, F32) if black else np.ones(3, F32)
                    events[i].append("checker")
            elif kind == ss.SPECULAR:
                state[i], r = _rnd_dir(state[i])
                diffuse = _unit32(nrm + r)
                spec = (d[i] - nrm * (F32(2) * (nrm * d[i]).sum(dtype=F32))).astype(F32)
                state[i], x = pcg_next(state[i])
                is_spec = F32(m["specularProbability"]) > x
                a = F32(m["smoothness"]) if is_spec else F32(0)
                d[i] = (diffuse * (F32(1) - a) + spec * a).astype(F32)
                atten = np.ones(3, F32) if is_spec else m["color"][:3].astype(F32)
                events[i].append("specular bounce" if is_spec else "specular declined")
            elif kind == ss.LIGHT:
                events[i].append("light")
                live[i] = False
                continue
            elif kind == ss.GLASS:
                eta = F32(m["refractiveIndex"]) if inside[i] else F32(1) / F32(m["refractiveIndex"])
                ni = (nrm * d[i]).sum(dtype=F32)
                kk = F32(1) - eta * eta * (F32(1) - ni * ni)
                if kk < 0:
                    d[i] = (d[i] - nrm * (F32(2) * ni)).astype(F32)
                    events[i].append("glass total internal reflection")
                else:
                    d[i] = (eta * d[i] - (eta * ni + np.sqrt(kk, dtype=F32)) * nrm).astype(F32)
                    inside[i] = not inside[i]
                    events[i].append("glass refracted")
                atten = m["color"][:3].astype(F32)
            else:
                events[i].append("glass highlight type" if kind == H.GLASS_HIGHLIGHT else "unknown type")
                live[i] = False
                continue
            if m["isEdgeHighlight"] and bounce > 1:
                d[i] = prev
                events[i].append("pass-through")
            else:
                colour[i] = (colour[i] * atten).astype(F32)
            pr = colour[i].max()
            state[i], x = pcg_next(state[i])
            if x > pr:
                events[i].append("roulette kill at bounce 1" if bounce == 1 else "roulette kill at a later bounce")
                live[i] = False
                continue
            if pr < 1:
                events[i].append("survival below one")
            with np.errstate(all="ignore"):
                colour[i] = (colour[i] * (F32(1) / pr)).astype(F32)
            if bounce >= max_bounce:
                events[i].append("cut at the limit")
                live[i] = False
    return events, segs, np.array(state, np.uint64)


# ---- chunks picked by the oracle's segment counts -----------------------------------------------------------------

def _take(mask, k, what):
    idx = np.flatnonzero(mask)
    assert len(idx) >= k, f"{what}: {len(idx)} rays, {k} needed"
    return idx[:k]


def compaction_chunks(oraclemod, rt2mod):
    """Indices into the Cornell box's rays at max_bounce = 8 with the sky on:
    (40 paths that end at bounce 1 in lanes 0 .. 39, then 24 that go on to a
    third bounce at least; 63 paths that end at bounce 1 around one in lane 37
    that goes on)."""
    _, segs = oracle_radiance(oraclemod, rt2mod, cornell(), 1, 8)
    first = np.concatenate([_take(segs == 1, 40, "one segment"), _take(segs >= 3, 24, "three or more segments")])
    second = _take(segs == 1, 64, "one segment").copy()
    second[37] = _take(segs >= 3, 25, "three or more segments")[24]
    return first, second


# ---- whole views --------------------------------------------------------------------------------------------------

VIEW_SIZES = ((67, 10), (64, 4))
VIEW_SCENES = {"diffuse_floor": lambda: rs.diffuse_floor(2), "specular_mix": rs.specular_mix,
               "glass_tinted": rs.glass_tinted, "open_box": rs.open_box, "jitter_defocus_ramp": rs.jitter_defocus_ramp}
VIEW_RAYS = (1, 3)
VIEW_FRAMES = (5, 2)  # first frame 5 (its term wraps 2^32), two frames

_views = {}


def view(name, w, h, rays):
    """The random_scenes scene as a w x h view with `rays` rays per pixel over
    VIEW_FRAMES (the viewport, the jitter and the disk are the scene's own)."""
    key = (name, w, h, rays)
    if key not in _views:
        s = VIEW_SCENES[name]()
        un = dict(s["uniforms"], width=w, height=h, numRaysPerPixel=rays)
        _views[key] = dict(s, name=f"rad_view/{name}/{w}x{h}/r{rays}", uniforms=un, frames=VIEW_FRAMES)
    return _views[key]
