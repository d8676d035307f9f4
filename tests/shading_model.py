"""An independent float64 model of the shader's per-sample path, for scenes
whose paths do not depend on the random numbers.

TEST INFRASTRUCTURE ONLY.  Written from compute.glsl (rayTriangleIntersect
:302-340, getTriangleTextureColor :342-368, trace :472-563,
getEnvironmentalLight :216-273, tonemapACES/toSRGB :647-658, main :660-701)
and, for textures, from GL 4.3 §8.14.2 (GL_LINEAR, GL_REPEAT) and the upload in
textureClass.cpp:65-101 (stb rows flipped on load, so memory row 0 is t = 0;
glTexImage2D with the default GL_UNPACK_ALIGNMENT 4; GL_RED swizzled to
r,r,r; GL_RG read as r,g,0).  It shares no code and no arithmetic with
oracle/rt_oracle.c, the product package or include/rt2_pinned_math.h: plain
numpy float64 and numpy's transcendentals.  Only numpy is imported.

What makes a path deterministic: pixelRight, pixelUp and the defocus disk are
zero, so the R rays of a pixel start alike, and
  - mirrors have specularProbability 1 and smoothness 1;
  - after every bounce max(rayColor) is 1 (the path survives `random > p`
    whatever the number) or exactly 0 (it ends, unless the number is exactly
    0: 2^-32 per draw);
  - a diffuse, checker or texture hit scatters into a random direction, so
    its next segment must end on one uniform emitter whatever the direction:
    the model checks that every triangle the scattered ray could meet (front
    towards the offset origin, partly inside the scatter hemisphere) is a light
    of one emission, and that sample directions over the hemisphere all hit.
Anything else raises NotDeterministic.  One-channel textures (their texels
cannot keep max(rayColor) at 1 next to the r,r,r swizzle unless they are 255
throughout), partial specular probability, survival below 1 and the diffuse
scatter cannot be made deterministic and are not approximated here:
tests/random_path_model.py follows them with the shader's own draws
(tests/test_random_paths.py, tests/test_gpu_random_paths.py).  One-channel
textures stay with the bit-exact oracle tests.

Comparison rule (assert_image): f32 and f64 may decide differently on a pixel
that straddles an edge, a texel boundary or a checker line, and a value near a
texel gradient is ill-conditioned by the texture's width.  Each pixel is
therefore evaluated at its direction and at four directions moved by +-DELTA
(in units of the viewport half-width / half-height) along the two viewport
axes.  A pixel whose five signatures differ is excluded; for the others the
bound is 2e-6 + max |value(moved) - value|.  2e-6 is the bound of
tests/test_oracle_kat.py for tonemap + sRGB.
"""
import math

import numpy as np

DIFFUSE, SPECULAR, LIGHT, CHECKER, GLASS, TEXTURE = 0, 1, 2, 3, 4, 5

# DELTA: the smallest power of two at which the CPU oracle passes every scene
# of shading_scenes.py under the rule above.  Only `textures` needs it: its
# quad with UVs around 1000 carries f32 errors of about 1e-4 texel, and at
# 2^-18 three of its pixels miss, the worst at 1.58 times its bound; every other
# scene passes from 2^-24 on.  The ceiling is 2^-16: above it the bracket would
# start to hide half-texel errors.  Measured at 2^-17, oracle against model (max
# error over the compared pixels / excluded pixels): sky_* 2.5e-7 / <= 0.49 %,
# emissive_ramp 8.6e-8 / 0.52 %, mirror_sky 2.7e-7 / 0.03 %, periscope 2.0e-7 /
# 1.27 %, edge_highlight_* 1.3e-7 / <= 0.52 %, glass_* 1.4e-7 / 0, checker
# 4.3e-8 / <= 0.03 %, textures 2.7e-4 (bound there 6.3e-4) / 0.42 %, composite
# 1.6e-6 / 0.  The full table is in DESIGN.md "Shading model".
DELTA = 2.0 ** -17
DELTA_MAX = 2.0 ** -16
BASE_BOUND = 2e-6
assert DELTA <= DELTA_MAX

# signature fields, one row per bounce
(F_TRI, F_BRANCH, F_REFRACTED, F_INSIDE, F_CHECKER, F_I0, F_J0, F_TEXRULE, F_SUNSIDE, F_BELOW, F_END, F_FU, F_FV,
 F_TEX) = range(14)
NF = 14
TRI_NOT_REACHED, TRI_MISS, TRI_EMITTER = -2, -1, -3
BR_SKY, BR_DARK, BR_PASS = 7, 8, 9           # F_BRANCH besides the material types
CH_WHITE, CH_BLACK, CH_GUARD = 0, 1, 2       # F_CHECKER
TR_SAMPLED, TR_NEGATIVE, TR_BEYOND, TR_MAGENTA, TR_UNBOUND = 0, 1, 2, 3, 4  # F_TEXRULE
END_LIGHT, END_SKY, END_DARK, END_CUT, END_SCATTER, END_ABSORBED, END_BADTYPE = 1, 2, 3, 4, 5, 6, 7


class NotDeterministic(Exception):
    """The scene lets a random number change a pixel."""


def _dot(a, b):
    return (a * b).sum(-1)


def _unit(v):
    return v / np.sqrt(_dot(v, v))[..., None]


def _mix(x, y, a):
    return x * (1.0 - a[..., None]) + y * a[..., None]


def _smoothstep(e0, e1, x):
    t = np.clip((x - e0) / (e1 - e0), 0.0, 1.0)
    return t * t * (3.0 - 2.0 * t)


def sky(d):
    """getEnvironmentalLight, compute.glsl:216-273 -> (colour, sunToOpposite < 0.5, horizonDot < 0)."""
    sun = np.array([0.6, 0.3, -0.2])
    sun = sun / math.sqrt(float(sun @ sun))
    sun_dot = d @ sun
    horizon = d[..., 1]
    zenith, orange, yellow = np.array([0.15, 0.25, 0.65]), np.array([1.2, 0.4, 0.1]), np.array([1.0, 0.8, 0.3])
    blue, ground = np.array([0.3, 0.4, 0.7]), np.array([0.2, 0.15, 0.1])
    s2o = (d @ (-sun) + 1.0) * 0.5
    sun_side = s2o < 0.5
    horizon_colour = np.where(sun_side[..., None], _mix(orange, yellow, s2o * 2.0),
                              _mix(yellow, blue, (s2o - 0.5) * 2.0))
    base = _mix(horizon_colour, zenith, _smoothstep(-0.2, 0.8, horizon))
    centre = np.array([15.0, 15.0, 10.0])
    angle = np.arccos(np.clip(sun_dot, -1.0, 1.0))
    glow = np.exp(-angle * 600.0) + np.exp(-angle * 150.0) * 0.3 + np.exp(-angle * 60.0) * 0.1 \
        + np.exp(-angle * 15.0) * 0.03
    final = base + centre * glow[..., None]
    below = horizon < 0.0
    g = _mix(ground, final, _smoothstep(-0.1, 0.0, horizon))
    g = g + centre * (np.exp(-angle * 15.0) * 0.2)[..., None] * 0.05
    return np.where(below[..., None], g, final), sun_side, below


def tonemap_srgb(x):
    """toSRGB(tonemapACES(x)), compute.glsl:647-658."""
    a, b, c, d, e = 2.51, 0.03, 2.43, 0.59, 0.14
    return np.clip((x * (a * x + b)) / (x * (c * x + d) + e), 0.0, 1.0) ** (1.0 / 2.2)


def gl_texels(image):
    """The texel array GL holds after glTexImage2D(format by channel count,
    GL_UNSIGNED_BYTE) of an stb buffer under GL_UNPACK_ALIGNMENT 4: row y starts
    at byte y * align4(w * channels); bytes past the buffer read as 0.  Returns
    (h, w, 3) float64 in [0, 1], row 0 = t 0, after the channel rules."""
    img = np.ascontiguousarray(image, dtype=np.uint8)
    if img.ndim == 2:
        img = img[..., None]
    h, w, ch = img.shape
    flat = img.reshape(-1)
    stride = (w * ch + 3) // 4 * 4
    y, x, k = np.meshgrid(np.arange(h), np.arange(w), np.arange(ch), indexing="ij")
    at = y * stride + x * ch + k
    padded = np.concatenate([flat, np.zeros(int(at.max()) + 1, np.uint8)])
    c = padded[at].astype(np.float64) / 255.0
    out = np.zeros((h, w, 3))
    if ch == 1:
        out[:] = c[..., :1]
    elif ch == 2:
        out[..., :2] = c
    else:
        out[:] = c[..., :3]
    return out


def sample_linear_repeat(texels, s, t):
    """texture(sampler2D, (s, t)) with GL_LINEAR and GL_REPEAT, GL 4.3 §8.14.2.
    Returns (rgb, i0, j0, floor(u - 1/2), floor(v - 1/2))."""
    h, w, _ = texels.shape
    u, v = s * w - 0.5, t * h - 0.5
    fu, fv = np.floor(u), np.floor(v)
    a, b = (u - fu)[:, None], (v - fv)[:, None]
    i0, j0 = np.mod(fu, w).astype(np.int64), np.mod(fv, h).astype(np.int64)
    i1, j1 = np.mod(fu + 1.0, w).astype(np.int64), np.mod(fv + 1.0, h).astype(np.int64)
    rgb = (1 - a) * (1 - b) * texels[j0, i0] + a * (1 - b) * texels[j0, i1] + (1 - a) * b * texels[j1, i0] \
        + a * b * texels[j1, i1]
    return rgb, i0, j0, fu.astype(np.int64), fv.astype(np.int64)


class _Geometry:
    def __init__(self, tris):
        self.a = tris["a"][:, :3].astype(np.float64)
        self.b = tris["b"][:, :3].astype(np.float64)
        self.c = tris["c"][:, :3].astype(np.float64)
        self.e0, self.e1 = self.b - self.a, self.c - self.a
        self.cr = np.cross(self.e0, self.e1)
        self.uv = np.stack([tris["aTex"], tris["bTex"], tris["cTex"]], 1).astype(np.float64)
        self.mat = tris["materialIndex"].astype(np.int64)
        self.n = len(self.a)

    def closest(self, o, d):
        """rayTriangleIntersect over every triangle, the closest kept (`dst <
        result.dst`, the first in array order on a tie).  -> tri (-1: none), dst, u, v."""
        m = len(o)
        tri = np.full(m, TRI_MISS, np.int64)
        dst, bu, bv = np.full(m, np.inf), np.zeros(m), np.zeros(m)
        if self.n == 0 or m == 0:
            return tri, dst, bu, bv
        step = max(1, 2_000_000 // self.n)
        for s in range(0, m, step):
            oo, dd = o[s:s + step], d[s:s + step]
            det = -(dd @ self.cr.T)
            ri, ti = np.nonzero(~(((det < 1e-10) & (det > -1e-10)) | (det < 0)))
            det = det[ri, ti]
            ao = oo[ri] - self.a[ti]
            t = _dot(ao, self.cr[ti]) / det
            dc = np.cross(dd[ri], ao)
            u = -_dot(self.e1[ti], dc) / det
            v = _dot(self.e0[ti], dc) / det
            keep = ~(t <= 1e-6) & ~((u < 0) | (v < 0) | (1 - u - v < 0))
            ri, ti, t, u, v = ri[keep], ti[keep], t[keep], u[keep], v[keep]
            order = np.lexsort((ti, t, ri))
            ri, ti, t, u, v = ri[order], ti[order], t[order], u[order], v[order]
            first = np.ones(len(ri), bool)
            first[1:] = ri[1:] != ri[:-1]
            r = ri[first] + s
            tri[r], dst[r], bu[r], bv[r] = ti[first], t[first], u[first], v[first]
        return tri, dst, bu, bv


_HEMISPHERE = np.array([(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1)], np.float64)
_HEMISPHERE[13] = 0.0  # the normal itself
_HEMISPHERE[np.arange(27) != 13] = 0.98 * _unit(_HEMISPHERE[np.arange(27) != 13])


def _emitter_behind_scatter(G, mtype, emission, origin, normal, hit_tri):
    """The one emission a ray scattered at `origin` into normalize(normal +
    unit-ball vector) ends on, or NotDeterministic."""
    E = np.zeros((len(origin), 3))
    vertices = np.stack([G.a, G.b, G.c], 0)  # (3, T, 3)
    is_light = mtype[G.mat] == LIGHT
    step = max(1, 1_000_000 // G.n)
    for s in range(0, len(origin), step):
        o, n = origin[s:s + step], normal[s:s + step]
        front = (o @ G.cr.T - _dot(G.a, G.cr)[None, :]) > 0                       # (m, T)
        ahead = ((vertices @ n.T).max(0).T - _dot(o, n)[:, None]) > 0             # some vertex in the hemisphere
        reach = front & ahead
        if (reach & ~is_light[None, :]).any():
            r, t = np.argwhere(reach & ~is_light[None, :])[0]
            raise NotDeterministic(f"a ray scattered on triangle {hit_tri[s + r]} could hit triangle {t}, "
                                   "which is no light")
        if not reach.any(1).all():
            raise NotDeterministic("a scattered ray has no emitter to hit")
        for k in range(3):
            e = np.where(reach, emission[G.mat][None, :, k], np.nan)
            lo, hi = np.nanmin(e, 1), np.nanmax(e, 1)
            if (lo != hi).any():
                raise NotDeterministic("a scattered ray could hit lights of different emission")
            E[s:s + step, k] = lo
    # closure: sample directions over the hemisphere from a few origins per scattering triangle
    for t in np.unique(hit_tri):
        rays = np.nonzero(hit_tri == t)[0]
        pick = rays[np.unique(np.linspace(0, len(rays) - 1, 4).astype(np.int64))]
        o = np.repeat(origin[pick], len(_HEMISPHERE), 0)
        d = _unit(np.repeat(normal[pick], len(_HEMISPHERE), 0) + np.tile(_HEMISPHERE, (len(pick), 1)))
        got, _, _, _ = G.closest(o, d)
        if (got < 0).any() or not is_light[got].all():
            raise NotDeterministic(f"a ray scattered on triangle {t} can leave the emitter")
    return E


def trace_paths(scene, X, Y):
    """main() and trace() for rays through viewport coordinates (X, Y) in
    [-1, 1).  -> radiance (n, 3) of one ray, signature (n, bounces, NF), segments (n,)."""
    un = scene["uniforms"]
    G = _Geometry(scene["triangles"])
    M = scene["materials"]
    mtype = M["materialType"].astype(np.int64)
    colour = M["color"][:, :3].astype(np.float64)
    emission = M["emissionColor"][:, :3].astype(np.float64) * M["emissionStrength"].astype(np.float64)[:, None]
    texels = [None if t is None else gl_texels(t) for t in scene["textures"]]
    if any(un[k] != (0.0, 0.0, 0.0) for k in ("pixelRight", "pixelUp", "defocusDiskRight", "defocusDiskUp")):
        raise NotDeterministic("jitter or defocus is not zero")
    f32 = lambda v: np.asarray(v, np.float32).astype(np.float64)
    cam, right, up, front = (f32(un[k]) for k in ("cameraPos", "viewportRight", "viewportUp", "viewportFront"))
    B = int(un["maxBounceCount"])
    n = len(X)
    end_point = cam + front + right * X[:, None] + up * Y[:, None]
    o = np.broadcast_to(cam, (n, 3)).copy()
    d = _unit(end_point - o)
    ray_colour, light = np.ones((n, 3)), np.zeros((n, 3))
    inside = np.zeros(n, bool)
    sig = np.full((n, max(B, 1), NF), -1, np.int64)
    sig[:, :, F_TRI] = TRI_NOT_REACHED
    segments = np.zeros(n, np.int64)
    alive = np.arange(n)
    for b in range(1, B + 1):
        if alive.size == 0:
            break
        row = b - 1
        segments[alive] += 1
        tri, dst, bu, bv = G.closest(o[alive], d[alive])
        sig[alive, row, F_TRI] = tri
        sig[alive, row, F_END] = 0
        # --- miss: compute.glsl:554-559
        miss = alive[tri < 0]
        if un["environmentalLight"]:
            c, sun_side, below = sky(d[miss])
            light[miss] += c * ray_colour[miss]
            sig[miss, row, F_BRANCH], sig[miss, row, F_END] = BR_SKY, END_SKY
            sig[miss, row, F_SUNSIDE], sig[miss, row, F_BELOW] = sun_side, below
        else:
            sig[miss, row, F_BRANCH], sig[miss, row, F_END] = BR_DARK, END_DARK
        hit = tri >= 0
        r, tri, dst, bu, bv = alive[hit], tri[hit], dst[hit], bu[hit], bv[hit]
        mi = G.mat[tri]
        ty = mtype[mi]
        sig[r, row, F_BRANCH] = ty
        bad = ~np.isin(ty, (DIFFUSE, SPECULAR, LIGHT, CHECKER, GLASS, TEXTURE))
        light[r[bad]] = (1.0, 0.0, 1.0)  # `default: return vec3(1, 0, 1)`
        sig[r[bad], row, F_END] = END_BADTYPE
        # --- LIGHT: :515-520
        L = ty == LIGHT
        light[r[L]] += emission[mi[L]] * ray_colour[r[L]]
        sig[r[L], row, F_END] = END_LIGHT
        go = ~L & ~bad
        r, tri, dst, bu, bv, mi, ty = r[go], tri[go], dst[go], bu[go], bv[go], mi[go], ty[go]
        normal = _unit(G.cr[tri])
        hit_point = o[r] + d[r] * dst[:, None]
        step = d[r] * dst[:, None] * -1e-3
        glass = ty == GLASS
        origin = np.where(glass[:, None], hit_point + step, hit_point - step)  # :489-492
        prev_d = d[r]
        new_d = prev_d.copy()
        att = np.zeros((len(r), 3))
        scatter = np.zeros(len(r), bool)
        # --- SPECULAR: :507-514
        S = ty == SPECULAR
        prob, smooth = M["specularProbability"][mi].astype(np.float64), M["smoothness"][mi].astype(np.float64)
        if (S & (prob != 0.0) & (prob != 1.0)).any():
            raise NotDeterministic("a specular probability other than 0 or 1")
        mirror = S & (prob == 1.0) & (smooth == 1.0)
        nd = _dot(normal, prev_d)
        new_d[mirror] = (prev_d - 2.0 * nd[:, None] * normal)[mirror]  # reflect(I, N); mix(., ., 1)
        att[S & (prob == 1.0)] = 1.0
        att[S & (prob == 0.0)] = colour[mi[S & (prob == 0.0)]]
        scatter |= S & ~mirror
        # --- DIFFUSE / TEXTURE: :501-506
        D = ty == DIFFUSE
        att[D] = colour[mi[D]]
        scatter |= D
        T = np.nonzero(ty == TEXTURE)[0]
        scatter[T] = True
        if T.size:
            w = 1.0 - bu[T] - bv[T]
            uv = G.uv[tri[T], 0] * bu[T, None] + G.uv[tri[T], 1] * bv[T, None] + G.uv[tri[T], 2] * w[:, None]
            index = M["textureIndex"][mi[T]].astype(np.int64)
            rule = np.full(len(T), TR_SAMPLED, np.int64)
            rule[index > 4] = TR_MAGENTA
            rule[index >= int(un["numTextures"])] = TR_BEYOND
            rule[index < 0] = TR_NEGATIVE
            for k in np.unique(index[rule == TR_SAMPLED]):
                sel = (rule == TR_SAMPLED) & (index == k)
                if k >= len(texels) or texels[k] is None:
                    rule[sel] = TR_UNBOUND  # a unit with no complete texture samples (0, 0, 0, 1)
                    continue
                rgb, i0, j0, fu, fv = sample_linear_repeat(texels[k], uv[sel, 0], uv[sel, 1])
                att[T[sel]] = rgb
                for f, val in ((F_I0, i0), (F_J0, j0), (F_FU, fu), (F_FV, fv)):
                    sig[r[T[sel]], row, f] = val
            att[T[rule == TR_MAGENTA]] = (1.0, 0.0, 1.0)
            sig[r[T], row, F_TEXRULE] = rule
            sig[r[T], row, F_TEX] = index
        # --- CHECKER: :521-530, at the offset origin
        K = np.nonzero(ty == CHECKER)[0]
        scatter[K] = True
        if K.size:
            s = M["checkerScale"][mi[K]].astype(np.float64)
            total = np.floor(origin[K] * s[:, None]).sum(-1)
            black = (s > 0.0) & (total - 2.0 * np.floor(total / 2.0) == 0.0)
            att[K] = np.where(black, 0.0, 1.0)[:, None]
            sig[r[K], row, F_CHECKER] = np.where(s > 0.0, np.where(black, CH_BLACK, CH_WHITE), CH_GUARD)
        # --- GLASS: :531-538 and refract_ :201-214
        Gl = np.nonzero(glass)[0]
        if Gl.size:
            ior = M["refractiveIndex"][mi[Gl]].astype(np.float64)
            eta = np.where(inside[r[Gl]], ior, 1.0 / ior)
            I, N, ndi = prev_d[Gl], normal[Gl], nd[Gl]
            k = 1.0 - eta * eta * (1.0 - ndi * ndi)
            refracted = ~(k < 0.0)
            with np.errstate(invalid="ignore"):
                bent = eta[:, None] * I - (eta * ndi + np.sqrt(k))[:, None] * N
            new_d[Gl] = np.where(refracted[:, None], bent, I - 2.0 * ndi[:, None] * N)
            inside[r[Gl]] = refracted != inside[r[Gl]]
            att[Gl] = colour[mi[Gl]]
            sig[r[Gl], row, F_REFRACTED] = refracted
        sig[r, row, F_INSIDE] = inside[r]
        # --- :543-552
        passes = (M["isEdgeHighlight"][mi] != 0) & (b > 1)
        new_d[passes] = prev_d[passes]
        scatter &= ~passes
        sig[r[passes], row, F_BRANCH] = BR_PASS
        ray_colour[r[~passes]] *= att[~passes]
        p = ray_colour[r].max(-1)
        absorbed = p == 0.0
        if (~absorbed & (np.abs(p - 1.0) > 1e-6)).any():
            raise NotDeterministic(f"survival probability {p[~absorbed & (np.abs(p - 1.0) > 1e-6)][0]!r}")
        sig[r[absorbed], row, F_END] = END_ABSORBED
        o[r], d[r] = origin, new_d
        sc = scatter & ~absorbed
        if sc.any() and b < B:
            E = _emitter_behind_scatter(G, mtype, emission, origin[sc], normal[sc], tri[sc])
            light[r[sc]] += E * ray_colour[r[sc]]
            segments[r[sc]] += 1
            sig[r[sc], row + 1, F_TRI], sig[r[sc], row + 1, F_END] = TRI_EMITTER, END_SCATTER
        elif sc.any():
            sig[r[sc], row, F_END] = END_CUT
        alive = r[~absorbed & ~scatter]
    if B > 0:
        sig[alive, B - 1, F_END] = END_CUT
    return light, sig, segments


class Model:
    """value (H, W, 3), signature (H, W, bounces, NF), segments (H, W) of one
    ray, bracket and bound (H, W), excluded (H, W)."""

    def __init__(self, scene, delta=DELTA):
        un = scene["uniforms"]
        W, H = int(un["width"]), int(un["height"])
        x = (np.arange(W) * 2.0 - W) / W
        y = (np.arange(H) * 2.0 - H) / H
        X, Y = (g.reshape(-1) for g in np.meshgrid(x, y))
        moves = ((0, 0), (delta, 0), (-delta, 0), (0, delta), (0, -delta))
        light, sig, seg = trace_paths(scene, np.concatenate([X + mx for mx, _ in moves]),
                                      np.concatenate([Y + my for _, my in moves]))
        value = tonemap_srgb(light).reshape(5, H, W, 3)
        sig = sig.reshape(5, H, W, -1, NF)
        self.name = scene["name"]
        self.delta = delta
        self.value = value[0]
        self.signature = sig[0]
        self.segments = seg.reshape(5, H, W)[0]
        self.excluded = (sig[1:] != sig[:1]).any((0, 3, 4))
        self.bracket = np.abs(value[1:] - value[:1]).max((0, 3))
        self.bound = BASE_BOUND + self.bracket
        for a in (self.value, self.signature, self.segments, self.excluded, self.bracket, self.bound):
            a.setflags(write=False)

    # --- signature classes: (H, W) masks
    def any_bounce(self, field, value):
        return (self.signature[..., field] == value).any(-1)

    def classes(self):
        s = self.signature
        glass = s[..., F_BRANCH] == GLASS
        refr, ins = s[..., F_REFRACTED], s[..., F_INSIDE]
        same_as_before = np.zeros(glass.shape, bool)
        same_as_before[..., 1:] = s[..., 1:, F_TRI] == s[..., :-1, F_TRI]
        inside_before = np.zeros(glass.shape, bool)
        inside_before[..., 1:] = ins[..., :-1] == 1
        sampled = s[..., F_TEXRULE] == TR_SAMPLED
        ended = s[..., F_END].max(-1)
        out = {
            "sky_below_horizon": self.any_bounce(F_BELOW, 1),
            "sky_sun_side": self.any_bounce(F_SUNSIDE, 1),
            "sky_opposite_side": self.any_bounce(F_SUNSIDE, 0),
            "glass_refracted_in": (glass & (refr == 1) & ~inside_before & (ins == 1)).any(-1),
            "glass_toggled_back": (glass & same_as_before & (refr == 1) & inside_before & (ins == 0)).any(-1),
            "glass_total_internal_reflection": (glass & (refr == 0) & inside_before).any(-1),
            "glass_entry_reflection": (glass & (refr == 0) & ~inside_before).any(-1),
            "edge_pass_through": self.any_bounce(F_BRANCH, BR_PASS),
            "checker_black": self.any_bounce(F_CHECKER, CH_BLACK),
            "checker_white": self.any_bounce(F_CHECKER, CH_WHITE),
            "checker_guard": self.any_bounce(F_CHECKER, CH_GUARD),
            "texel_negative_column": (sampled & (s[..., F_FU] < 0)).any(-1),
            "texel_negative_row": (sampled & (s[..., F_FV] < 0)).any(-1),
            "texture_rule_negative": self.any_bounce(F_TEXRULE, TR_NEGATIVE),
            "texture_rule_beyond": self.any_bounce(F_TEXRULE, TR_BEYOND),
            "texture_rule_magenta": self.any_bounce(F_TEXRULE, TR_MAGENTA),
            "texture_rule_unbound": self.any_bounce(F_TEXRULE, TR_UNBOUND),
        }
        for k in (1, 2, 3):
            out[f"cut_at_limit_{k}"] = (ended == END_CUT) & (self.segments == k)
        return out

    def texture_class(self, index, width, height):
        s = self.signature
        on = (s[..., F_TEXRULE] == TR_SAMPLED) & (s[..., F_TEX] == index)
        return {"sampled": on.any(-1), "column_wrap": (on & (s[..., F_I0] == width - 1)).any(-1),
                "row_wrap": (on & (s[..., F_J0] == height - 1)).any(-1)}

    def describe(self, y, x):
        names = ("tri", "branch", "refracted", "inside", "checker", "i0", "j0", "texrule", "sunside", "below", "end",
                 "fu", "fv", "tex")
        rows = [dict((k, int(v)) for k, v in zip(names, row) if v != -1) for row in self.signature[y, x]
                if row[F_TRI] != TRI_NOT_REACHED]
        return "; ".join(str(r) for r in rows)


_models = {}


def model_for(scene, delta=DELTA):
    """The model of a scene of shading_scenes.py, computed once per session (scene["name"] is the key)."""
    key = (scene["name"], delta)
    if key not in _models:
        _models[key] = Model(scene, delta)
    return _models[key]


def image_error(model, image):
    """Per-pixel max |image - model| over rgb; image: (H, W, >= 3) mean over rays and frames."""
    return np.abs(np.asarray(image)[..., :3].astype(np.float64) - model.value).max(-1)


def assert_image(model, image, what):
    """The comparison rule.  Returns the largest error over the compared pixels."""
    err = image_error(model, image)
    miss = ~model.excluded & ~(err <= model.bound)
    over = np.where(model.excluded, 0.0, err - model.bound)
    y, x = np.unravel_index(int(np.argmax(over)), over.shape)
    assert not miss.any(), (
        f"{model.name} ({what}): {int(miss.sum())} of {miss.size} pixels outside the bound; worst pixel x={x} y={y}: "
        f"image {np.asarray(image)[y, x, :3].tolist()} model {model.value[y, x].tolist()} error {err[y, x]:.3e} "
        f"bound {model.bound[y, x]:.3e}; path: {model.describe(y, x)}")
    return float(np.where(model.excluded, 0.0, err).max())


def assert_exclusions(model, extra_classes=None):
    """At most 3 % of the pixels excluded, and at most 10 % of any signature class."""
    frac = float(model.excluded.mean())
    assert frac <= 0.03, f"{model.name}: {frac:.1%} of the pixels excluded"
    classes = model.classes()
    classes.update(extra_classes or {})
    for name, mask in classes.items():
        if mask.any():
            f = float(model.excluded[mask].mean())
            assert f <= 0.10, f"{model.name}: {f:.1%} of the {int(mask.sum())} pixels of class {name} excluded"
    return frac
