"""The float64 model of tests/shading_model.py, extended to carry the shader's
random stream: one sample's path followed with its own draws.

TEST INFRASTRUCTURE ONLY.  Written from compute.glsl (random :148-159,
randomDirection2D :161-165, randomDirection :174-185, trace :472-563, main
:660-701).  Geometry, sky, tonemap and texture code are imported from
shading_model.py; nothing is shared with oracle/rt_oracle.c, the product
package or its headers, and nothing but numpy is imported besides.

Draws are exact.  The generator runs on uint64 integers masked to 32 bits.  The
shader returns `result / 4294967295.0`: `result` is a uint, the literal a
float, so the uint is converted to binary32 (round to nearest, ties to even:
the only rounding in the expression) and divided by the binary32 nearest to
2^32 - 1, which is 2^32 itself, since 2^32 - 1 needs 32 significant bits and
lies one 256th of a binary32 step below 2^32.  A division by a power of two
is exact (the smallest non-zero quotient, 2^-32, is a normal number).  The
value of a draw is therefore round24(r) * 2^-32, computed here on integers,
and it is 1.0 for r >= 2^32 - 128.  `specularProbability > random()` then
compares two binary32 values exactly.

Everything after a draw is float64: the disk point, the jitter, the candidate
vector, its length and normalisation, normalize(normal + dir), the mix by
smoothness (not normalised: the shader does not), the roulette and the
rescaling by 1 / p.

A sample is one (pixel, frame): its seed is set once, from x + y * width +
frame * 968824447 in 32 bits, and runs on through the numRaysPerPixel rays.  The
model vectorises over samples; a sample's state advances only when that
sample draws.

Comparison rule (assert_image).  f32 and f64 may decide a sample differently
at a triangle's edge, a texel boundary, a checker line, the accept test of a
candidate or the roulette.  Each scene is evaluated 7 times: as it is, and
with every segment's direction (primary, scattered, mixed, reflected,
refracted, passed through) moved by +-DELTA along one world axis before it is
normalised (or, where the shader does not normalise, as it stands).  A pixel
whose signatures differ between the evaluations, in any ray or frame, is
excluded, and so is one with a sample in which an accept test has |s - 1| <=
GUARD or a roulette has |rnd - p| <= GUARD.  The roulette needs no guard where
f32 holds the same p as the model: p = 0 (a product with an exact 0), and p = 1
while every attenuation of the path so far was exactly (1, 1, 1); there
`random > p` is decided by the draw alone, also for a draw of 1.0 against
p = 1.  For the others the bound is
BASE_BOUND + max |value(moved) - value| on the final value: mean over rays,
tonemap, mean over frames.
"""
import numpy as np

import shading_model as sm
from shading_model import (BASE_BOUND, BR_DARK, BR_PASS, BR_SKY, CH_BLACK, CH_GUARD, CH_WHITE, CHECKER, DELTA_MAX,
                           DIFFUSE, END_BADTYPE, END_CUT, END_DARK, END_LIGHT, END_SKY, F_BELOW, F_BRANCH, F_CHECKER,
                           F_END, F_FU, F_FV, F_I0, F_INSIDE, F_J0, F_REFRACTED, F_SUNSIDE, F_TEX, F_TEXRULE, F_TRI,
                           GLASS, LIGHT, SPECULAR, TEXTURE, TR_BEYOND, TR_MAGENTA, TR_NEGATIVE, TR_SAMPLED, TR_UNBOUND,
                           TRI_NOT_REACHED)

# DELTA: the smallest power of two at which the CPU oracle passes every scene of
# random_scenes.py under the rule above; the ceiling is shading_model.DELTA_MAX.
# One pixel needs it: (27, 4) of diffuse_floor/b2, the brightest of the scene,
# is off by 8.5e-5, 0.96 of its bound at 2^-17 and 1.87 times its bound at
# 2^-18.  Without it 2^-19 would do (diffuse_floor/b3 and checker_floor miss by
# up to 1.5 times at 2^-20); the sky, ramp, glass, edge and box scenes pass from
# 2^-24 on.  Measured at 2^-17, oracle against model (max error over the compared
# pixels / largest bound / excluded pixels): jitter_sky, defocus_sky,
# draw_is_one 1.6e-7 / 5.8e-5 / <= 0.06 %, jitter_defocus_ramp 8.6e-8 / 2.0e-6 /
# 0.44 %, diffuse_floor/b2 8.5e-5 / 8.8e-5 / 0, diffuse_floor/b3 5.4e-6 / 3.9e-5
# / 0, specular_mix 9.2e-6 / 4.7e-4 / 0, texture_floor 6.4e-6 / 4.7e-3 / 0,
# checker_floor 6.9e-6 / 6.7e-5 / 0.28 %, glass_tinted 1.5e-7 / 1.9e-4 / 0.11 %,
# edge_after_scatter 1.2e-7 / 2.1e-4 / 0, open_box 7.9e-7 / 1.4e-4 / 0.28 %,
# probability_is_one, roulette_is_one 2.1e-7 / 6.8e-6 / 0.  The table is in
# DESIGN.md "Random paths".
DELTA = 2.0 ** -17
assert DELTA <= DELTA_MAX
GUARD = 1e-5

# further signature fields, after shading_model's
F_CAND, F_SPECBOUNCE, F_ROULETTE, F_DISCARDED = range(sm.NF, sm.NF + 4)
NF = sm.NF + 4
RL_KILLED, RL_BELOW_ONE, RL_ONE = 0, 1, 2    # F_ROULETTE
END_KILLED = 8                               # F_END besides shading_model's

MASK32 = np.uint64(0xFFFFFFFF)
FRAME_MULTIPLIER = 968824447


def draw_bits(state, at):
    """random(), compute.glsl:148-152, on the samples `at` (distinct indices):
    advances their state and returns `result` as uint64."""
    s = (state[at] * np.uint64(747796405) + np.uint64(2891336453)) & MASK32
    state[at] = s
    r = (((s >> ((s >> np.uint64(28)) + np.uint64(4))) ^ s) * np.uint64(277803737)) & MASK32
    return (r >> np.uint64(22)) ^ r


def draw_value(r):
    """float(r) / 4294967295.0f as the header derives it: r rounded to 24
    significant bits, ties to even, times 2^-32."""
    r = np.asarray(r, np.uint64)
    bits = np.frexp(r.astype(np.float64))[1]            # exact: r < 2^53
    e = np.maximum(bits - 24, 0).astype(np.uint64)
    q = r >> e
    rem = r - (q << e)
    half = (np.uint64(1) << e) >> np.uint64(1)          # 0 where e == 0
    up = (e > 0) & ((rem > half) | ((rem == half) & ((q & np.uint64(1)) == 1)))
    q = q + up.astype(np.uint64)
    return np.ldexp(q.astype(np.float64), e.astype(np.int64) - 32)


def first_seed(x, y, width, frame):
    """texelCoord.x + texelCoord.y * size.x + frameIndex * 968824447u, in 32 bits."""
    x, y, frame = (np.asarray(v, np.uint64) for v in (x, y, frame))
    return (x + y * np.uint64(width) + frame * np.uint64(FRAME_MULTIPLIER)) & MASK32


def frame_term_wraps(frame):
    return int(frame) * FRAME_MULTIPLIER >= 2 ** 32


class _Stream:
    """The per-sample generator state with the bookkeeping the rule needs."""

    def __init__(self, seed):
        self.state = np.array(seed, np.uint64)
        n = len(self.state)
        self.draws = np.zeros(n, np.int64)
        self.guarded = np.zeros(n, bool)
        self.drew_one = np.zeros(n, bool)

    def random(self, at):
        v = draw_value(draw_bits(self.state, at))
        self.draws[at] += 1
        self.drew_one[at] |= v == 1.0
        return v

    def direction(self, at):
        """randomDirection, :174-185 -> (unit vectors, candidates used)."""
        out = np.zeros((len(at), 3))
        used = np.zeros(len(at), np.int64)
        pending = np.arange(len(at))
        for _ in range(100):
            if pending.size == 0:
                return out, used
            who = at[pending]
            v = np.stack([self.random(who) * 2.0 - 1.0 for _ in range(3)], -1)
            s = (v * v).sum(-1)
            length = np.sqrt(s)
            self.guarded[who] |= np.abs(s - 1.0) <= GUARD
            ok = length < 1.0
            with np.errstate(invalid="ignore", divide="ignore"):
                out[pending[ok]] = v[ok] / length[ok, None]
            used[pending] += 1
            pending = pending[~ok]
        if pending.size:
            raise NotImplementedError("randomDirection left its loop after 100 candidates: not modelled")
        return out, used


def _trace(ctx, stream, o, d, move, sig):
    """trace(), :472-563, for one ray of every sample.  o, d: (n, 3), changed in
    place; sig: (n, bounces, NF), filled.  -> incoming light (n, 3), segments (n,)."""
    un, G, M, mtype, colour, emission, texels = ctx
    B = int(un["maxBounceCount"])
    n = len(o)
    ray_colour, light = np.ones((n, 3)), np.zeros((n, 3))
    inside = np.zeros(n, bool)
    untouched = np.ones(n, bool)     # rayColor is (1, 1, 1) by construction: in f32 as here
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
        # --- miss: :554-559
        miss = alive[tri < 0]
        if un["environmentalLight"]:
            c, sun_side, below = sm.sky(d[miss])
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
        normal = sm._unit(G.cr[tri])
        hit_point = o[r] + d[r] * dst[:, None]
        step = d[r] * dst[:, None] * -1e-3
        glass = ty == GLASS
        origin = np.where(glass[:, None], hit_point + step, hit_point - step)  # :489-492
        prev_d = d[r]
        new_d = prev_d.copy()
        att = np.zeros((len(r), 3))
        nd = sm._dot(normal, prev_d)
        # --- every case but LIGHT and GLASS begins with randomDirection: :503, :508, :522
        scatter = np.isin(ty, (DIFFUSE, TEXTURE, SPECULAR, CHECKER))
        random_dir, used = stream.direction(r[scatter])
        sig[r[scatter], row, F_CAND] = np.minimum(used, 3)
        D = ty == DIFFUSE
        att[D] = colour[mi[D]]
        plain = scatter & (ty != SPECULAR)
        new_d[plain] = sm._unit(normal[plain] + random_dir[(ty != SPECULAR)[scatter]] + move)
        # --- SPECULAR: :507-514; the probability draw follows the direction's draws
        S = np.nonzero(ty == SPECULAR)[0]
        if S.size:
            diffuse_dir = sm._unit(normal[S] + random_dir[(ty == SPECULAR)[scatter]])
            mirrored = prev_d[S] - 2.0 * nd[S, None] * normal[S]                      # reflect(I, N)
            is_specular = M["specularProbability"][mi[S]].astype(np.float64) > stream.random(r[S])
            a = np.where(is_specular, M["smoothness"][mi[S]].astype(np.float64), 0.0)
            new_d[S] = sm._mix(diffuse_dir, mirrored, a) + move                       # mix(), left as long as it is
            att[S] = np.where(is_specular[:, None], 1.0, colour[mi[S]])
            sig[r[S], row, F_SPECBOUNCE] = is_specular
        # --- TEXTURE: getTriangleTextureColor :342-368
        T = np.nonzero(ty == TEXTURE)[0]
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
                    rule[sel] = TR_UNBOUND
                    continue
                rgb, i0, j0, fu, fv = sm.sample_linear_repeat(texels[k], uv[sel, 0], uv[sel, 1])
                att[T[sel]] = rgb
                for f, val in ((F_I0, i0), (F_J0, j0), (F_FU, fu), (F_FV, fv)):
                    sig[r[T[sel]], row, f] = val
            att[T[rule == TR_MAGENTA]] = (1.0, 0.0, 1.0)
            sig[r[T], row, F_TEXRULE] = rule
            sig[r[T], row, F_TEX] = index
        # --- CHECKER: :521-530, at the offset origin
        K = np.nonzero(ty == CHECKER)[0]
        if K.size:
            s = M["checkerScale"][mi[K]].astype(np.float64)
            total = np.floor(origin[K] * s[:, None]).sum(-1)
            black = (s > 0.0) & (total - 2.0 * np.floor(total / 2.0) == 0.0)
            att[K] = np.where(black, 0.0, 1.0)[:, None]
            sig[r[K], row, F_CHECKER] = np.where(s > 0.0, np.where(black, CH_BLACK, CH_WHITE), CH_GUARD)
        # --- GLASS: :531-538 and refract_ :201-214; no draw
        Gl = np.nonzero(glass)[0]
        if Gl.size:
            ior = M["refractiveIndex"][mi[Gl]].astype(np.float64)
            eta = np.where(inside[r[Gl]], ior, 1.0 / ior)
            I, N, ndi = prev_d[Gl], normal[Gl], nd[Gl]
            k = 1.0 - eta * eta * (1.0 - ndi * ndi)
            refracted = ~(k < 0.0)
            with np.errstate(invalid="ignore"):
                bent = eta[:, None] * I - (eta * ndi + np.sqrt(k))[:, None] * N
            new_d[Gl] = np.where(refracted[:, None], bent, I - 2.0 * ndi[:, None] * N) + move
            inside[r[Gl]] = refracted != inside[r[Gl]]
            att[Gl] = colour[mi[Gl]]
            sig[r[Gl], row, F_REFRACTED] = refracted
        sig[r, row, F_INSIDE] = inside[r]
        # --- :543-546: the direction just drawn is dropped, the colour kept
        passes = (M["isEdgeHighlight"][mi] != 0) & (b > 1)
        new_d[passes] = prev_d[passes] + move
        sig[r[passes], row, F_BRANCH] = BR_PASS
        sig[r[passes & scatter], row, F_DISCARDED] = 1
        ray_colour[r[~passes]] *= att[~passes]
        untouched[r[~passes]] &= (att[~passes] == 1.0).all(-1)
        # --- :548-552: one draw whatever the material
        p = ray_colour[r].max(-1)
        rnd = stream.random(r)
        same_in_f32 = (p == 0.0) | (untouched[r] & (p == 1.0))
        stream.guarded[r] |= (np.abs(rnd - p) <= GUARD) & ~same_in_f32
        killed = rnd > p
        sig[r, row, F_ROULETTE] = np.where(killed, RL_KILLED, np.where(p < 1.0, RL_BELOW_ONE, RL_ONE))
        sig[r[killed], row, F_END] = END_KILLED
        live = ~killed
        ray_colour[r[live]] *= (1.0 / p[live])[:, None]
        o[r], d[r] = origin, new_d
        alive = r[live]
    if B > 0:
        sig[alive, B - 1, F_END] = END_CUT
    return light, segments


def evaluate(scene, move=(0.0, 0.0, 0.0)):
    """main(), :660-701, for every (frame, pixel) of the scene.  -> per-frame
    colour before the tonemap (F, H, W, 3), signature (F, H, W, rays, bounces,
    NF), segments, draws, guarded, drew_one (F, H, W)."""
    un = scene["uniforms"]
    ctx = (un, sm._Geometry(scene["triangles"]), scene["materials"],
           scene["materials"]["materialType"].astype(np.int64),
           scene["materials"]["color"][:, :3].astype(np.float64),
           scene["materials"]["emissionColor"][:, :3].astype(np.float64)
           * scene["materials"]["emissionStrength"].astype(np.float64)[:, None],
           [None if t is None else sm.gl_texels(t) for t in scene["textures"]])
    f32 = lambda v: np.asarray(v, np.float32).astype(np.float64)
    cam, right, up, front, pixel_right, pixel_up, disk_right, disk_up = (f32(un[k]) for k in (
        "cameraPos", "viewportRight", "viewportUp", "viewportFront", "pixelRight", "pixelUp", "defocusDiskRight",
        "defocusDiskUp"))
    W, H, R, B = int(un["width"]), int(un["height"]), int(un["numRaysPerPixel"]), int(un["maxBounceCount"])
    first, count = scene["frames"]
    move = np.asarray(move, np.float64)
    fr, ty, tx = (g.reshape(-1) for g in np.meshgrid(np.arange(first, first + count), np.arange(H), np.arange(W),
                                                     indexing="ij"))
    n = len(tx)
    x, y = (tx * 2.0 - W) / W, (ty * 2.0 - H) / H
    stream = _Stream(first_seed(tx, ty, W, fr))
    end_point = cam + front + right * x[:, None] + up * y[:, None]
    everyone = np.arange(n)
    total = np.zeros((n, 3))
    sig = np.full((n, R, max(B, 1), NF), -1, np.int64)
    sig[..., F_TRI] = TRI_NOT_REACHED
    segments = np.zeros(n, np.int64)
    for i in range(R):
        angle = stream.random(everyone)                                             # drawn whatever the disk
        o = cam + disk_right * np.cos(angle)[:, None] + disk_up * np.sin(angle)[:, None]
        jr = -0.5 + (0.5 - -0.5) * stream.random(everyone)
        ju = -0.5 + (0.5 - -0.5) * stream.random(everyone)
        jittered = end_point + pixel_right * jr[:, None] + pixel_up * ju[:, None]
        d = sm._unit(jittered - o + move)
        light, seg = _trace(ctx, stream, o, d, move, sig[:, i])       # a view: filled in place
        total += light
        segments += seg
    shape = (count, H, W)
    return ((total / R).reshape(shape + (3,)), sig.reshape(shape + sig.shape[1:]), segments.reshape(shape),
            stream.draws.reshape(shape), stream.guarded.reshape(shape), stream.drew_one.reshape(shape))


class Model:
    """value (H, W, 3): the mean over the frames of toSRGB(tonemapACES(mean over
    the rays)); signature (F, H, W, rays, bounces, NF), segments, draws, drew_one
    (F, H, W); excluded, bracket and bound (H, W)."""

    def __init__(self, scene, delta=DELTA):
        colour, sig, seg, draws, guarded, one = evaluate(scene)
        self.name, self.delta = scene["name"], delta
        self.frames = scene["frames"]
        self.value = sm.tonemap_srgb(colour).mean(0)
        self.signature, self.segments, self.draws, self.drew_one = sig, seg, draws, one
        self.guarded = guarded.any(0)
        differs = np.zeros(self.guarded.shape, bool)
        self.bracket = np.zeros(self.guarded.shape)
        for axis in range(3):
            for sign in (1.0, -1.0):
                move = np.zeros(3)
                move[axis] = sign * delta
                c2, sig2, _, draws2, _, _ = evaluate(scene, move)
                differs |= (sig2 != sig).any((0, 3, 4, 5)) | (draws2 != draws).any(0)
                self.bracket = np.maximum(self.bracket, np.abs(sm.tonemap_srgb(c2).mean(0) - self.value).max(-1))
        self.excluded = differs | self.guarded
        self.bound = BASE_BOUND + self.bracket
        for a in (self.value, self.signature, self.segments, self.draws, self.drew_one, self.guarded, self.excluded,
                  self.bracket, self.bound):
            a.setflags(write=False)

    def classes(self):
        """name -> (F, H, W) mask of the pixel-frames with a ray that takes the branch."""
        s = self.signature
        any_ = lambda field, value: (s[..., field] == value).any((-1, -2))
        roulette, bounce = s[..., F_ROULETTE], np.arange(s.shape[-2])
        glass = s[..., F_BRANCH] == GLASS
        return {
            "candidates_1": any_(F_CAND, 1), "candidates_2": any_(F_CAND, 2), "candidates_3_or_more": any_(F_CAND, 3),
            "specular_bounce": any_(F_SPECBOUNCE, 1), "specular_declined": any_(F_SPECBOUNCE, 0),
            "killed_at_bounce_1": (roulette[..., 0] == RL_KILLED).any(-1),
            "killed_at_a_later_bounce": ((roulette == RL_KILLED) & (bounce > 0)).any((-1, -2)),
            "survived_below_one": any_(F_ROULETTE, RL_BELOW_ONE), "survived_at_one": any_(F_ROULETTE, RL_ONE),
            "scatter_discarded": any_(F_DISCARDED, 1),
            "drew_one": np.asarray(self.drew_one),
            "sky_below_horizon": any_(F_BELOW, 1), "sky_sun_side": any_(F_SUNSIDE, 1),
            "sky_opposite_side": any_(F_SUNSIDE, 0),
            "glass_refracted": (glass & (s[..., F_REFRACTED] == 1)).any((-1, -2)),
            "glass_reflected": (glass & (s[..., F_REFRACTED] == 0)).any((-1, -2)),
            "edge_pass_through": any_(F_BRANCH, BR_PASS),
            "checker_black": any_(F_CHECKER, CH_BLACK), "checker_white": any_(F_CHECKER, CH_WHITE),
            "texture_sampled": any_(F_TEXRULE, TR_SAMPLED),
            "ended_on_light": any_(F_END, END_LIGHT), "ended_in_sky": any_(F_END, END_SKY),
            "cut_at_limit": any_(F_END, END_CUT),
        }

    def compared(self, cls):
        """The compared pixel-frames of a class."""
        return int((self.classes()[cls] & ~self.excluded[None]).sum())

    def describe(self, y, x):
        names = ("tri", "branch", "refracted", "inside", "checker", "i0", "j0", "texrule", "sunside", "below", "end",
                 "fu", "fv", "tex", "candidates", "specular", "roulette", "discarded")
        out = []
        for f in range(self.signature.shape[0]):
            for i in range(self.signature.shape[3]):
                rows = [dict((k, int(v)) for k, v in zip(names, row) if v != -1)
                        for row in self.signature[f, y, x, i] if row[F_TRI] != TRI_NOT_REACHED]
                out.append(f"frame {self.frames[0] + f} ray {i}: " + "; ".join(str(r) for r in rows))
        return " | ".join(out)


_models = {}


def model_for(scene, delta=DELTA):
    """The model of a scene of random_scenes.py, computed once per session (scene["name"] is the key)."""
    key = (scene["name"], delta)
    if key not in _models:
        _models[key] = Model(scene, delta)
    return _models[key]


def assert_image(model, image, what, rows=None):
    """The comparison rule; rows: the image holds these rows of the model's.
    Returns the largest error over the compared pixels."""
    rows = np.arange(model.value.shape[0]) if rows is None else np.asarray(rows)
    value, bound, excluded = model.value[rows], model.bound[rows], model.excluded[rows]
    err = np.abs(np.asarray(image)[..., :3].astype(np.float64) - value).max(-1)
    miss = ~excluded & ~(err <= bound)
    over = np.where(excluded, 0.0, err - bound)
    y, x = np.unravel_index(int(np.argmax(over)), over.shape)
    assert not miss.any(), (
        f"{model.name} ({what}): {int(miss.sum())} of {miss.size} pixels outside the bound; worst pixel x={x} "
        f"y={rows[y]}: image {np.asarray(image)[y, x, :3].tolist()} model {value[y, x].tolist()} error {err[y, x]:.3e} "
        f"bound {bound[y, x]:.3e}; path: {model.describe(rows[y], x)}")
    return float(np.where(excluded, 0.0, err).max())


def assert_exclusions(model):
    """At most 3 % of the pixels excluded, and at most 10 % of the pixel-frames of any signature class."""
    frac = float(model.excluded.mean())
    assert frac <= 0.03, f"{model.name}: {frac:.1%} of the pixels excluded"
    for name, mask in model.classes().items():
        if mask.any():
            f = float(np.broadcast_to(model.excluded[None], mask.shape)[mask].mean())
            assert f <= 0.10, f"{model.name}: {f:.1%} of the {int(mask.sum())} pixel-frames of class {name} excluded"
    return frac
