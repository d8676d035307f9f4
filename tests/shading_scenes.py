"""Scenes whose paths do not depend on the random numbers, for
tests/shading_model.py: no pixel jitter, no defocus, mirrors of probability 1
and smoothness 1, colours whose largest channel is 1, and every randomly
scattered ray ending on one uniform emitter.

Each scene is a dict: name, triangles / materials (numpy records in the
reference's layouts, rt2.TRI_DTYPE / MAT_DTYPE field for field), textures (stb
layout uint8 arrays; None = a unit with nothing bound), uniforms (numbers and
3-tuples named after GlobalUniforms) and frames = (first, count).  Only numpy is
imported; textures come from a fixed seed.

Scattering surfaces (diffuse, checker, texture) sit inside an inward-facing
emissive box of one colour and all lie in one plane facing the camera, together
with everything else the scene shows.  The offset origin of a scattered ray is
behind that plane (`hit - dir * dst * -1e-3` moves past the surface), and the
scatter hemisphere points back to the camera's side, where back-face culling
leaves only the box.  A textured quad cannot be shown in a mirror this way (the
mirror would face the scattered ray), so the non-primary textured hit is seen
through a glass pane instead.

Glass distances.  A glass face is hit again from its own front at about 1e-3
and 1e-6 of the first distance before the next candidate falls under the
shader's 1e-6.  The third hit is decided by dst, a difference of f32
coordinates, against 1e-6: with first hits 2 to 4 units away and vertices
within +-3 the second re-hit lies near 2e-6 .. 4e-6 and the third near 1e-9,
both decisive against half an ulp of the hit point (about 1.2e-7).  Farther or
larger glass makes f32 and f64 take different paths, which is the reference's
own noise; every glass face here stays in that range.
"""
import numpy as np

TRI_DTYPE = np.dtype([("a", "<f4", 4), ("b", "<f4", 4), ("c", "<f4", 4), ("aTex", "<f4", 2), ("bTex", "<f4", 2),
                      ("cTex", "<f4", 2), ("materialIndex", "<i4"), ("pad", "<f4")])
MAT_DTYPE = np.dtype([("color", "<f4", 4), ("specularColor", "<f4", 4), ("emissionColor", "<f4", 4),
                      ("textureIndex", "<i4"), ("emissionStrength", "<f4"), ("smoothness", "<f4"),
                      ("specularProbability", "<f4"), ("checkerScale", "<f4"), ("refractiveIndex", "<f4"),
                      ("materialType", "<i4"), ("index", "<i4"), ("isEdgeHighlight", "<i4"), ("pad1", "<i4"),
                      ("pad2", "<i4"), ("pad3", "<i4")])
DIFFUSE, SPECULAR, LIGHT, CHECKER, GLASS, TEXTURE = 0, 1, 2, 3, 4, 5

BOX_EMISSION = ((0.9, 0.7, 0.5), 0.8)
RAMP_STRENGTHS = [float(s) for s in np.logspace(-4, 3, 16)]
BOUNCE_LIMITS = (1, 2, 3, 4, 12)
# With viewportFront (0, 0, -1) the middle row looks along y = 0 exactly, where horizonDot < 0 is decided by
# rounding; this puts the horizon half a row (of 48) above row 23 instead.
HORIZON_FRONT = (0.0, 0.0125, -1.0)


class _Builder:
    def __init__(self):
        self.mats, self.tris = [], []

    def material(self, kind, color=(1, 1, 1), emission=(0, 0, 0), strength=0.0, smooth=0.0, prob=0.0, checker=0.0,
                 ior=1.0, texture=-1, edge=0):
        m = np.zeros((), MAT_DTYPE)
        m["color"][:3], m["color"][3] = color, 1.0
        m["specularColor"][:] = 1.0
        m["emissionColor"][:3] = emission
        m["emissionStrength"], m["smoothness"], m["specularProbability"] = strength, smooth, prob
        m["checkerScale"], m["refractiveIndex"], m["textureIndex"] = checker, ior, texture
        m["materialType"], m["isEdgeHighlight"], m["index"] = kind, edge, len(self.mats)
        self.mats.append(m)
        return len(self.mats) - 1

    def light(self, colour, strength):
        return self.material(LIGHT, emission=colour, strength=strength)

    def mirror(self):
        return self.material(SPECULAR, smooth=1.0, prob=1.0)

    def quad(self, p, eu, ev, mat, uv=None):
        """Two triangles over p + s*eu + t*ev; front (normal eu x ev) towards the
        viewer.  uv: at p, p+eu, p+eu+ev, p+ev."""
        p, eu, ev = (np.asarray(v, np.float64) for v in (p, eu, ev))
        q = [p, p + eu, p + eu + ev, p + ev]
        uv = uv or [(0, 0), (1, 0), (1, 1), (0, 1)]
        for a, b, c in ((0, 1, 2), (0, 2, 3)):
            t = np.zeros((), TRI_DTYPE)
            t["a"][:3], t["b"][:3], t["c"][:3] = q[a], q[b], q[c]
            t["aTex"], t["bTex"], t["cTex"] = uv[a], uv[b], uv[c]
            t["materialIndex"] = mat
            self.tris.append(t)

    def box(self, half, mat):
        """Six quads facing inward."""
        for ax in range(3):
            for sg in (-1.0, 1.0):
                n, e1, e2 = np.zeros(3), np.zeros(3), np.zeros(3)
                n[ax], e1[(ax + 1) % 3], e2[(ax + 2) % 3] = -sg, 1.0, 1.0
                if np.cross(e1, e2) @ n < 0:
                    e1, e2 = e2, e1
                self.quad(-n * half - half * (e1 + e2), 2 * half * e1, 2 * half * e2, mat)

    def inert(self, total):
        """Pads to `total` triangles with small ones beyond the box, facing away from it."""
        k = 0
        while len(self.tris) < total:
            x, y = -8.0 + 0.125 * (k % 128), -8.0 + 0.25 * (k // 128)
            t = np.zeros((), TRI_DTYPE)
            t["a"][:3], t["b"][:3], t["c"][:3] = (x, y, -25.0), (x, y + 0.1, -25.0), (x + 0.1, y, -25.0)  # normal -z
            self.tris.append(t)
            k += 1

    def scene(self, name, W, H, bounces, rays, env, textures=(), num_textures=None, frames=(0, 1), cam=(0, 0, 0),
              front=(0, 0, -1), right=(0.8, 0, 0), up=(0, 0.6, 0)):
        tris = np.array(self.tris, TRI_DTYPE) if self.tris else np.zeros(0, TRI_DTYPE)
        mats = np.array(self.mats, MAT_DTYPE) if self.mats else np.zeros(1, MAT_DTYPE)
        zero = (0.0, 0.0, 0.0)
        un = dict(width=W, height=H, numTriangles=len(tris), environmentalLight=int(env), maxBounceCount=bounces,
                  numRaysPerPixel=rays, numTextures=len(textures) if num_textures is None else num_textures,
                  cameraPos=tuple(map(float, cam)), viewportFront=tuple(map(float, front)),
                  viewportRight=tuple(map(float, right)), viewportUp=tuple(map(float, up)), pixelRight=zero,
                  pixelUp=zero, defocusDiskRight=zero, defocusDiskUp=zero)
        return dict(name=name, triangles=tris, materials=mats, textures=list(textures), uniforms=un, frames=frames)


def _pixel_rect(b, z, W, H, tx0, tx1, ty0, ty1, mat, uv=None, flip_u=False):
    """A quad in the plane z (camera at the origin looking down -z, viewport
    0.8 x 0.6) over the pixel centres tx0 .. tx1-1, ty0 .. ty1-1: its edges lie
    half a pixel off the centres."""
    sx, sy = 0.8 * -z * 2 / W, 0.6 * -z * 2 / H
    x0, x1 = (tx0 - W / 2 - 0.5) * sx, (tx1 - W / 2 - 0.5) * sx
    y0, y1 = (ty0 - H / 2 - 0.5) * sy, (ty1 - H / 2 - 0.5) * sy
    if uv is not None:
        (u0, v0), (u1, v1) = uv
        if flip_u:
            u0, u1 = u1, u0
        uv = [(u0, v0), (u1, v0), (u1, v1), (u0, v1)]
    b.quad((x0, y0, z), (x1 - x0, 0, 0), (0, y1 - y0, 0), mat, uv)


# --- sky -----------------------------------------------------------------------

def _sky_builder():
    """No triangle is ever hit: one inert triangle, so that every kernel and the BVH have something to hold."""
    b = _Builder()
    b.inert(1)
    return b


def sky_up():
    return _sky_builder().scene("sky_up", 64, 48, 4, 3, True, front=(0.1, 1.0, -0.1), right=(0.8, 0, 0), up=(0, 0, -0.6))


def sky_horizon():
    """Along the horizon: rows 0 .. 23 look below it."""
    return _sky_builder().scene("sky_horizon", 64, 48, 4, 3, True, front=HORIZON_FRONT)


def sky_sun():
    """Towards the sun's side; the nearest pixel stays about 0.2 rad off the
    sun: nearer, acos of an f32 dot product near 1 is the reference's own
    noise (0.15 rad keeps it under 3e-7 after the tonemap)."""
    f = np.array([0.6, 0.3, -0.2])
    f /= np.linalg.norm(f)
    r = np.cross(f, (0, 1, 0))
    r /= np.linalg.norm(r)
    u = np.cross(r, f)
    return _sky_builder().scene("sky_sun", 64, 48, 4, 3, True, front=f + 0.45 * r, right=0.25 * r, up=0.2 * u)


# --- lights -------------------------------------------------------------------

def emissive_ramp(rays=1):
    """16 light quads stacked in the plane z = -3, three pixel rows each."""
    b = _Builder()
    for k, s in enumerate(RAMP_STRENGTHS):
        _pixel_rect(b, -3.0, 64, 48, -1, 66, 3 * k, 3 * k + 3, b.light((1.0, 0.5, 0.25), s))
    return b.scene(f"emissive_ramp/r{rays}", 64, 48, 4, rays, False, frames=(0, 3))


# --- mirrors ------------------------------------------------------------------

def mirror_sky():
    b = _Builder()
    n = np.array([0.3, 0.5, 1.0])
    n /= np.linalg.norm(n)
    t1 = np.cross((0, 1, 0), n)
    t1 /= np.linalg.norm(t1)
    t2 = np.cross(n, t1)
    b.quad(np.array([0, 0, -4.0]) - 20 * (t1 + t2), 40 * t1, 40 * t2, b.mirror())
    return b.scene("mirror_sky", 64, 48, 4, 3, True)


def periscope():
    """Down -z onto a 45-degree mirror (plane y + z = -4), up onto a second one
    (y + z = 2), and down -z again onto four light patches that meet off the
    image's centre lines."""
    b = _Builder()
    m = b.mirror()
    b.quad((-4, -3, -1), (8, 0, 0), (0, 6, -6), m)    # normal (0, 1, 1)
    b.quad((-5, 9, -7), (10, 0, 0), (0, -8, 8), m)    # normal (0, -1, -1)
    cx, cy = 0.13, 6.09
    for k, (sx, sy) in enumerate(((-1, -1), (1, -1), (1, 1), (-1, 1))):
        col = ((1, 0.2, 0.1), (0.1, 1, 0.2), (0.2, 0.1, 1), (1, 0.9, 0.1))[k]
        p = (cx if sx > 0 else cx - 20, cy if sy > 0 else cy - 20, -14.0)
        b.quad(p, (20, 0, 0), (0, 20, 0), b.light(col, 0.3 + 0.4 * k))
    return b.scene("periscope", 64, 48, 6, 1, True)


def edge_highlight_mirror():
    """Camera -> 45-degree mirror -> up through a diffuse quad marked
    isEdgeHighlight (bounce 2: direction and rayColor kept) -> a light above
    it.  The quad covers x < 0.3 only; the light is seen unobstructed beside it."""
    b = _Builder()
    b.quad((-12, -7, 3), (24, 0, 0), (0, 14, -14), b.mirror())      # plane y + z = -4, fills the view
    # normal -y; it ends at z = -8, short of where a camera ray could reach y = 5 before the mirror
    b.quad((-6, 5, -8), (6.3, 0, 0), (0, 0, 8), b.material(DIFFUSE, color=(0.3, 1.0, 0.6), edge=1))
    b.quad((-9, 7, -14), (18, 0, 0), (0, 0, 16), b.light((1.0, 0.8, 0.6), 0.7))
    return b.scene("edge_highlight_mirror", 64, 48, 5, 1, True)


def edge_highlight_direct():
    """The same material seen directly (bounce 1) inside the emissive box: ordinary attenuation."""
    b = _Builder()
    b.box(10.0, b.light(*BOX_EMISSION))
    _pixel_rect(b, -3.0, 64, 48, 10, 50, 8, 40, b.material(DIFFUSE, color=(0.3, 1.0, 0.6), edge=1))
    return b.scene("edge_highlight_direct", 64, 48, 4, 3, False)


# --- glass (see "Glass distances" above) ---------------------------------------------

def _slab_front(b, glass):
    b.quad((-2.8, -2.2, -2.7), (5.6, 0, 0.5), (0, 4.4, -0.4), glass)


def glass_slab(bounces=12):
    b = _Builder()
    g = b.material(GLASS, color=(1.0, 0.8, 0.6), ior=1.5)
    _slab_front(b, g)
    b.quad((-2.8, -2.2, -3.2), (0, 4.4, -0.4), (5.6, 0, 0.5), g)    # the slab's far face looks away
    return b.scene(f"glass_slab/b{bounces}", 32, 24, bounces, 1, True, front=HORIZON_FRONT)


def glass_tir(bounces=12):
    """Behind the front face a second glass face, front towards the ray and 55
    degrees off the view axis: beyond the critical angle (41.8 degrees) for most
    of the rays that reach it with insideGlass set."""
    b = _Builder()
    g = b.material(GLASS, color=(1.0, 0.8, 0.6), ior=1.5)
    _slab_front(b, g)
    b.quad((0.5, -1.6, -3.9), (0, 3.2, 0), (-0.63, 0, 0.9), g)      # normal (0.819, 0, 0.574)
    return b.scene(f"glass_tir/b{bounces}", 32, 24, bounces, 1, True, front=HORIZON_FRONT)


def glass_low_index(bounces=12):
    """Index 0.8: eta = 1.25 on entry, k < 0 beyond 53.1 degrees.  Two faces
    with the critical band left out between them: one square to the view axis,
    met below 34 degrees (k > 0.5, refracted), and one 65 degrees off the axis,
    met beyond 69 degrees (k < -0.3, reflected on entry).  Within a pixel or two
    of k = 0 the refracted ray grazes the face (cos_t < 0.1) and the f32 error
    of the hit point, divided by cos_t, decides the 1e-6 test of the third
    re-hit: the reference's own noise, as with distant glass."""
    b = _Builder()
    g = b.material(GLASS, color=(0.7, 1.0, 0.9), ior=0.8)
    b.quad((-1.4, -1.0, -2.6), (1.5, 0, 0), (0, 2.0, 0), g)
    b.quad((0.8345, -1.2, -3.859), (0, 2.4, 0), (-0.6345, 0, 1.359), g)  # normal (0.906, 0, 0.423)
    return b.scene(f"glass_low_index/b{bounces}", 64, 48, bounces, 1, True, front=HORIZON_FRONT)


# --- checker ------------------------------------------------------------------------

def checker(scale=0.75):
    """A tilted quad through the origin, seen from z = 6 inside the box."""
    b = _Builder()
    b.box(10.0, b.light(*BOX_EMISSION))
    eu, ev = np.array([5.0, 0.8, -1.5]), np.array([-0.6, 4.0, 1.2])
    b.quad(np.array([0.1, 0.05, 0.0]) - (eu + ev) / 2, eu, ev, b.material(CHECKER, checker=scale))
    return b.scene(f"checker/s{scale:g}", 64, 48, 4, 1, False, cam=(0.3, 0.2, 6.0))


# --- textures -------------------------------------------------------------------------

def _textures():
    """8x5x3, 7x5x3 (21-byte rows: not a multiple of 4), 2x3x2 and 1x1x4.  The
    first channel of every texel GL sees is 255, so max(rayColor) stays 1 under
    any bilinear blend.  For the 7-wide texture GL's rows start every 24 bytes:
    the 255s are placed where GL reads a red byte, and its last row, which
    runs past the buffer (zeros: black texels), is kept out of the UVs used.  A
    3x2x2 texture (6-byte rows) would have such a black texel in its second and
    last row, so the two-channel texture is 2 wide and 3 high."""
    rng = np.random.default_rng(20240607)
    out = [rng.integers(0, 256, s, dtype=np.uint8) for s in ((5, 8, 3), (5, 7, 3), (3, 2, 2))]
    for t in out:
        h, w, ch = t.shape
        flat = t.reshape(-1)
        at = (np.arange(h)[:, None] * ((w * ch + 3) // 4 * 4) + np.arange(w)[None, :] * ch).reshape(-1)
        flat[at[at < flat.size]] = 255
    out.append(np.array([[[255, 90, 30, 128]]], np.uint8))
    return out


NUM_TEXTURES = 6   # numTextures; units 0..3 hold textures, unit 4 holds none
TEXTURE_SHAPES = {0: (8, 5), 1: (7, 5), 2: (2, 3), 3: (1, 1)}  # index -> (width, height)


def textures():
    """Coplanar textured quads at z = -3 inside the box (64 x 48):
         rows 24..47: A texture 0, UV -0.7 .. 2.6 | B texture 1 (unaligned rows), the same u | C (8 x 7 pixels)
                      texture 2, UVs around 1000;
         rows 10..23: D texture 0 with u mirrored | E texture 0 with pixel centres on texel centres, F the 1x1
                      texture | index -1 | index 7 >= numTextures | index 5 of 6 | unit 4, nothing bound;
         rows 0..9:   K texture 0 seen through a glass pane at z = -2.4."""
    b = _Builder()
    b.box(10.0, b.light(*BOX_EMISSION))
    tex = lambda i: b.material(TEXTURE, texture=i)
    wide = ((-0.7, -0.35), (1.9, 2.6))
    R = lambda *a, **k: _pixel_rect(b, -3.0, 64, 48, *a, **k)
    R(0, 28, 24, 48, tex(0), uv=wide)
    R(28, 56, 24, 48, tex(1), uv=((-0.7, 0.12), (1.9, 0.68)))   # rows 0..3 of texture 1 only
    R(56, 64, 24, 31, tex(2), uv=((997.53, 997.07), (1002.41, 1003.19)))
    R(56, 64, 31, 48, tex(3), uv=wide)
    R(0, 20, 10, 24, tex(0), uv=wide, flip_u=True)
    R(20, 28, 10, 15, tex(0), uv=((0.0, 0.0), (1.0, 1.0)))   # 8 x 5 pixels over 8 x 5 texels
    R(20, 28, 15, 24, tex(3), uv=wide)
    R(28, 36, 10, 24, tex(-1), uv=wide)
    R(36, 44, 10, 24, tex(7), uv=wide)
    R(44, 52, 10, 24, tex(5), uv=wide)
    R(52, 65, 10, 24, tex(4), uv=wide)
    R(-1, 65, -1, 10, tex(0), uv=wide)
    b.quad((-2.0, -1.6, -2.4), (4.0, 0, 0), (0, 0.73, 0), b.material(GLASS, color=(1.0, 0.8, 0.6), ior=1.5))
    return b.scene("textures", 64, 48, 6, 3, False, textures=_textures() + [None], num_textures=NUM_TEXTURES)


# --- all of it in one frame ----------------------------------------------------------

# Off the axes: at x = 0 or y = 0 exactly the checker's floor() would be decided by rounding.
COMPOSITE_CAMERA = (0.0137, 0.0071, 0.0)


def composite(total=0):
    """Mirror, glass, texture and checker patches and two lights in the plane
    z = -3 inside the box, padded with inert triangles to `total`."""
    b = _Builder()
    b.box(10.0, b.light(*BOX_EMISSION))
    R = lambda *a, **k: _pixel_rect(b, -3.0, 32, 24, *a, **k)
    R(-1, 8, 12, 25, b.mirror())
    R(8, 16, 12, 25, b.material(GLASS, color=(0.6, 0.8, 1.0), ior=1.5))
    R(16, 24, 12, 25, b.material(TEXTURE, texture=0), uv=((-0.7, -0.35), (1.9, 2.6)))
    R(24, 33, 12, 25, b.material(CHECKER, checker=0.75))
    R(-1, 16, -1, 12, b.light((0.2, 1.0, 0.4), 0.35))
    R(16, 33, -1, 12, b.light((1.0, 0.3, 0.9), 2.5))
    b.inert(total)
    return b.scene(f"composite/n{max(total, len(b.tris))}" if total else "composite", 32, 24, 6, 4, False,
                   textures=_textures()[:1], num_textures=1, cam=COMPOSITE_CAMERA)


def all_scenes():
    """name -> scene, every case of the table in DESIGN.md "Shading model"."""
    out = [sky_up(), sky_horizon(), sky_sun(), mirror_sky(), periscope(), edge_highlight_mirror(),
           edge_highlight_direct(), textures(), composite(), composite(1217), composite(8193)]
    out += [emissive_ramp(r) for r in (1, 3, 4)]
    out += [f(n) for f in (glass_slab, glass_tir, glass_low_index) for n in BOUNCE_LIMITS]
    out += [checker(s) for s in (0.75, 8.0, 0.0, -1.0)]
    return {s["name"]: s for s in out}
