"""Linear renders without a GPU: the C-ABI's symbols and argument checks, the
numpy statement of the accumulation rule that tests/test_gpu_linear.py uses as
its yardstick helper, and on the oracle alone the premises of that file's views
(the tonemap saturates few of the compared values; the corridor's lanes end at
different bounces; the constant view is constant), so none of its tests passes
vacuously."""
import ctypes as C

import numpy as np

import linear_lib as LL
import radiance_scenes as R
from test_shading_model import to_uniforms

F32 = np.float32


def test_symbols_and_abi(rt2mod):
    L = rt2mod.lib()
    assert L.rt2_abi_version() == 4  # the entry points only add to the interface
    for name in ("rt2_render_linear", "rt2_render_linear_host", "rt2_resolve_tonemap"):
        assert hasattr(L, name) and name in rt2mod.EXPORTED
    for f in ("render_linear", "render_linear_host", "radiance_image"):
        assert callable(getattr(rt2mod.Scene, f))
    assert callable(rt2mod.resolve_tonemap) and rt2mod.LINEAR_TWIN == 1000
    # every variant the launcher chooses on its own has a twin named after it; a twin cannot be forced
    for v in (136, 86, 92, 109, 227, 353, 354, 355, 356, 380):
        name, twin = L.rt2_variant_name(v), L.rt2_variant_name(1000 + v)
        assert name is not None and twin == name + b"/lin", v
    assert L.rt2_variant_name(1000) is None
    assert "render_linear_host" in rt2mod.Scene.radiance_image.__doc__


def _fake_scene():
    """Zeroed memory in place of a scene: nothing on a device."""
    buf = C.create_string_buffer(8192)
    return buf, C.c_void_p(C.addressof(buf))


def test_argument_validation(rt2mod):
    """Every bad argument returns < 0 with a message before any device call
    (there is no device here; `fake` is no scene)."""
    L = rt2mod.lib()
    keep, fake = _fake_scene()
    buf = np.full(64 + 8, 0xAB, np.uint8)
    base = buf.ctypes.data + (-buf.ctypes.data) % 16
    sh = rt2mod.shard()

    def uni(**kw):
        v = rt2mod.offline_uniforms(4, 2, 8, 2, 0)
        for k, x in kw.items():
            setattr(v, k, x)
        return C.byref(v)

    good = uni()
    bad_both = [(None, good, sh, base, base), (fake, None, sh, base, base), (fake, good, sh, None, base),
                (fake, good, sh, None, None), (fake, uni(numRaysPerPixel=0), sh, base, None),
                (fake, uni(numRaysPerPixel=-2), sh, base, base), (fake, uni(width=0), sh, base, None),
                (fake, uni(height=0), sh, base, None), (fake, good, rt2mod.shard(0, 0, 1), base, None),
                (fake, good, rt2mod.shard(1, 2, 2), base, None), (fake, good, rt2mod.shard(1, -1, 2), base, None),
                (fake, uni(basicShading=1), sh, base, None), (fake, uni(basicShading=1, numRaysPerPixel=0), sh, base, base)]
    bad_dev = bad_both + [(fake, good, sh, base + 4, None), (fake, good, sh, base + 8, base),
                          (fake, good, sh, base, base + 4), (fake, good, sh, base, base + 12)]
    for s, up, shd, a, b in bad_dev:
        L.rt2_scene_create(None, 0, None, 0, None, 0, 0, None)  # leaves another message behind
        assert L.rt2_render_linear(s, up, 0, 1, shd, a, b, None) < 0, (a, b)
        assert b"rt2_render_linear: bad argument" in L.rt2_last_error()
        assert L.rt2_render_linear(s, up, 0, 0, shd, a, b, None) < 0  # whatever the frame count
    for s, up, shd, a, b in bad_both:
        L.rt2_scene_create(None, 0, None, 0, None, 0, 0, None)
        assert L.rt2_render_linear_host(s, up, 0, 1, shd, a, b) < 0, (a, b)
        assert b"rt2_render_linear_host: bad argument" in L.rt2_last_error()
    # the host form takes any alignment: with no frames it returns before it would touch a device
    assert L.rt2_render_linear_host(fake, good, 0, 0, sh, base + 4, base + 12) == 0
    # frame_count == 0 or an empty slab: nothing to do, nothing launched
    assert L.rt2_render_linear(fake, good, 7, 0, sh, base, base, None) == 0
    assert L.rt2_render_linear(fake, good, 7, 0, sh, base, None, None) == 0
    empty = rt2mod.shard(2, 1, 2)  # the 2 rows are rank 0's
    assert rt2mod.shard_rows(2, empty) == 0
    assert L.rt2_render_linear(fake, good, 0, 3, empty, base, base, None) == 0
    assert L.rt2_render_linear_host(fake, good, 0, 3, empty, base, base) == 0
    # the resolve: rt2_resolve_rgba32f's rules
    for a, n, fr, o in ((None, 4, 1, base), (base, 4, 1, None), (base, -1, 1, base), (base, 4, 0, base)):
        L.rt2_scene_create(None, 0, None, 0, None, 0, 0, None)
        assert L.rt2_resolve_tonemap(a, n, fr, o, None) < 0
        assert b"rt2_resolve_tonemap: bad argument" in L.rt2_last_error()
    assert L.rt2_resolve_tonemap(base, 0, 1, base, None) == 0
    # a twin's id is not a variant to force
    assert L.rt2_scene_set_variant(fake, 1353) < 0 and b"linear twin" in L.rt2_last_error()
    assert (buf == 0xAB).all() and not any(keep.raw)


def test_accumulation_rule():
    """The helper is the header's rule: the product is rounded before it is
    added (a value whose fused form differs), frames continue a given sum, and
    the fourth float is 0."""
    x = F32(1) + F32(2.0 ** -12)            # x * x = 1 + 2^-11 + 2^-24: rounds to 1 + 2^-11
    big = F32(2.0 ** 24)
    v = np.zeros((1, 2, 1, 3), F32)
    v[0, 0, 0] = (big, 3.0, 0.5)
    v[0, 1, 0] = (x, 4.0, 0.25)
    s, q = LL.accumulate(v)
    assert s.shape == (1, 4) and s.dtype == F32 and q.dtype == F32 and s[0, 3] == 0 and q[0, 3] == 0
    assert s[0, 1] == F32(3.5) and s[0, 2] == F32(0.375)
    assert q[0, 1] == F32(12.5) and q[0, 2] == F32((0.25 + 0.0625) / 2)
    assert s[0, 0] == (big + x) / F32(2)
    # q.x = RN(RN(big * big) + RN(x * x)) / 2; a fused multiply-add would add the unrounded x * x
    rounded = F32(F32(big * big) + F32(x * x))
    assert q[0, 0] == rounded / F32(2)
    y = F32(1) + F32(2.0 ** -23)
    w = np.zeros((1, 2, 1, 3), F32)
    w[0, 0, 0, 0], w[0, 1, 0, 0] = F32(2.0 ** -12), y
    _, q2 = LL.accumulate(w)
    fused = F32(np.float64(F32(2.0 ** -24)) + np.float64(y) * np.float64(y))
    plain = F32(F32(2.0 ** -24) + F32(y * y))
    assert fused != plain and q2[0, 0] == plain / F32(2)
    # two frames in one call = one frame after the other into the same sums
    rng = np.random.default_rng(5)
    many = rng.uniform(0, 9, (2, 3, 7, 3)).astype(F32)
    a, a2 = LL.accumulate(many)
    b, b2 = LL.accumulate(many[:1])
    b, b2 = LL.accumulate(many[1:], b, b2)
    assert np.array_equal(LL.bits(a), LL.bits(b)) and np.array_equal(LL.bits(a2), LL.bits(b2))
    # a NaN sample stays a NaN in its own pixel and channel only
    many[0, 1, 2, 1] = np.nan
    a, a2 = LL.accumulate(many)
    assert np.isnan(a[2, 1]) and np.isnan(a2[2, 1]) and np.isnan(a).sum() == 1 and np.isnan(a2).sum() == 1


def test_the_tonemap_saturates_few_values(rt2mod, oraclemod):
    """In every view the GPU file compares through the tonemap at most 10 % of
    the channel values of oracle.render are exactly 1.0 (the ceiling rule of
    tests/test_radiance_cpu.py), and the image is not black."""
    first, count = LL.TONEMAP_FRAMES
    worst = {}
    for name, w, h in LL.TONEMAP_VIEWS:
        scene = R.view(name, w, h, LL.TONEMAP_RAYS)
        u = to_uniforms(rt2mod, scene["uniforms"])
        u.numTextures = 0
        rows = np.arange(h, dtype=np.int32)
        for frame in range(first, first + count):
            acc, _, _, _ = oraclemod.render(scene["triangles"], scene["materials"], u, rows, frame, 1, "brute")
            frac = float((acc[..., :3] == 1.0).mean())
            worst[name, w, h] = max(worst.get((name, w, h), 0.0), frac)
            assert frac <= 0.10, (name, w, h, frame, frac)
            assert (acc[..., :3] > 0).mean() > 0.25, (name, w, h, frame)
    print(worst)


def test_view_premises(rt2mod, oraclemod):
    """The corridor view's first wave of pixels ends its paths at several
    different bounces; the constant view's pixels are the emission or 0."""
    sc = LL.corridor_view(64, 4, 1)
    u = to_uniforms(rt2mod, sc["uniforms"])
    xs, ys = np.arange(64, dtype=np.int32), np.zeros(64, np.int32)
    counts = set()
    for x, y in zip(xs, ys):
        _, _, s, _ = oraclemod.render_pixels(sc["triangles"], sc["materials"], u, [int(x)], [int(y)], 0, 1, threads=1)
        counts.add(int(s))
    assert len(counts) >= 4 and min(counts) == 1, counts
    _, _, total, _ = oraclemod.render(sc["triangles"], sc["materials"], u, np.arange(4, dtype=np.int32), 0, 1, "brute")
    assert total > 1.5 * 64 * 4  # and on average a path goes on past its first hit
    cv = LL.constant_view()
    uc = to_uniforms(rt2mod, cv["uniforms"])
    acc, _, _, _ = oraclemod.render(cv["triangles"], cv["materials"], uc, np.arange(uc.height, dtype=np.int32), 0, 1,
                                    "brute")
    want = R.tonemap(oraclemod, np.array(LL.CONSTANT_EMISSION, F32))
    lit = (acc[..., :3] != 0).any(-1)
    assert 0.1 < lit.mean() < 0.9 and len(cv["triangles"]) == 1
    assert np.array_equal(LL.bits(acc[lit][:, :3]), LL.bits(np.broadcast_to(want, (int(lit.sum()), 3))))
    for e in LL.CONSTANT_EMISSION:  # e * e is exact in binary32
        assert float(F32(e) * F32(e)) == float(e) * float(e)
