"""Linear renders (rt2_render_linear, rt2_render_linear_host,
rt2_resolve_tonemap) on the GPU.  Every comparison is by bits over every pixel,
so NaNs compare too.

The yardstick is the oracle-pinned query chain with RT2_TRACE_SCALAR
(linear_lib.chain_samples: Scene.path_rays and Scene.radiance per sample on one
stream array) with the sums formed in numpy float32 exactly as include/rt2.h
states them (linear_lib.accumulate).  u.numTextures is the number of bound
images (none here), so the render's texture rule and the queries' coincide.

tests/test_linear_cpu.py asserts on the oracle alone what the views are built
to give.
"""
import numpy as np
import pytest

import closest_hit_scenes as S
import linear_lib as LL
import radiance_scenes as R
from test_shading_model import to_uniforms

pytestmark = pytest.mark.gpu

F32 = np.float32
POISON = 0x5A5A5A5A
GUARD = 8  # pixels before and after each device array
TWINS = [(0, "brute"), (136, "brute"), (86, "brute"), (92, "brute"), (227, "brute"), (353, "brute"), (354, "brute"),
         (355, "brute"), (356, "brute"), (380, "brute"), (109, "bvh")]

_gpu, _yard = {}, {}


def _shard_key(sh):
    return None if sh is None else (sh.tile_rows, sh.rank, sh.nranks)


def _guarded(n):
    import torch
    buf = torch.full(((n + 2 * GUARD) * 4,), POISON, dtype=torch.int32, device="cuda")
    mid = buf[GUARD * 4:(GUARD + n) * 4]
    return buf, mid


def _read(buf, n):
    got = buf.cpu().numpy().view(np.uint32)
    assert (got[:GUARD * 4] == POISON).all() and (got[(GUARD + n) * 4:] == POISON).all(), "guard region written"
    return got[GUARD * 4:(GUARD + n) * 4].view(F32).reshape(n, 4).copy()


def _linear(rt2mod, scene, u, calls, sh=None, moments=True):
    """rt2_render_linear over zeroed device arrays between poisoned guards, one
    call per (frame_begin, frame_count) of `calls` into the same arrays, on a
    stream of its own.  Returns (sum, sumsq or None) as float32 [n][4]; the
    guards are checked and .w is 0.0."""
    import torch
    sh = sh or rt2mod.shard()
    n = rt2mod.shard_rows(u.height, sh) * u.width
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        bs, ms = _guarded(n)
        bq, mq = _guarded(n)
        ms.zero_()
        if moments:
            mq.zero_()
        st.synchronize()
        for f0, fc in calls:
            scene.render_linear(u, f0, fc, sh, ms.data_ptr(), mq.data_ptr() if moments else 0, st.cuda_stream)
        st.synchronize()
        total = _read(bs, n)
        sq = _read(bq, n)
    assert (LL.bits(total[:, 3]) == 0).all()
    if moments:
        assert (LL.bits(sq[:, 3]) == 0).all()
        return total, sq
    assert (sq.view(np.uint32) == POISON).all(), "a null d_sumsq: the moment array is not touched"
    return total, None


def _yardstick(rt2mod, key, scene, u, f0, fc, sh=None):
    """(sum, sumsq, segments) of the query chain; once per key, read-only."""
    k = (key, u.width, u.height, u.numRaysPerPixel, u.maxBounceCount, f0, fc, _shard_key(sh))
    if k not in _yard:
        v, segs = LL.chain_samples(rt2mod, scene, u, f0, fc, sh)
        total, sq = LL.accumulate(v)
        total.setflags(write=False)
        sq.setflags(write=False)
        _yard[k] = (total, sq, segs)
    return _yard[k]


def _same(got, want, what):
    bad = (LL.bits(got) != LL.bits(want)).any(1)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {len(bad)} pixels differ; pixel {i}: {got[i]} against "
                             f"{want[i]}")


# ---- config B's scene, every twin --------------------------------------------------------------------------------------

def _config_b(rt2mod, config_scene, traversal):
    if ("B", traversal) not in _gpu:
        sd, spec = config_scene("B")
        scene = rt2mod.Scene(sd)
        if traversal == "bvh":
            scene.set_traversal("bvh")
        _gpu["B", traversal] = (scene, sd, spec)
    scene, sd, spec = _gpu["B", traversal]
    return scene, rt2mod.offline_uniforms(96, 54, spec.bounces, 4, sd.num_triangles)


@pytest.mark.parametrize("split", (True, False))
@pytest.mark.parametrize("variant,traversal", TWINS)
def test_twins_equal_the_yardstick(rt2mod, config_scene, variant, traversal, split):
    """Config B's scene at 96 x 54, 4 rays, frames 1 and 2, the whole image and
    the shard {2, 1, 3}: sums and moments equal the yardstick on every pixel,
    the kernel is the forced variant's twin, and the segments counted are
    rt2_render's for the same call."""
    import torch
    scene, u = _config_b(rt2mod, config_scene, traversal)
    scene.set_frame_split(split)
    try:
        assert scene.set_variant(variant) == variant
        for sh in (None, rt2mod.shard(2, 1, 3)):
            want, want2, segs = _yardstick(rt2mod, ("B", traversal), scene, u, 1, 2, sh)
            assert np.isfinite(want).all() and (want[:, :3] > 0).mean() > 0.5 and (want2[:, :3] > 0).mean() > 0.5
            shd = sh or rt2mod.shard()
            n = rt2mod.shard_rows(u.height, shd) * u.width
            acc = torch.zeros(n * 4, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            scene.stats(reset=True)
            scene.render(u, 1, 2, shd, acc.data_ptr())
            ren = scene.stats(reset=True)
            parent = scene.last_kernel()  # 0 is the automatic choice: whatever rt2_render takes for this call
            assert parent == variant or (variant == 0 and parent in (353, 354))
            got, got2 = _linear(rt2mod, scene, u, [(1, 2)], sh)
            assert scene.last_kernel() == rt2mod.LINEAR_TWIN + parent
            lin = scene.stats(reset=True)
            _same(got, want, f"sums, variant {variant}, split {split}")
            _same(got2, want2, f"moments, variant {variant}, split {split}")
            assert (lin.samples, lin.segments, lin.tests, lin.node_visits) == \
                   (ren.samples, ren.segments, ren.tests, ren.node_visits)
            assert lin.segments == segs and lin.samples == n * 4 * 2
    finally:
        scene.set_variant(0)
        scene.set_frame_split(True)


def test_cost_order_changes_nothing(rt2mod, config_scene):
    """Two consecutive linear renders with cost_order on (the second one takes
    its pixel order from the first one's cost map): the yardstick's bits."""
    scene, u = _config_b(rt2mod, config_scene, "brute")
    want, want2, _ = _yardstick(rt2mod, ("B", "brute"), scene, u, 1, 2, None)
    scene.set_cost_order(True)
    try:
        for k in range(2):
            got, got2 = _linear(rt2mod, scene, u, [(1, 2)])
            _same(got, want, f"sums, cost-ordered render {k}")
            _same(got2, want2, f"moments, cost-ordered render {k}")
        assert scene.cost_map() is not None
    finally:
        scene.set_cost_order(False)


def test_automatic_selection(rt2mod, config_scene):
    """With no variant forced the twin chosen is 1000 + the variant rt2_render
    chooses for the same call: on config B's scene and on the 1,217-triangle
    soup, which takes the L2 form."""
    scene, u = _config_b(rt2mod, config_scene, "brute")
    scene.set_variant(0)
    scene.render_host(u, 0, 1)
    chosen = scene.last_kernel()
    assert chosen in (353, 354)
    scene.render_linear_host(u, 0, 1)
    assert scene.last_kernel() == rt2mod.LINEAR_TWIN + chosen
    n = 1217
    tris, mats = S.coded_scene("soup", n)
    w, h = S.SIZES[n]
    us = S.coded_uniforms(w, h, n)
    soup = rt2mod.Scene(triangles=tris, materials=mats)
    soup.render_host(us, 0, 1)
    chosen = soup.last_kernel()
    assert chosen in (355, 356)
    soup.render_linear_host(us, 0, 1, moments=True)
    assert soup.last_kernel() == rt2mod.LINEAR_TWIN + chosen


# ---- small shapes where the sink can go wrong -------------------------------------------------------------------------

def _view_gpu(rt2mod, sc):
    key = ("view", sc["name"].split("/")[1] if "/" in sc["name"] else sc["name"])
    if key not in _gpu:
        _gpu[key] = rt2mod.Scene(triangles=sc["triangles"], materials=sc["materials"])
    return key, _gpu[key]


def _view_uniforms(rt2mod, sc, rays, bounces):
    assert not [t for t in sc["textures"] if t is not None]
    return to_uniforms(rt2mod, dict(sc["uniforms"], numRaysPerPixel=rays, maxBounceCount=bounces, numTextures=0))


@pytest.mark.parametrize("w,h", R.VIEW_SIZES)
@pytest.mark.parametrize("name", sorted(R.VIEW_SCENES))
def test_small_views(rt2mod, name, w, h):
    """67 x 10 and 64 x 4 views; 1, 3 and 65 rays (one item outlives its wave's
    other lanes: path states are compacted and moved while a moment is
    half-summed); 1 and 8 bounces, and 0, which gives all-zero sums.  The
    automatic twin, and the tiled and L2-reading twins, which move states too."""
    sc = R.view(name, w, h, 1)
    key, gpu = _view_gpu(rt2mod, sc)
    try:
        for rays in LL.SMALL_RAYS:
            for bounces in LL.SMALL_BOUNCES:
                u = _view_uniforms(rt2mod, sc, rays, bounces)
                f0, fc = (5, 2) if rays < 65 else (0xFFFFFFFE, 1)
                want, want2, _ = _yardstick(rt2mod, key, gpu, u, f0, fc)
                for variant in (0, 380, 227):
                    gpu.set_variant(variant)
                    got, got2 = _linear(rt2mod, gpu, u, [(f0, fc)])
                    assert gpu.last_kernel() in ((1353, 1354) if variant == 0 else (1000 + variant,))
                    _same(got, want, f"{name} sums, {rays} rays, {bounces} bounces, variant {variant}")
                    _same(got2, want2, f"{name} moments, {rays} rays, {bounces} bounces, variant {variant}")
        gpu.set_variant(0)
        zero, zero2 = _linear(rt2mod, gpu, _view_uniforms(rt2mod, sc, 3, 0), [(5, 2)])
        assert not LL.bits(zero).any() and not LL.bits(zero2).any()
    finally:
        gpu.set_variant(0)


@pytest.mark.parametrize("rays", (3, 65))
def test_corridor(rt2mod, rays):
    """The facing mirrors: the lanes of a wave end at different bounces."""
    sc = LL.corridor_view(64, 4, rays)
    key, gpu = _view_gpu(rt2mod, sc)
    u = _view_uniforms(rt2mod, sc, rays, 8)
    want, want2, segs = _yardstick(rt2mod, key, gpu, u, 3, 1)
    assert segs > 1.5 * 64 * 4 * rays
    for split in (True, False):
        gpu.set_frame_split(split)
        got, got2 = _linear(rt2mod, gpu, u, [(3, 1)])
        _same(got, want, f"corridor sums, {rays} rays")
        _same(got2, want2, f"corridor moments, {rays} rays")
    gpu.set_frame_split(True)


# ---- frame order -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("split", (True, False))
def test_frame_order(rt2mod, config_scene, split):
    """Frames 0 .. 3 in one call, in two calls of two and in four calls of one
    into the same arrays: the same bits, which are the yardstick's."""
    scene, u = _config_b(rt2mod, config_scene, "brute")
    u.numRaysPerPixel = 2
    scene.set_frame_split(split)
    try:
        one, one2 = _linear(rt2mod, scene, u, [(0, 4)])
        two, two2 = _linear(rt2mod, scene, u, [(0, 2), (2, 2)])
        four, four2 = _linear(rt2mod, scene, u, [(0, 1), (1, 1), (2, 1), (3, 1)])
    finally:
        scene.set_frame_split(True)
    _same(two, one, "sums, two calls")
    _same(two2, one2, "moments, two calls")
    _same(four, one, "sums, four calls")
    _same(four2, one2, "moments, four calls")
    want, want2, _ = _yardstick(rt2mod, ("B", "brute"), scene, u, 0, 4)
    _same(one, want, "sums, four frames")
    _same(one2, want2, "moments, four frames")


# ---- the tonemap path ---------------------------------------------------------------------------------------------------

def _tonemapped(rt2mod, gpu, u, frame):
    """resolve_tonemap (in place, frames = 1) of a one-frame linear sum, (n, 4)."""
    import torch
    n = u.width * u.height
    d = torch.zeros(n * 4, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    gpu.render_linear(u, frame, 1, rt2mod.shard(), d.data_ptr(), 0, stream)
    rt2mod.resolve_tonemap(d.data_ptr(), n, 1, d.data_ptr(), stream)
    return d.cpu().numpy().reshape(n, 4)


@pytest.mark.parametrize("name,w,h", LL.TONEMAP_VIEWS)
def test_tonemap_path(rt2mod, oraclemod, name, w, h):
    """One frame: resolve_tonemap of the linear sum is render_host's image on
    every pixel, and oracle.render's.  Three frames: the float32 sum of three
    one-frame resolves reproduces rt2_render's accumulator."""
    sc = R.view(name, w, h, LL.TONEMAP_RAYS)
    _, gpu = _view_gpu(rt2mod, sc)
    u = _view_uniforms(rt2mod, sc, LL.TONEMAP_RAYS, sc["uniforms"]["maxBounceCount"])
    first, count = LL.TONEMAP_FRAMES
    rows = np.arange(h, dtype=np.int32)
    total = np.zeros((w * h, 3), F32)
    for frame in range(first, first + count):
        tm = _tonemapped(rt2mod, gpu, u, frame)
        ren = gpu.render_host(u, frame, 1).reshape(-1, 4)
        assert np.array_equal(LL.bits(tm), LL.bits(ren)), f"{name}: frame {frame} against render_host"
        acc, _, _, _ = oraclemod.render(sc["triangles"], sc["materials"], u, rows, frame, 1, "brute")
        assert np.array_equal(LL.bits(tm[:, :3]), LL.bits(acc[..., :3].reshape(-1, 3))), f"{name}: against the oracle"
        total = (total + tm[:, :3]).astype(F32)
    ren = gpu.render_host(u, first, count).reshape(-1, 4)
    assert np.array_equal(LL.bits(total / F32(count)), LL.bits(ren[:, :3])), f"{name}: {count} frames"


# ---- the moments mean something --------------------------------------------------------------------------------------

def test_second_moment_bounds_the_mean(rt2mod, config_scene):
    """meansq >= mean^2 (1 - 2^-20) per channel wherever both are finite:
    Jensen's inequality, less the rounding of at most 4 samples' sums and the
    two divisions (under 12 * 2^-24 relative).  One frame of config B's scene
    through the blocking form, and the views."""
    scene, u = _config_b(rt2mod, config_scene, "brute")
    cases = [(scene, u)]
    for name in sorted(R.VIEW_SCENES):
        sc = R.view(name, 67, 10, 1)
        cases.append((_view_gpu(rt2mod, sc)[1], _view_uniforms(rt2mod, sc, 3, 8)))
    spread = 0
    for gpu, uu in cases:
        mean, meansq = gpu.render_linear_host(uu, 2, 1, moments=True)
        assert mean.shape == (uu.height, uu.width, 4) and mean.dtype == F32 and meansq.shape == mean.shape
        assert (mean[..., 3] == 1).all() and (meansq[..., 3] == 1).all()
        m, q = mean[..., :3].astype(np.float64), meansq[..., :3].astype(np.float64)
        ok = np.isfinite(m) & np.isfinite(q)
        assert ok.mean() > 0.99
        assert (q[ok] >= m[ok] * m[ok] * (1 - 2.0 ** -20)).all()
        spread += int((q[ok] > m[ok] * m[ok] * 1.01).sum())
        only = gpu.render_linear_host(uu, 2, 1)
        assert np.array_equal(LL.bits(only), LL.bits(mean))
    assert spread > 1000  # and the samples of many pixels do differ


def test_constant_samples(rt2mod):
    """Every path of a pixel returns the same value (one emissive triangle, no
    sky, no jitter): meansq == mean * mean wherever that product is exact."""
    sc = LL.constant_view()
    _, gpu = _view_gpu(rt2mod, sc)
    u = _view_uniforms(rt2mod, sc, 4, 4)
    mean, meansq = gpu.render_linear_host(u, 0, 2, moments=True)
    m = mean[..., :3]
    lit = (m != 0).any(-1)
    assert 0.1 < lit.mean() < 0.9
    assert np.array_equal(LL.bits(m[lit]), LL.bits(np.broadcast_to(np.array(LL.CONSTANT_EMISSION, F32), m[lit].shape)))
    exact = (m.astype(np.float64) * m.astype(np.float64)) == (m * m).astype(np.float64)
    assert exact.all()
    assert np.array_equal(LL.bits(meansq[..., :3]), LL.bits(m * m))


# ---- robustness, existing behaviour -------------------------------------------------------------------------------------

def test_null_moments_give_the_same_sums(rt2mod, config_scene):
    """d_sumsq = NULL: a poisoned moment array stays as it is (checked in
    _linear) and the sums are those of the call with moments."""
    scene, u = _config_b(rt2mod, config_scene, "brute")
    for split in (True, False):
        scene.set_frame_split(split)
        with_m, _ = _linear(rt2mod, scene, u, [(1, 2)])
        without, none = _linear(rt2mod, scene, u, [(1, 2)], moments=False)
        assert none is None
        _same(without, with_m, f"sums without moments, split {split}")
    scene.set_frame_split(True)
    part, _ = _linear(rt2mod, scene, u, [(1, 2)], rt2mod.shard(2, 1, 3), moments=False)
    pick = (rt2mod.shard_row_ids(u.height, rt2mod.shard(2, 1, 3))[:, None] * u.width + np.arange(u.width)[None])
    _same(part, with_m[pick.reshape(-1)], "the shard's rows of the whole image")


def test_renders_and_linear_renders_do_not_disturb_each_other(rt2mod, config_scene):
    """A render, a linear render and a render on one scene give the bits each
    gives alone on a scene of its own; render_host's images (float and 8-bit)
    before and after a linear render are identical."""
    sd, spec = config_scene("B")
    u = rt2mod.offline_uniforms(96, 54, spec.bounces, 4, sd.num_triangles)
    alone_r, alone_r8 = rt2mod.Scene(sd).render_host(u, 1, 2, rgb8=True)
    alone_l, alone_l2 = rt2mod.Scene(sd).render_linear_host(u, 1, 2, moments=True)
    scene = rt2mod.Scene(sd)
    before, before8 = scene.render_host(u, 1, 2, rgb8=True)
    lin, lin2 = scene.render_linear_host(u, 1, 2, moments=True)
    after, after8 = scene.render_host(u, 1, 2, rgb8=True)
    assert np.array_equal(LL.bits(before), LL.bits(alone_r)) and np.array_equal(before8, alone_r8)
    assert np.array_equal(LL.bits(after), LL.bits(before)) and np.array_equal(after8, before8)
    assert np.array_equal(LL.bits(lin), LL.bits(alone_l)) and np.array_equal(LL.bits(lin2), LL.bits(alone_l2))
    want, want2, _ = _yardstick(rt2mod, ("B", "brute"), _config_b(rt2mod, config_scene, "brute")[0], u, 1, 2)
    assert np.array_equal(LL.bits(lin[..., :3].reshape(-1, 3)), LL.bits(want[:, :3] / F32(2)))
    assert np.array_equal(LL.bits(lin2[..., :3].reshape(-1, 3)), LL.bits(want2[:, :3] / F32(2)))
