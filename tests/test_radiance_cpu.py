"""Radiance queries without a GPU: the C-ABI's layouts, symbols and argument
checks, and the premises of tests/test_gpu_radiance.py on the CPU oracle alone
(the one-pixel camera gives trace() for one ray and four seeds; the tonemap
saturates few of the compared rays; the ray sets reach every branch of trace;
the compaction chunks and the frames with a draw of 1.0 hold what those tests
say they hold), so none of them passes vacuously."""
import ctypes as C

import numpy as np
import pytest

import radiance_scenes as R
import random_path_model as rm
import shading_scenes as ss

F32 = np.float32


def test_layouts_symbols_and_codes(rt2mod):
    s = rt2mod.RADIANCE_DTYPE
    assert s.itemsize == 16 and s.fields["rgb"][1] == 0 and s.fields["segments"][1] == 12  # one 16-byte store
    assert s.fields["rgb"][0].shape == (3,) and s.fields["segments"][0] == np.dtype("<i4")
    o = rt2mod.PathOpts
    assert C.sizeof(o) == 16 and (o.max_bounce.offset, o.environmental_light.offset, o.pad.offset) == (0, 4, 8)
    po = rt2mod.path_opts(5, False)
    assert (po.max_bounce, po.environmental_light, list(po.pad)) == (5, 0, [0, 0])
    L = rt2mod.lib()
    assert L.rt2_abi_version() == 4  # the entry points only add to the interface
    for name in ("rt2_radiance_rays", "rt2_radiance_rays_host", "rt2_path_rays", "rt2_path_rays_host"):
        assert hasattr(L, name) and name in rt2mod.EXPORTED
    codes = (rt2mod.RADIANCE_RES, rt2mod.RADIANCE_RES_L2, rt2mod.RADIANCE_SCALAR, rt2mod.RADIANCE_BVH)
    assert codes == (-18, -19, -20, -21)  # the next four after the shading queries'
    assert min(rt2mod.SHADE_RES, rt2mod.SHADE_RES_L2, rt2mod.SHADE_SCALAR, rt2mod.SHADE_BVH) == -17
    for f in ("radiance", "radiance_device", "path_rays", "path_rays_device", "radiance_image"):
        assert callable(getattr(rt2mod.Scene, f))


def _fake_scene():
    """Zeroed memory in place of a scene: brute-force traversal, no nodes, nothing on a device."""
    buf = C.create_string_buffer(4096)
    return buf, C.c_void_p(C.addressof(buf))


def test_radiance_argument_validation(rt2mod):
    """Every bad argument returns < 0 with "bad argument" before any device
    call (there is no device here; `fake` is no scene)."""
    L = rt2mod.lib()
    rays = np.zeros(4, rt2mod.RAY_DTYPE)
    rng = np.full(8, 0xAAAAAAAA, np.uint32)
    out = np.full(6 * 16, 0xAA, np.uint8).view(rt2mod.RADIANCE_DTYPE)
    pr, pg, po = rays.ctypes.data, rng.ctypes.data, out.ctypes.data
    assert pr % 16 == 0 and po % 16 == 0 and pg % 4 == 0
    keep, fake = _fake_scene()
    good = rt2mod.path_opts(8, True)

    def opts(**kw):
        o = rt2mod.path_opts(8, True)
        for k, v in kw.items():
            if k.startswith("pad"):
                o.pad[int(k[3])] = v
            else:
                setattr(o, k, v)
        return o

    g = C.byref(good)
    bad_opts = [opts(pad0=1), opts(pad1=-1), opts(max_bounce=0), opts(max_bounce=-3), opts(max_bounce=257)]
    bad_both = [(None, pr, 4, g, pg, po, 0), (fake, pr, 4, None, pg, po, 0), (fake, pr, -1, g, pg, po, 0),
                (fake, None, 4, g, pg, po, 0), (fake, pr, 4, g, None, po, 0), (fake, pr, 4, g, pg, None, 0),
                (fake, pr, 4, g, pg, po, 2), (fake, pr, 4, g, pg, po, -1)]
    bad_both += [(fake, pr, 4, C.byref(b), pg, po, 0) for b in bad_opts]
    bad_dev = bad_both + [(fake, pr + 4, 4, g, pg, po, 0), (fake, pr + 8, 4, g, pg, po, 0),
                          (fake, pr, 4, g, pg, po + 8, 0), (fake, pr, 4, g, pg, po + 4, 0),
                          (fake, pr, 4, g, pg + 1, po, 0), (fake, pr, 4, g, pg + 2, po, 0)]
    for s, r, n, op, rg, o, fl in bad_dev:
        L.rt2_scene_create(None, 0, None, 0, None, 0, 0, None)  # leaves another message behind
        assert L.rt2_radiance_rays(s, r, n, op, rg, o, fl, None) < 0, (r, n, rg, o, fl)
        assert b"rt2_radiance_rays: bad argument" in L.rt2_last_error()
    for s, r, n, op, rg, o, fl in bad_both:
        L.rt2_scene_create(None, 0, None, 0, None, 0, 0, None)
        assert L.rt2_radiance_rays_host(s, r, n, op, rg, o, fl) < 0, (r, n, rg, o, fl)
        assert b"rt2_radiance_rays_host: bad argument" in L.rt2_last_error()
    # a null scene or options, bad options: whatever n
    for op in (None, C.byref(bad_opts[0]), C.byref(bad_opts[2])):
        assert L.rt2_radiance_rays(fake, None, 0, op, None, None, 0, None) < 0
        assert L.rt2_radiance_rays_host(fake, None, 0, op, None, None, 0) < 0
    assert L.rt2_radiance_rays(None, None, 0, g, None, None, 0, None) < 0
    # rng needs 4 bytes only: an address that is no multiple of 16 is an argument like any other (n = 0 here)
    for mb in (1, 256):
        assert L.rt2_radiance_rays(fake, None, 0, C.byref(opts(max_bounce=mb)), None, None, 0, None) == 0
    # n = 0: nothing to do, nothing launched (no device here to launch on)
    assert L.rt2_radiance_rays(fake, None, 0, g, None, None, 0, None) == 0
    assert L.rt2_radiance_rays(fake, pr, 0, g, pg + 4, po, rt2mod.TRACE_SCALAR, None) == 0
    assert L.rt2_radiance_rays_host(fake, None, 0, g, None, None, 0) == 0
    assert (out.view(np.uint8) == 0xAA).all() and (rng == 0xAAAAAAAA).all()
    # BVH traversal on a scene without nodes: rt2_scene_set_traversal refuses to bring a scene there
    assert L.rt2_scene_set_traversal(fake, 1) < 0
    assert b"BVH traversal needs the node array" in L.rt2_last_error()
    assert not any(keep.raw)


def test_path_rays_argument_validation(rt2mod):
    """rt2_camera_rays' bad arguments and a null or misaligned rng."""
    L = rt2mod.lib()
    keep, fake = _fake_scene()
    rays = np.zeros(4, rt2mod.RAY_DTYPE)
    rng = np.zeros(8, np.uint32)
    pr, pg = rays.ctypes.data, rng.ctypes.data
    u = R.one_pixel_uniforms(rt2mod, (0, 0, 0), (0, 0, -1), 1, 1, 8, 0)
    ub = C.byref(u)
    sh = rt2mod.shard()

    def uni(**kw):
        v = R.one_pixel_uniforms(rt2mod, (0, 0, 0), (0, 0, -1), 1, 1, 8, 0)
        for k, x in kw.items():
            setattr(v, k, x)
        return C.byref(v)

    bad_both = [(None, ub, sh, pg, pr), (fake, None, sh, pg, pr), (fake, uni(width=0), sh, pg, pr),
                (fake, uni(height=0), sh, pg, pr), (fake, ub, rt2mod.shard(0, 0, 1), pg, pr),
                (fake, ub, rt2mod.shard(1, 2, 2), pg, pr), (fake, ub, sh, None, pr), (fake, ub, sh, pg, None)]
    bad_dev = bad_both + [(fake, ub, sh, pg + 2, pr), (fake, ub, sh, pg + 1, pr), (fake, ub, sh, pg, pr + 8)]
    for s, up, shd, rg, r in bad_dev:
        for reseed in (0, 1):
            L.rt2_scene_create(None, 0, None, 0, None, 0, 0, None)
            assert L.rt2_path_rays(s, up, shd, 3, reseed, rg, r, None) < 0, (rg, r)
            assert b"rt2_path_rays: bad argument" in L.rt2_last_error()
    for s, up, shd, rg, r in bad_both:
        L.rt2_scene_create(None, 0, None, 0, None, 0, 0, None)
        assert L.rt2_path_rays_host(s, up, shd, 3, 1, rg, r) < 0, (rg, r)
        assert b"rt2_path_rays_host: bad argument" in L.rt2_last_error()
    # an empty slab: nothing to do, whatever the pointers
    empty = rt2mod.shard(2, 1, 2)  # the 2 rows are rank 0's
    assert rt2mod.shard_rows(2, empty) == 0
    assert L.rt2_path_rays(fake, ub, empty, 0, 1, None, None, None) == 0
    assert L.rt2_path_rays_host(fake, ub, empty, 0, 1, None, None) == 0
    assert not any(keep.raw)


# ---- the one-pixel camera ---------------------------------------------------------------------------------------

def test_frame_for_inverts_the_seed():
    for seed in (0, 1, 0xFFFFFFFF, 0x80000000, 123456789):
        for p in range(4):
            f = R.frame_for(seed, p)
            assert 0 <= f < 2 ** 32 and (p + f * R.MULT) & R.MASK == seed
            assert int(rm.first_seed(p % 2, p // 2, 2, f)) == seed
    p, frame = R.default_seeds(1025, 1)
    seeds = R.seed_of(p, frame)
    assert seeds[0] == 0 and seeds[1] == 0xFFFFFFFF and rm.frame_term_wraps(frame[2])
    assert np.mean([rm.frame_term_wraps(f) for f in frame]) > 0.9 and len(set(seeds.tolist())) > 1000


def test_one_pixel_premise(rt2mod, oraclemod):
    """Four pixels, the same ray, seeds p + frame * M: on a floor that scatters,
    the four pixels of one frame differ (each has its own stream), and pixel p
    at frame_for(seed, p) gives the same colour and segments for every p."""
    b = ss._Builder()
    b.quad((-50, -1, 50), (100, 0, 0), (0, 0, -100), b.material(ss.DIFFUSE, color=(0.9, 0.6, 0.3)))
    sc0 = b.scene("premise", 2, 2, 8, 1, True)
    o, f = (0.0, 0.0, 0.0), (0.1, -1.0, -0.3)
    u = R.one_pixel_uniforms(rt2mod, o, f, len(sc0["triangles"]), 1, 4, 0)

    def pixel(p, frame):
        acc, _, s, _ = oraclemod.render_pixels(sc0["triangles"], sc0["materials"], u, [p % 2], [p // 2], frame, 1,
                                               threads=1)
        return acc[0, :3].copy(), s

    same_frame = [pixel(p, 77)[0] for p in range(4)]
    assert len({c.tobytes() for c in same_frame}) == 4
    for seed in (0, 0xFFFFFFFF, 424242):
        got = [pixel(p, R.frame_for(seed, p)) for p in range(4)]
        assert len({c.tobytes() for c, _ in got}) == 1 and len({s for _, s in got}) == 1
        assert got[0][1] >= 2 and got[0][0].max() > 0  # it scattered and found the sky
    # R = 2: the second sample goes on from the first one's stream, so it is not the first again
    u2 = R.one_pixel_uniforms(rt2mod, o, f, len(sc0["triangles"]), 1, 4, 0, 2)
    acc2, _, s2, _ = oraclemod.render_pixels(sc0["triangles"], sc0["materials"], u2, [0], [0], 77, 1, threads=1)
    assert acc2[0, :3].tobytes() != same_frame[0].tobytes() and s2 >= 3


# ---- saturation, branch coverage ---------------------------------------------------------------------------------

COMPARED = [(name, env, mb) for name in R.ORACLE_SCENES for env, mb in R.SETTINGS]


def test_the_tonemap_saturates_few_rays(rt2mod, oraclemod):
    """On every compared ray set at most 10 % of the rays have a channel at 1.0
    after the tonemap: the comparison against the oracle sees the others'
    values below the tonemap's ceiling."""
    worst = {}
    for name, env, mb in COMPARED:
        sc = R.ORACLE_SCENES[name]()
        rgb, _ = R.oracle_radiance(oraclemod, rt2mod, sc, env, mb)
        if env and mb == 8:  # nor a black reference: with the sky on, paths that leave the scene bring light back
            assert (rgb.max(1) > 0.05).mean() > 0.05, (name, env, mb)
        for k in R.RAY_COUNTS:
            frac = float((rgb[:k] >= 1.0).any(1).mean())
            worst[name] = max(worst.get(name, 0.0), frac)
            assert frac <= 0.10, (name, env, mb, k, frac)
    rgb, _ = R.oracle_radiance(oraclemod, rt2mod, R.cornell(), 1, 8, rays=2)
    assert float((rgb >= 1.0).any(1).mean()) <= 0.10
    print(worst)


def test_ray_sets_reach_every_branch(rt2mod, oraclemod):
    """Every entry of radiance_scenes.BRANCHES is met by some ray of the oracle
    scenes.  The branches are named by a binary32 walk whose segment counts
    must equal the oracle's: only rays where they do are counted, and at least
    95 % must."""
    seen = {}
    for name, get in R.ORACLE_SCENES.items():
        sc = get()
        assert len(sc["o"]) == 1025
        for env, mb in ((1, 8), (0, 3)):
            events, segs, _ = R.walk(oraclemod, sc, env, mb)
            _, ref = R.oracle_radiance(oraclemod, rt2mod, sc, env, mb)
            same = segs == ref
            assert same.mean() >= 0.95, (name, env, mb, float(same.mean()))
            for i in np.flatnonzero(same):
                for e in events[i]:
                    seen.setdefault(e, set()).add(name)
    for branch in R.BRANCHES:
        assert branch in seen, f"no ray reaches: {branch}"
    print({k: sorted(v) for k, v in seen.items()})


def test_soup_rays_hit_the_group_read_from_l2(rt2mod, oraclemod):
    sc = R.soup(1217)
    d = (sc["f"] / np.linalg.norm(sc["f"], axis=1, keepdims=True)).astype(F32)
    _, tri, _, _ = oraclemod.closest_hits(sc["triangles"], sc["o"], d)
    assert (tri[:63] >= 1216).sum() >= 4 and (tri >= 1216).sum() >= 8
    assert len(R.soup(1216)["triangles"]) == 38 * 32  # every group resident


def test_corridor_lanes_end_at_different_bounces(rt2mod, oraclemod):
    _, segs = R.oracle_radiance(oraclemod, rt2mod, R.corridor(), 1, 8)
    assert set(range(1, 7)) <= set(segs[:64].tolist())


def test_compaction_chunks(rt2mod, oraclemod):
    _, segs = R.oracle_radiance(oraclemod, rt2mod, R.cornell(), 1, 8)
    first, second = R.compaction_chunks(oraclemod, rt2mod)
    assert len(first) == 64 and (segs[first[:40]] == 1).all() and (segs[first[40:]] >= 3).all()
    assert len(second) == 64 and (segs[second] >= 2).sum() == 1 and segs[second[37]] >= 3
    assert len(set(first.tolist())) == 64 and len(set(second.tolist())) == 64


def test_draws_of_exactly_one(rt2mod, oraclemod):
    """The three frames of random_scenes at which a draw is 1.0, as rays of the
    one-pixel camera: the seed's draw number `draw` is 1.0, and the walk names
    what follows (the probability draw declines the specular bounce, the
    roulette's draw survives at p = 1)."""
    for name, (sc, which) in R.draw_is_one_rays().items():
        seq = oraclemod.pcg_sequence(sc["seed"], which["draw"])
        assert seq[-1][1] == 1.0 and all(v < 1.0 for _, v in seq[:-1]), name
        assert int(R.seed_of(sc["p"], sc["frame"])[0]) == sc["seed"]
        events, segs, _ = R.walk(oraclemod, sc, 1, sc["max_bounce"])
        _, ref = R.oracle_radiance(oraclemod, rt2mod, sc, 1, sc["max_bounce"])
        assert segs[0] == ref[0], name
        if name == "probability_is_one":
            assert events[0][0] == "specular declined"
        if name == "roulette_is_one":
            assert events[0][0] == "specular bounce" and segs[0] >= 2


# ---- whole views ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", R.VIEW_SIZES)
@pytest.mark.parametrize("name", sorted(R.VIEW_SCENES))
def test_views_meet_the_models_rule(rt2mod, oraclemod, name, w, h):
    """The resized views keep the path model's premises: few pixels excluded,
    and the oracle's own image passes the rule."""
    from test_random_paths import oracle_image
    for rays in R.VIEW_RAYS:
        scene = R.view(name, w, h, rays)
        model = rm.model_for(scene)
        rm.assert_exclusions(model)
        img, segs = oracle_image(oraclemod, rt2mod, scene)
        rm.assert_image(model, img, "oracle")
        if not model.excluded.any():
            assert segs == int(model.segments.sum())
