"""Radiance queries (rt2_radiance_rays, rt2_path_rays, Scene.radiance_image) on
the GPU.  Every comparison is by bits over every ray.

  - against the oracle's trace() through one-pixel cameras (rays and stream
    states are rt2_path_rays_host's for the same uniforms; the query's linear
    colour goes through the oracle's tonemap), with the segment counts, on the
    matrix kernel (resident and L2 forms), the scalar kernel and the BVH walk,
    each query asserting which kernel ran;
  - raw records and stream states between the arms;
  - two chained samples against the oracle with numRaysPerPixel = 2, which
    pins the state a query leaves behind;
  - whole views through Scene.radiance_image against Scene.render_host,
    oracle.render and the float64 path model;
  - the move of at most 32 live lanes, rays outside the filter's range or not
    finite among ordinary ones, tmax, the device form, the counters and side
    effects.

The scenes, rays, seeds and references are those of tests/radiance_scenes.py;
tests/test_radiance_cpu.py asserts on the oracle alone what they are built to
give.
"""
import numpy as np
import pytest

import closest_hit_scenes as S
import radiance_scenes as R
import random_path_model as rm
import trace_rays_lib as T
from test_shading_model import scene_data, to_uniforms

pytestmark = pytest.mark.gpu

F32 = np.float32
ARMS = ("auto", "scalar", "bvh")
SENTINEL = 0xAB

_gpu = {}


def _scene(rt2mod, sc, arm):
    """(scene, triangles as uploaded, nodes or None), made once per scene and traversal."""
    key = (sc["name"].split("/")[0], arm == "bvh")
    if key not in _gpu:
        if arm == "bvh":
            sd = S.scene_data(sc["triangles"], sc["materials"])
            scene = rt2mod.Scene(sd)
            scene.set_traversal("bvh")
            up, nodes = sd.triangles().copy(), sd.nodes().copy()
        else:
            scene, up, nodes = rt2mod.Scene(triangles=sc["triangles"], materials=sc["materials"]), sc["triangles"], None
        if sc["textures"]:
            scene.set_textures(sc["textures"])
        _gpu[key] = (scene, up, nodes)
    return _gpu[key]


def _expected_kernel(rt2mod, scene, arm):
    if arm == "bvh":
        return rt2mod.RADIANCE_BVH
    if arm == "scalar":
        return rt2mod.RADIANCE_SCALAR
    return rt2mod.RADIANCE_RES if scene.n_tris <= 38 * 32 else rt2mod.RADIANCE_RES_L2


def _flags(rt2mod, arm):
    return rt2mod.TRACE_SCALAR if arm == "scalar" else rt2mod.TRACE_AUTO


def _radiance(rt2mod, scene, arm, o, d, rng, env, mb):
    before = np.array(rng, np.uint32)
    rec, out = scene.radiance(o, d, rng, mb, bool(env), _flags(rt2mod, arm))
    assert scene.last_kernel() == _expected_kernel(rt2mod, scene, arm), arm
    assert rec.dtype == rt2mod.RADIANCE_DTYPE and len(rec) == len(o) and out.dtype == np.uint32 and len(out) == len(o)
    assert np.array_equal(np.asarray(rng, np.uint32), before)  # the caller's array is not modified
    return rec, out


_rays = {}


def _camera(rt2mod, scene, sc, rng=None):
    """(o, d, state) of every ray of the scene from rt2_path_rays_host through
    its one-pixel camera: the render's own normalize(endPointJittered - o) and
    the stream after the camera's three draws.  The four pixels' rays are
    identical.  rng: the streams to go on from (one per ray) instead of a new
    seed."""
    n = len(sc["o"])
    o, d, state = np.zeros((n, 3), F32), np.zeros((n, 3), F32), np.zeros(n, np.uint32)
    for i in range(n):
        u = R.one_pixel_uniforms(rt2mod, sc["o"][i], sc["f"][i], 1, 1, 1, 0)
        p = int(sc["p"][i])
        if rng is None:
            rays, st = scene.path_rays(u, int(sc["frame"][i]))
            seeds = [(q + int(sc["frame"][i]) * R.MULT) & R.MASK for q in range(4)]
        else:
            seeds = [int(rng[i])] * 4
            rays, st = scene.path_rays(u, 12345, None, np.array(seeds, np.uint32))
        assert len(rays) == 4 and all(rays[q].tobytes() == rays[0].tobytes() for q in range(4))
        assert st.tolist() == [R.advance(s, 3) for s in seeds]
        assert np.array_equal(rays["o"][p], sc["o"][i]) and rays["tmax"][p] == 0 and rays["pad"][p] == 0
        o[i], d[i], state[i] = rays["o"][p], rays["d"][p], st[p]
    return o, d, state


def _device_rays(rt2mod, scene, sc):
    if sc["name"] not in _rays:
        got = _camera(rt2mod, scene, sc)
        for a in got:
            a.setflags(write=False)
        _rays[sc["name"]] = got
    return _rays[sc["name"]]


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _check(oraclemod, rec, rgb, segs, what):
    """The query's linear colour through main's sum, mean of one ray and tonemap against the oracle's pixel."""
    mine = R.tonemap(oraclemod, (F32(0) + rec["rgb"]) / F32(1))
    bad = (_bits(mine) != _bits(rgb)).any(1) | (rec["segments"] != segs)
    if bad.any():
        lines = [f"ray {i}: GPU {rec['rgb'][i]} -> {mine[i]} in {rec['segments'][i]} segments, reference {rgb[i]} in "
                 f"{segs[i]}" for i in np.flatnonzero(bad)[:6]]
        raise AssertionError(f"{what}: {int(bad.sum())} of {len(bad)} rays differ\n" + "\n".join(lines))


# ---- against the oracle through one-pixel cameras ---------------------------------------------------------------

@pytest.mark.parametrize("arm", ARMS)
@pytest.mark.parametrize("name", list(R.ORACLE_SCENES))
def test_against_the_oracle(rt2mod, oraclemod, name, arm):
    """1 triangle; the diverse Cornell box; the mirror corridor; 1,216
    triangles (all resident) and 1,217 (the last group from L2); 1, 63, 64, 65
    and 1,025 rays, with and without the sky, 1, 3 and 8 bounces."""
    sc = R.ORACLE_SCENES[name]()
    scene, up, nodes = _scene(rt2mod, sc, arm)
    o, d, state = _device_rays(rt2mod, scene, sc)
    for env, mb in R.SETTINGS:
        rgb, segs = R.oracle_radiance(oraclemod, rt2mod, sc, env, mb, "bvh" if arm == "bvh" else "brute",
                                      up if arm == "bvh" else None, nodes)
        whole = None
        for k in reversed(R.RAY_COUNTS):
            rec, out = _radiance(rt2mod, scene, arm, o[:k], d[:k], state[:k], env, mb)
            _check(oraclemod, rec, rgb[:k], segs[:k], f"{name} {arm} sky {env} max_bounce {mb}, {k} rays")
            if whole is None:
                whole = (rec, out)
            # a ray's record and stream do not depend on how many rays follow it
            assert rec.tobytes() == whole[0][:k].tobytes() and np.array_equal(out, whole[1][:k])
    if name == "soup1217" and arm == "auto":
        assert scene.last_kernel() == rt2mod.RADIANCE_RES_L2
    if name == "soup1216" and arm == "auto":
        assert scene.last_kernel() == rt2mod.RADIANCE_RES


@pytest.mark.parametrize("name", list(R.ORACLE_SCENES))
def test_arms_agree(rt2mod, name):
    """The matrix and the scalar kernel give the same bytes and leave the same
    stream states on every ray (the brute-force scan has one answer); without
    ties the BVH walk does too."""
    sc = R.ORACLE_SCENES[name]()
    scene, _, _ = _scene(rt2mod, sc, "auto")
    o, d, state = _device_rays(rt2mod, scene, sc)
    for env, mb in ((1, 8), (0, 3)):
        a, ra = _radiance(rt2mod, scene, "auto", o, d, state, env, mb)
        b, rb = _radiance(rt2mod, scene, "scalar", o, d, state, env, mb)
        assert a.tobytes() == b.tobytes() and np.array_equal(ra, rb), name
        assert (ra != state)[a["segments"] >= 2].all()  # a path that went on drew the roulette at least
        if name in R.TIE_FREE:
            bvh, _, _ = _scene(rt2mod, sc, "bvh")
            c, rc = _radiance(rt2mod, bvh, "bvh", o, d, state, env, mb)
            assert a.tobytes() == c.tobytes() and np.array_equal(ra, rc), name


@pytest.mark.parametrize("arm", ("auto", "scalar"))
def test_draws_of_exactly_one(rt2mod, oraclemod, arm):
    for name, (sc, which) in R.draw_is_one_rays().items():
        scene, _, _ = _scene(rt2mod, sc, arm)
        o, d, state = _device_rays(rt2mod, scene, sc)
        assert int(state[0]) == R.advance(sc["seed"], 3)
        rgb, segs = R.oracle_radiance(oraclemod, rt2mod, sc, 1, sc["max_bounce"])
        rec, _ = _radiance(rt2mod, scene, arm, o, d, state, 1, sc["max_bounce"])
        _check(oraclemod, rec, rgb, segs, f"{name} {arm}")


@pytest.mark.parametrize("arm", ARMS)
def test_two_chained_samples(rt2mod, oraclemod, arm):
    """numRaysPerPixel = 2 on the Cornell box: path_rays and radiance twice on
    one stream, summed, halved in binary32 and tonemapped, against the oracle's
    pixel.  A wrong state after the first sample gives another second path."""
    sc = R.cornell()
    scene, up, nodes = _scene(rt2mod, sc, arm)
    o1, d1, s1 = _device_rays(rt2mod, scene, sc)
    rec1, rng1 = _radiance(rt2mod, scene, arm, o1, d1, s1, 1, 8)
    o2, d2, s2 = _camera(rt2mod, scene, sc, rng1)
    rec2, _ = _radiance(rt2mod, scene, arm, o2, d2, s2, 1, 8)
    rgb, segs = R.oracle_radiance(oraclemod, rt2mod, sc, 1, 8, "bvh" if arm == "bvh" else "brute",
                                  up if arm == "bvh" else None, nodes, rays=2)
    total = (F32(0) + rec1["rgb"]) + rec2["rgb"]
    mine = R.tonemap(oraclemod, total / F32(2.0))
    assert np.array_equal(_bits(mine), _bits(rgb))
    assert np.array_equal(rec1["segments"] + rec2["segments"], segs)
    assert (rec2.tobytes() != rec1.tobytes()) and (rec2["segments"] != rec1["segments"]).any()


# ---- the move to lanes 0..31 ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("arm", ("auto", "scalar"))
@pytest.mark.parametrize("which", (0, 1))
def test_at_most_32_live_lanes(rt2mod, oraclemod, arm, which):
    """40 paths of a chunk end at bounce 1 and the 24 that go on sit in lanes
    40 to 63; or one lane alone goes on, lane 37.  The live lanes are moved to
    lanes 0 .. and every record and stream state lands at its own index."""
    full = R.cornell()
    idx = R.compaction_chunks(oraclemod, rt2mod)[which]
    sc = R.picked(full, idx, f"rad_cornell/picked{which}")
    scene, _, _ = _scene(rt2mod, sc, arm)
    o, d, state = _device_rays(rt2mod, scene, sc)
    rgb, segs = R.oracle_radiance(oraclemod, rt2mod, full, 1, 8)
    rec, out = _radiance(rt2mod, scene, arm, o, d, state, 1, 8)
    _check(oraclemod, rec, rgb[idx], segs[idx], f"compaction chunk {which} {arm}")
    if which == 0:
        assert (rec["segments"][:40] == 1).all() and (rec["segments"][40:] >= 3).all()
    else:
        assert (rec["segments"] >= 2).sum() == 1 and rec["segments"][37] >= 3
    # every lane's stream is its own: the state left is the whole set's for that ray
    fo, fd, fs = _device_rays(rt2mod, scene, full)
    _, whole = _radiance(rt2mod, scene, arm, fo, fd, fs, 1, 8)
    assert np.array_equal(out, whole[idx])
    # and behind a full chunk, in the second wave's place
    both, both_out = _radiance(rt2mod, scene, arm, np.concatenate([fo[:64], o]), np.concatenate([fd[:64], d]),
                               np.concatenate([fs[:64], state]), 1, 8)
    assert both[64:].tobytes() == rec.tobytes() and np.array_equal(both_out[64:], out)


# ---- whole views ------------------------------------------------------------------------------------------------

def _view_gpu(rt2mod, scene):
    key = ("view", scene["name"].split("/")[1])
    if key not in _gpu:
        _gpu[key] = rt2mod.Scene(triangles=scene["triangles"], materials=scene["materials"])
    return _gpu[key]


@pytest.mark.parametrize("rays", R.VIEW_RAYS)
@pytest.mark.parametrize("w,h", R.VIEW_SIZES)
@pytest.mark.parametrize("name", sorted(R.VIEW_SCENES))
def test_radiance_image(rt2mod, oraclemod, name, w, h, rays):
    scene = R.view(name, w, h, rays)
    gpu = _view_gpu(rt2mod, scene)
    u = to_uniforms(rt2mod, scene["uniforms"])
    model = rm.model_for(scene)
    first, count = scene["frames"]
    rows = np.arange(h, dtype=np.int32)
    sh = rt2mod.shard(2, 1, 3)
    part_rows = rt2mod.shard_row_ids(h, sh)
    frames = []
    for frame in range(first, first + count):
        gpu.stats(reset=True)
        img, segs = gpu.radiance_image(u, frame)
        qs = gpu.stats(reset=True)
        assert gpu.last_kernel() == rt2mod.RADIANCE_RES
        assert img.shape == (h, w, 3) and img.dtype == F32 and segs.shape == (h, w)
        tm = R.tonemap(oraclemod, img)
        ren = gpu.render_host(u, frame, 1)
        rs_ = gpu.stats(reset=True)
        acc, _, osegs, _ = oraclemod.render(scene["triangles"], scene["materials"], u, rows, frame, 1, "brute")
        assert np.array_equal(_bits(tm), _bits(ren[..., :3])), f"{name}: radiance_image against render_host"
        assert np.array_equal(_bits(tm), _bits(acc[..., :3])), f"{name}: radiance_image against the oracle"
        assert int(segs.sum()) == osegs == rs_.segments == qs.segments
        part, part_segs = gpu.radiance_image(u, frame, sh)
        assert part.shape == (len(part_rows), w, 3)
        assert np.array_equal(_bits(part), _bits(img[part_rows])) and np.array_equal(part_segs, segs[part_rows])
        other, other_segs = gpu.radiance_image(u, frame, None, rt2mod.TRACE_SCALAR)
        assert gpu.last_kernel() == rt2mod.RADIANCE_SCALAR
        assert np.array_equal(_bits(other), _bits(img)) and np.array_equal(other_segs, segs)
        frames.append(tm)
        if rays == 1:
            # the state a path leaves: the pixel's seed advanced by the model's number of draws
            r, st = gpu.path_rays(u, frame)
            rec, out = gpu.radiance(r["o"], r["d"], st, int(u.maxBounceCount), bool(u.environmentalLight))
            assert np.array_equal(_bits(rec["rgb"].reshape(h, w, 3)), _bits(img))
            draws = model.draws[frame - first]
            compared = 0
            for y in range(h):
                for x in range(w):
                    if model.excluded[y, x]:
                        continue
                    seed = int(rm.first_seed(x, y, w, frame))
                    want = oraclemod.pcg_sequence(seed, int(draws[y, x]) + 1)[-1][0]
                    got = oraclemod.pcg_sequence(int(out[y * w + x]), 1)[0][0]
                    assert got == want and int(out[y * w + x]) == R.advance(seed, draws[y, x]), (x, y)
                    compared += 1
            assert compared >= 0.97 * w * h
    total = np.zeros((h, w, 3), F32)
    for tm in frames:
        total = total + tm
    rm.assert_image(model, total / F32(count), f"radiance_image, {rays} rays")
    rm.assert_exclusions(model)


# ---- rays outside the filter's range or not finite among ordinary ones ---------------------------------------

MIXED = {"far": (5,), "long": (40,), "nan": (41,), "inf": (50,), "all": (5, 40, 41, 50)}


def _soup_rays(n):
    sc = R.soup(1217)
    rng = ((np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(97)) & np.uint64(R.MASK)).astype(np.uint32)
    return sc, sc["o"][:n].copy(), sc["f"][:n].copy(), rng


def _mixed_rays(which):
    """Two chunks of the 1,217-triangle soup's rays; in the first, lane 5 far
    outside the filter's range (2^21), lane 40 unnormalised, lane 41 a NaN
    origin, lane 50 an infinite direction component."""
    _, o, d, rng = _soup_rays(128)
    for lane in MIXED[which]:
        if lane == 5:
            o[5] = (T.FAR, 5.0, 10.0)
        elif lane == 40:
            d[40] *= F32(3)
        elif lane == 41:
            o[41, 0] = np.nan
        else:
            d[50, 1] = np.inf
    return o, d, rng


@pytest.mark.parametrize("arm", ("auto", "scalar"))
@pytest.mark.parametrize("which", list(MIXED))
def test_mixed_waves(rt2mod, which, arm):
    sc, o0, d0, rng = _soup_rays(128)
    scene, _, _ = _scene(rt2mod, sc, arm)
    base, base_out = _radiance(rt2mod, scene, arm, o0, d0, rng, 1, 8)
    o, d, _ = _mixed_rays(which)
    rec, out = _radiance(rt2mod, scene, arm, o, d, rng, 1, 8)
    others = np.setdiff1d(np.arange(128), MIXED[which])
    assert (base["segments"][others] >= 2).sum() >= 32
    assert np.array_equal(rec[others].view(np.uint8), base[others].view(np.uint8))  # undisturbed, every byte
    assert np.array_equal(out[others], base_out[others])
    # both kernels: equal where both are numbers, NaN in the same components; the same streams
    other, other_out = scene.radiance(o, d, rng, 8, True, _flags(rt2mod, "scalar" if arm == "auto" else "auto"))
    assert np.array_equal(rec["segments"], other["segments"]) and np.array_equal(out, other_out)
    nan_a, nan_b = np.isnan(rec["rgb"]), np.isnan(other["rgb"])
    assert np.array_equal(nan_a, nan_b)
    assert np.array_equal(_bits(rec["rgb"])[~nan_a], _bits(other["rgb"])[~nan_a])


def test_tmax_is_not_used(rt2mod):
    """tmax = 0, half the primary hit distance and a NaN: identical output."""
    import torch
    n = 193
    sc, o, d, rng = _soup_rays(n)
    for arm in ("auto", "scalar"):
        scene, _, _ = _scene(rt2mod, sc, arm)
        dst, tri = scene.trace_rays(o, d)
        assert (tri >= 0).sum() >= 48
        want, want_rng = _radiance(rt2mod, scene, arm, o, d, rng, 1, 8)
        for tmax in (np.zeros(n, F32), np.where(tri >= 0, dst * F32(0.5), F32(0.25)).astype(F32),
                     np.full(n, np.nan, F32)):
            rays = np.zeros(n, rt2mod.RAY_DTYPE)
            rays["o"], rays["d"], rays["tmax"] = o, d, tmax
            d_rays = torch.from_numpy(rays.view(np.uint8).copy()).to("cuda")
            d_rng = torch.from_numpy(rng.view(np.int32).copy()).to("cuda")
            d_out = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            scene.radiance_device(d_rays.data_ptr(), n, d_rng.data_ptr(), d_out.data_ptr(), 8, True,
                                  _flags(rt2mod, arm), torch.cuda.current_stream().cuda_stream)
            assert d_out.cpu().numpy().tobytes() == want.tobytes(), arm
            assert d_rng.cpu().numpy().view(np.uint32).tolist() == want_rng.tolist(), arm


# ---- device form, counters, side effects --------------------------------------------------------------------------

@pytest.mark.parametrize("arm", ARMS)
def test_device_form_guard_regions_and_stats(rt2mod, arm):
    """rt2_radiance_rays on a non-default stream with torch tensors: the host
    form's bytes; nothing before record 0 or after record n of either output is
    written, n = 0 writes nothing, and stats().segments is the sum of the
    records'."""
    import torch
    n, guard = 193, 5
    sc, o, d, rng = _soup_rays(n)
    scene, _, _ = _scene(rt2mod, sc, arm)
    rays = np.zeros(n, rt2mod.RAY_DTYPE)
    rays["o"], rays["d"] = o, d
    host, host_rng = _radiance(rt2mod, scene, arm, o, d, rng, 1, 8)
    guarded_rng = np.concatenate([np.full(guard, 0xABABABAB, np.uint32), rng, np.full(guard, 0xABABABAB, np.uint32)])
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        d_rays = torch.from_numpy(rays.view(np.uint8).copy()).to("cuda", non_blocking=False)
        d_buf = torch.full(((n + 2 * guard) * 16,), SENTINEL, dtype=torch.uint8, device="cuda")
        d_out = d_buf[guard * 16:]
        d_rng_buf = torch.from_numpy(guarded_rng.view(np.int32).copy()).to("cuda")
        d_rng = d_rng_buf[guard:]
        st.synchronize()
        scene.radiance_device(d_rays.data_ptr(), 0, d_rng.data_ptr(), d_out.data_ptr(), 8, True, _flags(rt2mod, arm),
                              st.cuda_stream)
        st.synchronize()
        assert (d_buf.cpu().numpy() == SENTINEL).all()
        assert d_rng_buf.cpu().numpy().view(np.uint32).tolist() == guarded_rng.tolist()
        for k in (1, 65, n):
            d_buf.fill_(SENTINEL)
            d_rng_buf.copy_(torch.from_numpy(guarded_rng.view(np.int32).copy()))
            st.synchronize()
            scene.stats(reset=True)
            scene.radiance_device(d_rays.data_ptr(), k, d_rng.data_ptr(), d_out.data_ptr(), 8, True,
                                  _flags(rt2mod, arm), st.cuda_stream)
            st.synchronize()
            assert scene.last_kernel() == _expected_kernel(rt2mod, scene, arm)
            got = d_buf.cpu().numpy()
            assert (got[:guard * 16] == SENTINEL).all(), k
            assert got[guard * 16:(guard + k) * 16].tobytes() == host[:k].tobytes(), k
            assert (got[(guard + k) * 16:] == SENTINEL).all(), k
            got_rng = d_rng_buf.cpu().numpy().view(np.uint32)
            assert got_rng[:guard].tolist() == guarded_rng[:guard].tolist(), k
            assert got_rng[guard:guard + k].tolist() == host_rng[:k].tolist(), k
            assert got_rng[guard + k:].tolist() == guarded_rng[guard + k:].tolist(), k  # the streams not run, untouched
            stats = scene.stats(reset=True)
            assert stats.segments == int(host["segments"][:k].sum()), k
            if arm == "bvh":
                assert 0 < stats.tests < stats.segments * 1217 and stats.node_visits > 0
            else:
                assert stats.tests == stats.segments * 1217 and stats.node_visits == 0


def test_path_rays_of_a_view_and_its_shard(rt2mod):
    """The device form over a whole 67 x 10 view and a shard's rows: reseeding
    gives x + y * width + frame * M advanced by three draws per pixel, going on
    from given states advances those, and nothing outside the slab's records is
    written."""
    import torch
    scene = R.view("jitter_defocus_ramp", 67, 10, 1)
    gpu = _view_gpu(rt2mod, scene)
    u = to_uniforms(rt2mod, scene["uniforms"])
    w, h, frame = 67, 10, 0xFFFFFFFE
    rays, st = gpu.path_rays(u, frame)
    ys, xs = np.divmod(np.arange(w * h), w)
    assert st.tolist() == [R.advance(int(rm.first_seed(x, y, w, frame)), 3) for x, y in zip(xs, ys)]
    assert len({r.tobytes() for r in rays}) == w * h and (rays["tmax"] == 0).all() and (rays["pad"] == 0).all()
    assert np.allclose(np.linalg.norm(rays["d"], axis=1), 1.0, atol=1e-6)
    rays2, st2 = gpu.path_rays(u, 7, None, st)
    assert st2.tolist() == [R.advance(int(s), 3) for s in st] and rays2.tobytes() != rays.tobytes()
    sh = rt2mod.shard(2, 1, 3)
    rows = rt2mod.shard_row_ids(h, sh)
    part, part_st = gpu.path_rays(u, frame, sh)
    pick = (rows[:, None] * w + np.arange(w)[None]).reshape(-1)
    assert part.tobytes() == rays[pick].tobytes() and np.array_equal(part_st, st[pick])
    n, guard = len(pick), 3
    d_rays = torch.full(((n + 2 * guard) * 32,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_rng = torch.full((n + 2 * guard,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    gpu.path_rays_device(u, frame, sh, True, d_rng[guard:].data_ptr(), d_rays[guard * 32:].data_ptr(),
                         torch.cuda.current_stream().cuda_stream)
    got, got_rng = d_rays.cpu().numpy(), d_rng.cpu().numpy()
    assert (got[:guard * 32] == SENTINEL).all() and (got[(guard + n) * 32:] == SENTINEL).all()
    assert got[guard * 32:(guard + n) * 32].tobytes() == part.tobytes()
    assert (got_rng[:guard] == 0x5A5A5A5A).all() and (got_rng[guard + n:] == 0x5A5A5A5A).all()
    assert np.array_equal(got_rng[guard:guard + n].view(np.uint32), part_st)


def test_render_unchanged_by_queries(rt2mod):
    """One index-coded image before the queries and one after them on the same scene: identical bits."""
    n = 1217
    tris, mats = S.coded_scene("soup", n)
    w, h = S.SIZES[n]
    u = S.coded_uniforms(w, h, n)
    scene = rt2mod.Scene(triangles=tris, materials=mats)
    before = scene.render_host(u, 0, 1)
    _, o, d, rng = _soup_rays(193)
    a, ra = scene.radiance(o, d, rng, 8, True)
    b, rb = scene.radiance(o, d, rng, 8, True, rt2mod.TRACE_SCALAR)
    assert a.tobytes() == b.tobytes() and np.array_equal(ra, rb) and (a["segments"] >= 1).all()
    scene.radiance_image(u, 3)
    after = scene.render_host(u, 0, 1)
    assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
