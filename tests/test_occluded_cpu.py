"""Occlusion queries without a GPU: the C-ABI's symbols and argument checks,
and the premises of tests/test_gpu_occluded.py on the CPU oracle alone (the
picket rays' accepting sets, the chunks' compositions, occluded and unoccluded
rays in every soup, bounds that flip what they claim to flip), so none of
those tests can pass vacuously."""
import ctypes as C

import numpy as np
import pytest

import closest_hit_scenes as S
import occluded_lib as O
import trace_rays_lib as T

F32 = np.float32


def test_symbols_and_codes(rt2mod):
    L = rt2mod.lib()
    assert L.rt2_abi_version() == 4  # the entry points only add to the interface
    for name in ("rt2_occluded", "rt2_occluded_host"):
        assert hasattr(L, name) and name in rt2mod.EXPORTED
    occ = (rt2mod.OCCLUDED_RES, rt2mod.OCCLUDED_RES_L2, rt2mod.OCCLUDED_SCALAR, rt2mod.OCCLUDED_BVH)
    qry = (rt2mod.QUERY_RES, rt2mod.QUERY_RES_L2, rt2mod.QUERY_SCALAR, rt2mod.QUERY_BVH)
    assert len(set(occ + qry)) == 8 and all(c < -1 for c in occ)  # -1 is the preview, >= 0 a render's variant
    assert callable(rt2mod.Scene.occluded) and callable(rt2mod.Scene.occluded_device)


def test_argument_validation(rt2mod):
    """Bad arguments return < 0 with "bad argument" before any device call
    (and before the scene is read: `fake` is no scene)."""
    L = rt2mod.lib()
    rays = np.zeros(4, rt2mod.RAY_DTYPE)
    out = np.full(8, 0xAA, np.uint8)
    pr, po = rays.ctypes.data, out.ctypes.data
    assert pr % 16 == 0
    buf = C.create_string_buffer(4096)
    fake = C.c_void_p(C.addressof(buf))
    bad_dev = [(None, pr, 4, po, 0), (fake, pr, -1, po, 0), (fake, None, 4, po, 0), (fake, pr, 4, None, 0),
               (fake, pr, 4, po, 2), (fake, pr, 4, po, -1), (fake, pr + 4, 4, po, 0), (fake, pr + 8, 4, po, 0)]
    for s, r, n, o, fl in bad_dev:
        L.rt2_scene_create(None, 0, None, 0, None, 0, 0, None)  # leaves another message behind
        assert L.rt2_occluded(s, r, n, o, fl, None) < 0, (r, n, o, fl)
        assert b"rt2_occluded: bad argument" in L.rt2_last_error()
    for s, r, n, o, fl in bad_dev[:6]:
        L.rt2_scene_create(None, 0, None, 0, None, 0, 0, None)
        assert L.rt2_occluded_host(s, r, n, o, fl) < 0, (r, n, o, fl)
        assert b"rt2_occluded_host: bad argument" in L.rt2_last_error()
    assert L.rt2_occluded(None, None, 0, None, 0, None) < 0  # a null scene, whatever n
    assert L.rt2_occluded_host(None, None, 0, None, 0) < 0
    # n = 0: nothing to do, nothing launched (no device here to launch on); the output may sit at any address
    assert L.rt2_occluded(fake, None, 0, None, 0, None) == 0
    assert L.rt2_occluded(fake, pr, 0, po + 1, rt2mod.TRACE_SCALAR, None) == 0
    assert L.rt2_occluded_host(fake, None, 0, None, 0) == 0
    assert (out == 0xAA).all()


# ---- premises -------------------------------------------------------------------------------------------------

def test_picket_rays_accepting_sets(rt2mod, oraclemod):
    """Every picket ray is accepted by exactly the triangle its chunk claims
    (or by none), by a full scan with the oracle's rayTriangleIntersect."""
    pairs = 0
    for n in O.PICKETS:
        tris = O.pickets(n)
        ch = O.chunks(n)
        o, d = O._cat(*[ch[k][:2] for k in ch])
        claim = np.concatenate([ch[k][2] for k in ch])
        pairs += len(np.unique(np.concatenate([o, d], 1), axis=0)) * n
        sets = O.accepting_sets(oraclemod, tris, o, d)
        for i, (got, want) in enumerate(zip(sets, claim)):
            assert got == ([] if want < 0 else [int(want)]), f"pickets({n}) ray {i}: accepted by {got}, claim {want}"
        # and the oracle's scan agrees: the reference of the GPU tests
        occ = O.occluded_ref(oraclemod, tris, o, d)[0]
        assert np.array_equal(occ, claim >= 0)
    assert pairs <= O.MAX_SCAN_PAIRS, pairs


@pytest.mark.parametrize("n", O.PICKETS)
def test_chunk_compositions(rt2mod, oraclemod, n):
    ch = O.chunks(n)
    last, ng = n - 1, S.n_groups(n)
    for k in O.FULL:
        assert len(ch[k][0]) == len(ch[k][1]) == len(ch[k][2]) == 64
    assert ((ch["a"][2] >= 0) & (ch["a"][2] < 32)).all()
    b, c = ch["b"][2], ch["c"][2]
    assert (np.delete(b, 17) < 32).all() and (np.delete(b, 17) >= 0).all() and b[17] == last and last // 32 == ng - 1
    assert (np.delete(c, 17) < 32).all() and (np.delete(c, 17) >= 0).all() and c[17] == -1
    assert (ch["d"][2] == -1).all()
    g = O.e_group(n, np.arange(64))
    assert sorted(set(g.tolist())) == list(range(ng))  # every group of the sweep is some ray's only occluder
    assert np.array_equal(ch["e0"][2], 32 * g) and np.array_equal(ch["e1"][2], np.minimum(32 * g + 31, last))
    assert ((ch["e0"][2] // 32) == g).all() and ((ch["e1"][2] // 32) == g).all()
    assert n != 1217 or (g == 38).sum() >= 1  # the group read from L2 has a ray of its own
    fa, fb = ch["f33a"][2], ch["f33b"][2]
    assert len(fa) == len(fb) == 33
    assert fa[0] == last and (fa[1:] < 0).any() and fa[32] < 0 and (fa[1:] >= 0).any()
    assert fb[0] < 0 and (fb[1:] >= 0).any() and fb[32] >= 0 and (fb[1:] < 0).any()
    assert ch["f1a"][2].tolist() == [last] and ch["f1b"][2].tolist() == [-1]
    assert np.array_equal(O.pickets(1217)[:1216], O.pickets(1216))


@pytest.mark.parametrize("kind,n", [("soup", n) for n in T.SOUP_SIZES] + [("far", 33)])
def test_soups_hold_both_kinds(rt2mod, oraclemod, kind, n):
    nr = 1025 if (kind, n) == ("soup", 1217) else T.n_rays_for(n)
    o, d = T.scene_rays(kind, n, nr)
    occ, dst, _, _ = O.occluded_ref(oraclemod, T.scene_tris(kind, n), o, d)
    assert occ.mean() >= 0.25 and (~occ).any()
    # the C loop and the ctypes scan of trace_rays_lib are the same reference
    rd, rt, _ = T.scene_ref(oraclemod, kind, n, nr)
    assert np.array_equal(occ, rt >= 0) and np.array_equal(dst.view(np.uint32), rd.view(np.uint32))
    if (kind, n) == ("soup", 1217):
        for k in T.RAY_COUNTS:
            assert k == 1 or (occ[:k].any() and (~occ[:k]).any()), k
        assert occ[1024]  # the second workgroup's only ray
        assert occ[:257].any() and (~occ[:257]).any()


@pytest.mark.parametrize("order", T.FAN_ORDERS)
def test_fans_occlude_every_ray(rt2mod, oraclemod, order):
    """The fan's rays from around the camera are accepted by all 64 triangles."""
    o, d = O.fan_rays(order)
    assert len(o) == 97
    tris = T.scene_tris("fan_" + order, 64)
    sets = O.accepting_sets(oraclemod, tris, o, d)
    assert all(len(s) == 64 for s in sets), [len(s) for s in sets]
    assert O.occluded_ref(oraclemod, tris, o, d)[0].all()


def test_bounds_flip(rt2mod, oraclemod):
    o, d = (a[:193] for a in T.scene_rays("soup", 1217, 1025))
    tris = T.scene_tris("soup", 1217)
    hit, dst, _, _ = O.occluded_ref(oraclemod, tris, o, d)
    assert hit.sum() >= 48 and (~hit).sum() >= 8
    for name, tmax, want in O.bound_cases(dst, hit):
        got = O.occluded_ref(oraclemod, tris, o, d, tmax)[0]
        assert np.array_equal(got, want), name
    names = [c[0] for c in O.bound_cases(dst, hit)]
    assert len(names) == 8
