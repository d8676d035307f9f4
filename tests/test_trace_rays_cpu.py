"""Ray queries without a GPU: the C-ABI's argument checks and struct layouts,
and the premises of tests/test_gpu_trace_rays.py on the CPU oracle alone (its
rays hit and miss, the soups have no exact distance ties on them, the tie
scene has), so none of those tests can pass vacuously."""
import ctypes as C

import numpy as np
import pytest

import closest_hit_scenes as S
import trace_rays_lib as T


def test_struct_layouts(rt2mod):
    r, h = rt2mod.RAY_DTYPE, rt2mod.HIT_DTYPE
    assert r.itemsize == 32 and h.itemsize == 8
    assert r.fields["o"][1] == 0 and r.fields["tmax"][1] == 12 and r.fields["d"][1] == 16 and r.fields["pad"][1] == 28
    assert h.fields["dst"][1] == 0 and h.fields["tri"][1] == 4
    assert rt2mod.TRACE_AUTO == 0 and rt2mod.TRACE_SCALAR == 1
    assert rt2mod.lib().rt2_abi_version() == 4  # the entry points only add to the interface


def test_argument_validation(rt2mod):
    """Bad arguments return < 0 with "bad argument" before any device call
    (and before the scene is read: `fake` is no scene)."""
    L = rt2mod.lib()
    rays = np.zeros(4, rt2mod.RAY_DTYPE)
    hits = np.zeros(4, rt2mod.HIT_DTYPE)
    pr, ph = rays.ctypes.data, hits.ctypes.data
    assert pr % 16 == 0 and ph % 8 == 0
    buf = C.create_string_buffer(4096)
    fake = C.c_void_p(C.addressof(buf))
    bad_dev = [(None, pr, 4, ph, 0), (fake, pr, -1, ph, 0), (fake, None, 4, ph, 0), (fake, pr, 4, None, 0),
               (fake, pr, 4, ph, 2), (fake, pr, 4, ph, -1), (fake, pr + 4, 4, ph, 0), (fake, pr, 4, ph + 4, 0)]
    for s, r, n, h, fl in bad_dev:
        L.rt2_scene_create(None, 0, None, 0, None, 0, 0, None)  # leaves another message behind
        assert L.rt2_trace_rays(s, r, n, h, fl, None) < 0, (r, n, h, fl)
        assert b"rt2_trace_rays: bad argument" in L.rt2_last_error()
    for s, r, n, h, fl in bad_dev[:6]:
        L.rt2_scene_create(None, 0, None, 0, None, 0, 0, None)
        assert L.rt2_trace_rays_host(s, r, n, h, fl) < 0, (r, n, h, fl)
        assert b"rt2_trace_rays_host: bad argument" in L.rt2_last_error()
    assert L.rt2_trace_rays(None, None, 0, None, 0, None) < 0  # a null scene, whatever n
    # n = 0: nothing to do, nothing launched (no device here to launch on)
    assert L.rt2_trace_rays(fake, None, 0, None, 0, None) == 0
    assert L.rt2_trace_rays(fake, pr, 0, ph, rt2mod.TRACE_SCALAR, None) == 0
    assert L.rt2_trace_rays_host(fake, None, 0, None, 0) == 0


@pytest.mark.parametrize("kind,n", [("soup", n) for n in T.SOUP_SIZES] + [("fan_" + o, 64) for o in T.FAN_ORDERS] +
                         [("far", 33)])
def test_rays_hit_and_miss(rt2mod, oraclemod, kind, n):
    nr = 1025 if (kind, n) == ("soup", 1217) else T.n_rays_for(n)
    dst, tri, ties = T.scene_ref(oraclemod, kind, n, nr)
    hit = tri >= 0
    assert hit.mean() >= 0.25, f"{int(hit.sum())} of {nr} rays hit"
    assert (~hit).any()
    assert np.array_equal(dst[~hit], np.full(int((~hit).sum()), T.UNBOUNDED))
    if kind == "soup":
        # what lets BVH results be compared with the array-order scan
        assert ties[hit].max() == 1, f"{int((ties > 1).sum())} rays with an exact distance tie"
        if n >= 1216:
            assert len(np.unique(tri[hit] // 32)) >= 20  # winners all over the scan
    if kind == "fan_far_first":
        assert (tri[hit] >= 32).mean() >= 0.75  # the bound improves through the first group into the second
    if kind == "fan_near_first":
        assert (tri[hit] < 32).mean() >= 0.75


def test_soup_1217_prefixes(rt2mod, oraclemod):
    """The ray-count cases are prefixes of the 1,025 rays: the 193-ray prefix
    has hits beyond the resident groups (index 1,216 is group 38)."""
    dst, tri, _ = T.scene_ref(oraclemod, "soup", 1217, 1025)
    assert (tri[:193] >= 0).mean() >= 0.25 and (tri[:193] < 0).any()
    assert (tri[:64] >= 0).any() and (tri[:64] < 0).any()
    assert (tri[1024:] >= 0).all()  # the second workgroup's only ray is a hit
    assert ((dst[tri >= 0] > 0) & (dst[tri >= 0] < 30)).all()


def test_tie_scene_has_ties(rt2mod, oraclemod):
    n = 1217
    fams = S.tie_families(n)
    dst, tri, ties = T.scene_ref(oraclemod, "ties", n, 193)
    for fam in fams:
        low = min(fam)
        own = tri == low
        assert own.sum() >= 4, f"family {fam}: {int(own.sum())} rays"
        assert (ties[own] == len(fam)).all()
        assert not np.isin(tri, [i for i in fam if i != low]).any()
    assert any(1216 in fam for fam in fams)  # the family across the resident / L2 edge
