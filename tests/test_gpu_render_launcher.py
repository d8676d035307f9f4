"""The render launcher's paths that no other file asserts (DESIGN.md "The
render launcher"): the scalar choice for a scene outside the matrix filter's
range, forced variants the launcher must refuse, the host image set that
rt2_render_host and rt2_render_linear_host share, and the preview between two
path-traced renders on another stream.  Images are compared by bits.

Asserted elsewhere and not repeated here: the automatic matrix-kernel choice at
every boundary, frame split, cost order, chunked frames and slabs
(test_gpu_parity.py); every twin's id, name and sums (test_gpu_linear.py,
test_linear_cpu.py); which kernel runs when a forced variant cannot hold the
scenes of test_gpu_closest_hit.py; the launch order on the query side
(test_gpu_query_staging.py).
"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_parity import oracle_mean, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu

ORDINARY = ((-4, 9.5, -4), (4, 9.5, -4), (0, 9.5, 4))         # hit by the sky-bound rays of config B's view
ASSIST, SCALAR = 92, 0                                        # kSlab and kDefaultBrute of the launcher
ASSIST_BLOCK = 768

_refs = {}


def _name(rt2mod, v):
    return rt2mod.lib().rt2_variant_name(v).decode()


def _with_extra(tris, extra):
    out = np.concatenate([tris, np.zeros(len(extra), dtype=tris.dtype)])
    for k, (a, b, c) in enumerate(extra):
        t = out[len(tris) + k]
        t["a"][:3], t["b"][:3], t["c"][:3] = a, b, c
        t["materialIndex"] = 0
    return out


def _bits_equal(got, want, what):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, what
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ"


def _reference(oraclemod, key, sd, u, rows, fc, mode="brute", tris=None):
    """The oracle's mean over frames 0 .. fc of the listed rows; once per key, read-only."""
    if key not in _refs:
        ref, _, _ = oracle_mean(oraclemod, sd, u, np.asarray(rows), 0, fc, mode, tris=tris)
        ref.setflags(write=False)
        _refs[key] = ref
    return _refs[key]


# ---- a scene outside the matrix filter's range: the scalar choice ------------------------------------------------------

def _out_of_range(rt2mod):
    """The scene without triangles (the sky alone): the one scene the launcher keeps off the matrix kernels.  A
    triangle outside the filter's validated range (a coordinate of 3e6, say) does not take its scene there: it gets
    an always-pass record (test_gpu_mfma.py, test_gpu_valu_diet.py) and the automatic choice stays the matrix
    kernel."""
    sd = rt2mod.SceneData()
    sd.add_material(rt2mod.Material.diffuse((0.7, 0.7, 0.7)))
    return sd, sd.triangles()


def _lanes_of_assist(rt2mod, torch):
    """The resident lanes the launcher counts for its scalar choice: CUs x the occupancy API's workgroups of the
    assist kernel x its block."""
    L = rt2mod.lib()
    L.rt2_variant_occupancy.restype = C.c_int
    L.rt2_variant_occupancy.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    occ = C.c_int(0)
    assert L.rt2_variant_occupancy(ASSIST, C.byref(occ), None, None) == 0
    return torch.cuda.get_device_properties(0).multi_processor_count * max(occ.value, 1) * ASSIST_BLOCK


def test_out_of_range_scene_few_items_per_lane(rt2mod, oraclemod, config_scene, torch_cuda):
    """1 ray per pixel, 1 bounce, 64 x 36: fewer than 4 items per resident lane, so the assist kernel runs, and its
    linear twin for the linear render; the whole image equals the oracle."""
    sd, tris = _out_of_range(rt2mod)
    W, H = 64, 36
    assert W * H < 4 * _lanes_of_assist(rt2mod, torch_cuda)
    u = rt2mod.offline_uniforms(W, H, 1, 1, len(tris))
    scene = rt2mod.Scene(triangles=tris, materials=sd.materials())
    img = scene.render_host(u, 0, 1)
    assert scene.last_kernel() == ASSIST and _name(rt2mod, ASSIST) == "assist12/max3f8/w6"
    ref = _reference(oraclemod, ("empty", W, H), sd, u, np.arange(H), 1, tris=tris)
    assert (ref != ref[0, 0]).any()  # not a constant image
    _bits_equal(img[..., :3], ref, "out of range, 64x36")
    scene.render_linear_host(u, 0, 1)
    twin = scene.last_kernel()
    assert twin == rt2mod.LINEAR_TWIN + ASSIST and _name(rt2mod, twin) == _name(rt2mod, ASSIST) + "/lin"


def test_out_of_range_scene_many_items_per_lane(rt2mod, oraclemod, config_scene, torch_cuda):
    """The smallest 1,024-pixel-wide image with at least 4 items per resident lane: the 6-wave scalar-path kernel
    runs (the automatic id 0), and 136's twin for the linear render; 8 rows, the first and the last among them,
    equal the oracle."""
    sd, tris = _out_of_range(rt2mod)
    W = 1024
    H = -(-4 * _lanes_of_assist(rt2mod, torch_cuda) // W)
    u = rt2mod.offline_uniforms(W, H, 1, 1, len(tris))
    scene = rt2mod.Scene(triangles=tris, materials=sd.materials())
    img = scene.render_host(u, 0, 1)
    assert scene.last_kernel() == SCALAR and _name(rt2mod, 136) == "smem/256/max3f8/coop32/w6/lockstep"
    rows = np.array([0, 1, 2, H // 3, H // 2, H - 3, H - 2, H - 1])
    ref = _reference(oraclemod, ("empty", W, H), sd, u, rows, 1, tris=tris)
    assert (ref != ref[0, 0]).any()
    _bits_equal(img[rows][..., :3], ref, f"out of range, {W}x{H}")
    scene.render_linear_host(u, 0, 1)
    twin = scene.last_kernel()
    assert twin == rt2mod.LINEAR_TWIN + 136 and _name(rt2mod, twin) == _name(rt2mod, 136) + "/lin"


# ---- forced variants the launcher must refuse ----------------------------------------------------------------------------

REFUSED_W, REFUSED_H, REFUSED_RAYS, REFUSED_FRAMES = 40, 24, 2, 2


def _refused(rt2mod, oraclemod, key, sd, bounces, tris, forced, traversal, ran):
    u = rt2mod.offline_uniforms(REFUSED_W, REFUSED_H, bounces, REFUSED_RAYS, len(tris))
    scene = rt2mod.Scene(triangles=tris, materials=sd.materials(), nodes=sd.nodes() if traversal == "bvh" else None)
    scene.set_traversal(traversal)
    assert scene.set_variant(forced) == forced
    img = scene.render_host(u, 0, REFUSED_FRAMES)
    assert scene.last_kernel() == ran
    ref = _reference(oraclemod, key, sd, u, np.arange(REFUSED_H), REFUSED_FRAMES, traversal, tris=tris)
    assert (ref != ref[0, 0]).any()  # not a constant image
    _bits_equal(img[..., :3], ref, f"forced {forced}, {traversal}")


def test_resident_variant_on_39_groups_runs_the_l2_form(rt2mod, oraclemod, config_scene, torch_cuda):
    """353 holds 38 groups: on 39 the launcher takes the automatic choice, the L2 form (a 40 x 24 image is a slab of
    fewer than 6 items per lane: its fair-share kernel)."""
    sd, spec = config_scene("B")
    tris = sd.triangles()
    assert len(tris) <= 38 * 32
    tris = _with_extra(tris, [ORDINARY] * (38 * 32 + 1 - len(tris)))
    assert (len(tris) + 31) // 32 == 39
    assert _name(rt2mod, 356).startswith("mfmarl2/")
    _refused(rt2mod, oraclemod, "B39", sd, spec.bounces, tris, 353, "brute", 356)


def test_bvh_variant_under_brute_traversal_runs_the_matrix_kernel(rt2mod, oraclemod, config_scene, torch_cuda):
    """109 walks the BVH: under brute traversal the launcher takes the automatic matrix kernel (config B's 38 groups
    resident; the 40 x 24 slab: the fair-share kernel)."""
    sd, spec = config_scene("B")
    assert _name(rt2mod, 354).startswith("mfmar/")
    _refused(rt2mod, oraclemod, "B", sd, spec.bounces, sd.triangles(), 109, "brute", 354)


def test_matrix_variant_under_bvh_traversal_runs_the_bvh_kernel(rt2mod, oraclemod, config_scene, torch_cuda):
    sd, spec = config_scene("B")
    assert _name(rt2mod, 109) == "bvh4/256/t16/w5"
    _refused(rt2mod, oraclemod, "Bbvh", sd, spec.bounces, sd.triangles(), 353, "bvh", 109)


def test_matrix_variant_on_out_of_range_scene_runs_the_scalar_choice(rt2mod, oraclemod, config_scene, torch_cuda):
    """353 filters on the matrix cores: a scene outside the filter's range takes the scalar choice (40 x 24: the
    assist kernel)."""
    sd, tris = _out_of_range(rt2mod)
    assert REFUSED_W * REFUSED_H * REFUSED_FRAMES < 4 * _lanes_of_assist(rt2mod, torch_cuda)
    _refused(rt2mod, oraclemod, "empty", sd, 4, tris, 353, "brute", ASSIST)


# ---- the shared host image set -----------------------------------------------------------------------------------------

def test_host_image_set_shared_by_both_blocking_renders(rt2mod, config_scene, torch_cuda):
    """render_host (8-bit output too) and render_linear_host alternate on one Scene: grow, reuse at a smaller size,
    grow again for the other user, reuse.  Every result equals the same call on a fresh Scene."""
    sd, spec = config_scene("A")

    def uniforms(w, h):
        return rt2mod.offline_uniforms(w, h, spec.bounces, 2, sd.num_triangles)

    calls = [("render_host", 32, 20, dict(rgb8=True)), ("render_linear_host", 64, 36, dict(moments=True)),
             ("render_host", 48, 28, dict(rgb8=True)), ("render_linear_host", 32, 20, dict(moments=False))]
    shared = rt2mod.Scene(sd)
    for fn, w, h, kw in calls:
        got = getattr(shared, fn)(uniforms(w, h), 0, 2, **kw)
        want = getattr(rt2mod.Scene(sd), fn)(uniforms(w, h), 0, 2, **kw)
        got, want = (got, want) if isinstance(got, tuple) else ((got,), (want,))
        assert len(got) == len(want)
        for k, (g, fresh) in enumerate(zip(got, want)):
            assert g.dtype == fresh.dtype and g.shape == fresh.shape
            assert (g[..., :3] != 0).any(), f"{fn} {w}x{h}: output {k} is empty"
            assert np.array_equal(g.view(np.uint8), fresh.view(np.uint8)), f"{fn} {w}x{h}: output {k} differs"


# ---- the preview through the shared launch bookkeeping -----------------------------------------------------------------

def test_preview_between_renders_on_another_stream(rt2mod, config_scene, torch_cuda):
    """A basicShading render on a second stream between two path-traced renders on a first: it waits for the render
    before it and the render after it waits for it (they share the scene's counters), so both path-traced images
    equal those of a scene that never ran the preview; the scene reports -1 after the preview and the path-traced
    kernel's id after the last render."""
    torch = torch_cuda
    sd, spec = config_scene("B")
    W, H = 48, 28
    n = W * H
    u = rt2mod.offline_uniforms(W, H, spec.bounces, 2, sd.num_triangles)
    up = rt2mod.Uniforms.from_buffer_copy(u)
    up.basicShading = 1
    sh = rt2mod.shard()

    def run(preview):
        scene = rt2mod.Scene(sd)
        a, b = torch.cuda.Stream(), torch.cuda.Stream()
        acc = torch.zeros((3, n, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        kernels = []
        scene.render(u, 0, 2, sh, acc[0].data_ptr(), 0, a.cuda_stream)
        kernels.append(scene.last_kernel())
        if preview:
            scene.render(up, 0, 1, sh, acc[2].data_ptr(), 0, b.cuda_stream)
            kernels.append(scene.last_kernel())
        scene.render(u, 2, 2, sh, acc[1].data_ptr(), 0, a.cuda_stream)
        kernels.append(scene.last_kernel())
        a.synchronize()
        b.synchronize()
        return acc.cpu().numpy(), kernels

    got, k_got = run(True)
    want, k_want = run(False)
    assert k_want[0] > 0 and k_want[0] == k_want[1]
    assert k_got == [k_want[0], -1, k_want[1]]
    assert (got[2][:, :3] != 0).any(), "the preview drew nothing"
    for i in (0, 1):
        assert (want[i][:, :3] != 0).any()
        _bits_equal(got[i], want[i], f"path-traced render {i} with the preview between")
