"""The BVH walks on hand-built trees that read out each of their decisions.

Renders (render_bvh4, the product kernel, and the experiment build's earlier
walks), the traceBasic preview and ray queries on the scenes of
tests/bvh_edge_scenes.py: skipped axes (|d_i| < 1e-6 decided by the pixel
jitter, lane by lane), boxes flat on an axis, boxes with a face, an edge or a
corner at the camera, chains as deep as the host accepts (depth 62: the stack's
last slots, 64 KiB of LDS for the per-lane stacks of the preview and the
query), leaves of 0, 1, 30, 31, 32, 33 and -1 triangles, and waves that mix
lanes inside and outside the fast slab's range.

The reference is the CPU oracle's BVH mode on the same node array: images and
dst as uint32 views (no tolerance), indices and counters exactly.  The
leaf-test count is compared everywhere: it sees a box that is wrongly visited
or wrongly pruned also where the image stays the same.  The array scan is no
reference here (the boxes need not bound their triangles).
tests/test_bvh_edge_scenes.py asserts on the oracle alone what the scenes are
built to give, and that each of five changed walks is seen by them.

Every test asserts which kernel ran (rt2_scene_diag).
"""
import ctypes as C

import numpy as np
import pytest

import bvh_edge_scenes as E
import closest_hit_scenes as S
import trace_rays_lib as T
from conftest import require_variant

pytestmark = pytest.mark.gpu

# render_bvh4 (the product's BVH kernel); in the experiment build: render_bvh3
# with its default spec (53), unconstrained registers (46), the binary64 slab
# (50), the filtered slab (55: its own flat-box and near-tie logic),
# render_bvh2 (40) and the node-array walk render_bvh (37)
BVH4 = 109
VARIANTS = (BVH4, 53, 46, 50, 55, 40, 37)
PREVIEW = -1  # rt2_scene_diag after a traceBasic launch

CASES = {c[0]: c for c in E.render_cases()}
_refs = {}


def _bits(img):
    return np.ascontiguousarray(img[..., :3], dtype=np.float32).view(np.uint32)


def _ref(oraclemod, name, sc, u, fb, fc):
    """(mean image, segments, leaf tests) of the oracle's BVH mode, once per case and left unchanged."""
    if name not in _refs:
        acc, _, segs, tests = oraclemod.render(sc.tris, sc.mats, u, np.arange(u.height, dtype=np.int32), fb, fc,
                                               "bvh", nodes=sc.nodes)
        img = acc[..., :3] / np.float32(fc)
        img.setflags(write=False)
        _refs[name] = (img, segs, tests)
    return _refs[name]


def _render(rt2mod, sc, u, fb, fc, variant):
    """The image, the stats and the id of the kernel that ran."""
    scene = rt2mod.Scene(triangles=sc.tris, materials=sc.mats, nodes=sc.nodes)
    try:
        scene.set_traversal("bvh")
        if variant > 0:
            scene.set_variant(variant)
        img = scene.render_host(u, fb, fc)
        st = scene.stats(reset=True)
        return img, st, scene.last_kernel()
    finally:
        scene.close()


def _winner(px, coded):
    if not coded:
        return str(px[:3])
    try:
        i = int(S.decode(px[None])[0])
    except ValueError:
        return f"no index code {px[:3]}"
    return "a miss" if i < 0 else f"triangle {i}"


def _same_image(gpu, ref, what, coded=True):
    bad = (_bits(gpu) != _bits(ref)).any(-1)
    if bad.any():
        lines = [f"pixel x={x} y={y}: GPU {_winner(gpu[y, x], coded)}, oracle {_winner(ref[y, x], coded)}"
                 for y, x in np.argwhere(bad)[:6]]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} pixels differ in their bits\n" +
                             "\n".join(lines))


# ---- renders -------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", list(CASES))
def test_render(rt2mod, oraclemod, name, variant):
    require_variant(rt2mod, variant)
    _, sc, u, fb, fc = CASES[name]
    ref, segs, tests = _ref(oraclemod, name, sc, u, fb, fc)
    img, st, ran = _render(rt2mod, sc, u, fb, fc, variant)
    assert ran == variant, f"kernel {ran} ran, not {variant}"
    coded = not name.startswith("slab_switch")
    print(f"{name} v{variant}: segments {st.segments} / {segs}, leaf tests {st.tests} / {tests}")
    _same_image(img, ref, f"{name}, variant {variant}", coded)
    assert st.segments == segs
    assert st.tests == tests, f"{name}, variant {variant}: {st.tests} leaf tests, the oracle makes {tests}"


# ---- the traceBasic preview --------------------------------------------------------------------

PREVIEWS = [("chain62-interior", "chain", (E.MAX_DEPTH, "interior", 0), "none", (64, 64)),
            ("chain62-leaf", "chain", (E.MAX_DEPTH, "leaf", 1), "none", (64, 64)),
            ("displaced-x-none", "displaced", ("x",), "none", (64, 16)),   # only the centre column skips x
            ("displaced-x-zero", "displaced", ("x",), "zero", (64, 16))]  # every lane does


@pytest.mark.parametrize("name,kind,args,skip,size", PREVIEWS, ids=[p[0] for p in PREVIEWS])
def test_preview(rt2mod, oraclemod, name, kind, args, skip, size):
    """render_basic<256, true>: closest_bvh with depth + 2 stack slots per lane
    (64 KiB of LDS at depth 62)."""
    sc = E.get(kind, *args)
    u = E.uniforms(size[0], size[1], len(sc.tris), skip, "x", sc.shift, basic=True)
    acc, _, segs, tests = oraclemod.render(sc.tris, sc.mats, u, np.arange(u.height, dtype=np.int32), 0, 1, "bvh",
                                           nodes=sc.nodes)
    img, st, ran = _render(rt2mod, sc, u, 0, 1, 0)
    assert ran == PREVIEW
    print(f"preview {name}: segments {st.segments} / {segs}, leaf tests {st.tests} / {tests}")
    _same_image(img, acc, f"preview {name}", coded=False)
    assert st.segments == segs == u.width * u.height and st.tests == tests
    # the preview shows a light's emission colour itself (a miss shows the sky): all three channels are levels
    win = np.isin(_bits(acc), S.LEV.view(np.uint32)).all(-1)
    if kind == "chain":
        assert 1000 < win.sum() < 3000
    elif skip == "none":
        assert win.all() and tests == segs + u.height  # the centre column's lanes test both leaves
    else:
        assert win.all() and tests == 2 * segs


# ---- ray queries -------------------------------------------------------------------------------------

_query_scenes = {}


def _query_scene(rt2mod, sc):
    if sc.name not in _query_scenes:
        scene = rt2mod.Scene(triangles=sc.tris, materials=sc.mats, nodes=sc.nodes)
        scene.set_traversal("bvh")
        _query_scenes[sc.name] = scene
    return _query_scenes[sc.name]


def _same_hits(got, ref, what):
    gd, gt = got
    dst, tri = ref[0], ref[1]
    assert gd.dtype == np.float32 and gt.dtype == np.int32 and len(gd) == len(dst) == len(gt)
    bad = (gd.view(np.uint32) != dst.view(np.uint32)) | (gt != tri)
    if bad.any():
        lines = [f"ray {i}: GPU ({gd[i]!r}, {gt[i]}), oracle ({dst[i]!r}, {tri[i]})" for i in np.flatnonzero(bad)[:6]]
        raise AssertionError(f"{what}: {int(bad.sum())} of {len(bad)} rays differ\n" + "\n".join(lines))


def _query(rt2mod, scene, o, d, tmax, ref, what):
    scene.stats(reset=True)
    got = scene.trace_rays(o, d, tmax)
    assert scene.last_kernel() == rt2mod.QUERY_BVH
    st = scene.stats(reset=True)
    print(f"{what}: leaf tests {st.tests} / {int(ref[2].sum())}, node visits {st.node_visits} / {int(ref[3].sum())}")
    _same_hits(got, ref, what)
    assert st.segments == len(o)
    assert st.tests == int(ref[2].sum()) and st.node_visits == int(ref[3].sum()), what


@pytest.mark.parametrize("n", E.RAY_COUNTS)
@pytest.mark.parametrize("sc", E.query_scenes(), ids=[s.name for s in E.query_scenes()])
def test_queries(rt2mod, oraclemod, sc, n):
    """trace_rays_scalar<256, true> against oracle.closest_hits' BVH walk: 193
    rays (one ragged block) and 257 (a second block of one ray), without bounds
    and with bvh_edge_scenes.bounded_tmax's."""
    o, d, _ = E.query_rays(sc, n)
    scene = _query_scene(rt2mod, sc)
    ref = oraclemod.closest_hits(sc.tris, o, d, None, "bvh", sc.nodes)
    _query(rt2mod, scene, o, d, None, ref, f"{sc.name}, {n} rays")
    tmax = E.bounded_tmax(sc, o, d, ref[0], ref[1])
    bounded = oraclemod.closest_hits(sc.tris, o, d, T.bound_of(tmax), "bvh", sc.nodes)
    assert (bounded[1] != ref[1]).sum() >= 8  # the bounds do cut hits off
    _query(rt2mod, scene, o, d, tmax, bounded, f"{sc.name}, {n} rays, bounded")


# ---- the depth limit ---------------------------------------------------------------------------------------

def test_depth_limit(rt2mod, oraclemod):
    """A chain of 63 levels is refused; 62 is accepted (its renders, previews and
    queries are the tests above: here one more of each on the other chain)."""
    sc = E.chain(E.MAX_DEPTH + 1)
    with pytest.raises(rt2mod.RT2Error, match="deeper than"):
        rt2mod.Scene(triangles=sc.tris, materials=sc.mats, nodes=sc.nodes)
    sc = E.get("chain", E.MAX_DEPTH, "interior", 1)
    scene = rt2mod.Scene(triangles=sc.tris, materials=sc.mats, nodes=sc.nodes)
    try:
        scene.set_traversal("bvh")
        rows = np.arange(64, dtype=np.int32)
        for basic, kernel in ((False, BVH4), (True, PREVIEW)):
            u = E.uniforms(64, 64, len(sc.tris), basic=basic)
            acc, _, segs, tests = oraclemod.render(sc.tris, sc.mats, u, rows, 0, 1, "bvh", nodes=sc.nodes)
            img = scene.render_host(u, 0, 1)
            st = scene.stats(reset=True)
            assert scene.last_kernel() == kernel
            _same_image(img, acc, f"chain 62, basicShading {basic}", coded=not basic)
            assert (st.segments, st.tests) == (segs, tests) == (4096, 62 * 4096)
        o, d, _ = E.query_rays(sc, 193)
        ref = oraclemod.closest_hits(sc.tris, o, d, None, "bvh", sc.nodes)
        _query(rt2mod, scene, o, d, None, ref, "chain 62, second slot")
    finally:
        scene.close()
