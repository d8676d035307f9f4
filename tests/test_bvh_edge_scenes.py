"""The premises of tests/test_gpu_bvh_edges.py, on the CPU oracle alone: the
hand-built trees of tests/bvh_edge_scenes.py give what the GPU tests rely on
(every chain leaf wins somewhere and is tested in every segment, the
reference's stack fills to the chain's depth, the jitter decides the skipped
axis pixel by pixel in every row and block, every class of query rays hits and
misses, the BVH walk differs from the array scan where boxes do not bound
their triangles), so none of those tests can pass vacuously.

The scenes are shown to be sensitive the way tests/test_filter_exactness.py
shows it of its harness: a copy of oracle/rt_oracle.c with one decision of the
walk changed is compiled beside the oracle, and must give another image, another
per-ray result or another leaf-test count on the scene built for that decision.
"""
import os
import subprocess

import numpy as np
import pytest

import bvh_edge_scenes as E
import closest_hit_scenes as S
import trace_rays_lib as T

F32 = np.float32
ORACLE_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle")
ORACLE_SRC = os.path.join(ORACLE_DIR, "rt_oracle.c")

_images = {}


def _cases():
    return {c[0]: c for c in E.render_cases()}


def _image(oraclemod, name, mode="bvh", library=None):
    """(decoded winners or None for the mixed soups, image, segments, tests) of a render case."""
    key = (name, mode, library is None)
    if library is not None or key not in _images:
        _, sc, u, fb, fc = _cases()[name]
        rows = np.arange(u.height, dtype=np.int32)
        acc, _, segs, tests = oraclemod.render(sc.tris, sc.mats, u, rows, fb, fc, mode, nodes=sc.nodes,
                                               library=library)
        idx = None if name.startswith("slab_switch") else S.decode(acc)
        if library is not None:
            return idx, acc, segs, tests
        _images[key] = (idx, acc, segs, tests)
    return _images[key]


CHAINS = [(d, near, slot) for d in E.CHAIN_DEPTHS for near in ("interior", "leaf") for slot in (0, 1)]


@pytest.mark.parametrize("depth,near,slot", CHAINS)
def test_chain_every_leaf_wins_and_is_tested(rt2mod, oraclemod, depth, near, slot):
    sc = E.get("chain", depth, near, slot)
    assert len(sc.nodes) == 2 * depth - 1 and len(sc.tris) == depth
    idx, _, segs, tests = _image(oraclemod, sc.name)
    cnt = np.bincount(idx[idx >= 0], minlength=depth)
    assert cnt.min() >= 8, f"triangle {int(cnt.argmin())} wins {int(cnt.min())} pixels"
    assert segs == 64 * 64 and tests == depth * segs
    # each winner inside its own 8 x 8 tile: a lost leaf is a lost tile
    ys, xs = np.nonzero(idx >= 0)
    assert np.array_equal(idx[ys, xs], (ys // 8) * 8 + xs // 8)


@pytest.mark.parametrize("depth,near", [(d, n) for d in E.CHAIN_DEPTHS for n in ("interior", "leaf")])
def test_chain_stack_fill(rt2mod, oraclemod, depth, near):
    """The walk restated in Python: with the interior child near, the stack
    holds `depth` entries (every leaf of the chain) before the first leaf is
    tested; with the leaf near, never more than 3."""
    sc = E.get("chain", depth, near, 0)
    o, d, cls = E.query_rays(sc, 193)
    pick = np.flatnonzero(cls == E.ORDINARY)
    dst, tri, tests, visits = oraclemod.closest_hits(sc.tris, o[pick], d[pick], None, "bvh", sc.nodes)
    assert (tri >= 0).sum() >= 4
    for k, i in enumerate(pick):
        if tri[k] < 0 or k >= 12:
            continue
        w = E.walk(oraclemod, sc.tris, sc.nodes, o[i], d[i])
        assert (w[0].view(np.uint32), w[1], w[2], w[3]) == (dst[k].view(np.uint32), tri[k], tests[k], visits[k])
        assert w[2] == depth and w[3] == depth - 1
        assert w[4] == depth if near == "interior" else w[4] <= 3


def test_depth_63_chain_is_one_level_too_deep(rt2mod):
    sc = E.chain(E.MAX_DEPTH + 1)
    assert len(sc.nodes) == 2 * 63 - 1 and len(sc.tris) == 63 <= 64


def _blocks(mask):
    h, w = mask.shape
    return mask.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 64)


JITTER = [f"displaced-{a}-jitter" for a in ("x", "y", "z", "xy")] + [f"flat-{a}-jitter" for a in "xyz"]


@pytest.mark.parametrize("name", JITTER)
def test_jitter_decides_the_skip_in_every_row_and_block(rt2mod, oraclemod, name):
    """Triangle 0 wins exactly where the lane skips the axis; both outcomes
    occur in every image row and every 8 x 8 block, whatever lanes share a wave."""
    idx, _, segs, _ = _image(oraclemod, name)
    assert segs == idx.size and (idx >= 0).all()
    skipped = idx == 0
    for what, m in (("skipped", skipped), ("not skipped", ~skipped)):
        assert m.any(1).all(), f"a row without a {what} lane"
        assert _blocks(m).any(1).all(), f"an 8 x 8 block without a {what} lane"
    if name.startswith("flat"):
        assert set(np.unique(idx)) == {0, 2, 3}  # triangle 1's box is flat on the view axis: never entered


@pytest.mark.parametrize("axes", ("x", "y", "z", "xy"))
def test_displaced_all_or_no_lane_skips(rt2mod, oraclemod, axes):
    idx, _, _, tests = _image(oraclemod, f"displaced-{axes}-zero")
    assert (idx == 0).all() and tests == 2 * idx.size  # d_axis = +-0 everywhere: both leaves
    idx, _, _, tests = _image(oraclemod, f"displaced-{axes}-none")
    assert (idx == 1).all() and tests == idx.size


def test_touching_winners(rt2mod, oraclemod):
    """Which of the boxes at the camera are admitted (bvh_edge_scenes.touching)."""
    idx, _, _, _ = _image(oraclemod, "touching")
    cnt = np.bincount(idx[idx >= 0], minlength=8)
    assert cnt[0] > 30 and cnt[1] > 30  # tMin = -0; tMax = -0 is not < 0
    assert cnt[4] == 0                  # behind the camera
    assert cnt[6] == 0 and cnt[7] > 30  # dA < dB false: the second twin is near and keeps the ties
    xs = np.nonzero(idx == 2)[1]
    assert len(xs) > 30 and xs.min() >= 32  # the edge box: d.x > 0 only (column 32 is x = 0 before the jitter)
    ys, xs = np.nonzero(idx == 3)
    assert len(xs) > 10 and xs.min() >= 32 and ys.min() >= 32  # the corner box: d.x > 0 and d.y > 0
    brute, _, _, _ = _image(oraclemod, "touching", "brute")
    assert (brute == 4).sum() > 30 and (brute == 6).sum() > 30


def test_leaf_sizes_every_triangle_wins(rt2mod, oraclemod):
    sc = E.get("leaf_sizes")
    counts = sc.nodes["triangleCount"][sc.nodes["childIndex"] == -1]
    assert sorted(counts.tolist()) == sorted(E.LEAF_COUNTS) and {30, 31, -1} <= set(counts.tolist())
    idx, _, segs, tests = _image(oraclemod, sc.name)
    cnt = np.bincount(idx[idx >= 0], minlength=127)
    assert len(cnt) == 127 and cnt.min() >= 3
    assert tests == 127 * segs


def test_root_leaf(rt2mod, oraclemod):
    sc = E.get("root_leaf")
    assert len(sc.nodes) == 1 and sc.nodes["childIndex"][0] == -1
    idx, _, segs, tests = _image(oraclemod, sc.name)
    assert np.bincount(idx[idx >= 0], minlength=3).min() >= 8 and tests == 3 * segs


@pytest.mark.parametrize("which", "abc")
def test_slab_switch_has_scattered_rays(rt2mod, oraclemod, which):
    """More than two segments per sample: beside the primary rays (camera x =
    2^-40: outside the fast slab's range) a wave holds rays from surface points."""
    name = f"slab_switch-{which}"
    _, sc, u, fb, fc = _cases()[name]
    _, _, segs, _ = _image(oraclemod, name)
    assert segs / (u.width * u.height * fc) >= 2.0
    ok = lambda c: c == 0 or 2.0 ** -37 <= abs(c) <= 2.0 ** 59  # rt2_bvh.h mk_coord_ok
    boxes = np.concatenate([sc.nodes["bmin"].ravel(), sc.nodes["bmax"].ravel()])
    assert ok(u.cameraPos.x) == (which == "b") and all(ok(c) for c in boxes) == (which != "b")


@pytest.mark.parametrize("name", ["displaced-x-jitter", "displaced-xy-jitter", "displaced-z-none", "flat-x-jitter",
                                  "flat-y-none", "touching"])
def test_bvh_walk_differs_from_the_array_scan(rt2mod, oraclemod, name):
    """Why the array scan cannot be the reference here: boxes that do not bound
    their triangles hide hits the scan finds."""
    bvh, _, _, _ = _image(oraclemod, name)
    brute, _, _, _ = _image(oraclemod, name, "brute")
    assert (bvh != brute).mean() > 0.1


# ---- query rays ------------------------------------------------------------------------

QUERIES = [(sc.name, n) for sc in E.query_scenes() for n in E.RAY_COUNTS]
_by_name = {sc.name: sc for sc in E.query_scenes()}


@pytest.mark.parametrize("name,n", QUERIES)
def test_query_ray_classes_hit_and_miss(rt2mod, oraclemod, name, n):
    sc = _by_name[name]
    o, d, cls = E.query_rays(sc, n)
    assert o.dtype == F32 and d.dtype == F32 and len(o) == n
    dst, tri, tests, visits = oraclemod.closest_hits(sc.tris, o, d, None, "bvh", sc.nodes)
    for c, cname in enumerate(E.CLASS_NAMES):
        m = cls == c
        assert (tri[m] >= 0).any() and (tri[m] < 0).any(), f"{cname}: {int((tri[m] >= 0).sum())} hits of {int(m.sum())}"
    assert np.isnan(o[E.NAN_RAY]).any() and np.isinf(d[E.INF_RAY]).any()
    assert tri[E.NAN_RAY] == -1 and tri[E.INF_RAY] == -1
    # the threshold values themselves arrive bit for bit, on every axis
    comp = np.abs(d[cls == E.THRESHOLD])
    for v in (0.0, E.SKIP, np.nextafter(E.SKIP, F32(1)), np.nextafter(E.SKIP, F32(0)), F32(9.99e-7)):
        assert ((comp == F32(v)).sum(0) > 0).all()
    assert np.signbit(d[cls == E.THRESHOLD][d[cls == E.THRESHOLD] == 0]).any()
    tiny = d[cls == E.TINY]
    assert (np.abs(tiny) < E.SKIP).all() and (tiny == 0).all(1).any()
    ln = np.linalg.norm(d[cls == E.LONG].astype(np.float64), axis=1)
    assert np.allclose(ln, 3.0, rtol=1e-6)
    ext = np.abs(o[cls == E.EXTREME_ORIGIN])
    assert (ext == F32(2.0 ** -40)).any() and (ext == F32(2.0 ** 60)).any() and ((ext > 0) & (ext < 1.2e-38)).any()
    # origins of the box class lie on the nodes' own coordinates
    bo = E._roll(o[cls == E.BOX_ORIGIN], -sc.shift)
    coords = np.concatenate([sc.canon_nodes["bmin"], sc.canon_nodes["bmax"]])
    on = np.array([[np.isin(p[a], coords[:, a]) for a in range(3)] for p in bo])
    assert on.any(1).all() and on.all(1).any() and not on.all()  # corners, and edges or faces


@pytest.mark.parametrize("name", sorted(_by_name))
def test_bounds_from_the_hit_leafs_box(rt2mod, oraclemod, name):
    """bounded_tmax's four kinds: the same hit one ulp above it, a miss at half
    of it, and with the hit leaf's float32 entry distance as the bound the strict
    `<` does not push that leaf: its triangle is not the hit."""
    sc = _by_name[name]
    o, d, _ = E.query_rays(sc, 257)
    dst, tri, tests, _ = oraclemod.closest_hits(sc.tris, o, d, None, "bvh", sc.nodes)
    tmax = E.bounded_tmax(sc, o, d, dst, tri)
    bd, bt, btests, _ = oraclemod.closest_hits(sc.tris, o, d, T.bound_of(tmax), "bvh", sc.nodes)
    i = np.arange(257)
    hit = tri >= 0
    k1, k2, k3 = (hit & (i % 4 == k) for k in (1, 2, 3))
    assert k1.sum() >= 8 and k2.sum() >= 8
    same = k1 & (bt == tri)
    assert same.sum() >= 8 and np.array_equal(bd[same].view(np.uint32), dst[same].view(np.uint32))
    leaf = E.leaf_of_triangle(sc.nodes)
    for r in np.flatnonzero(k1 & ~same):  # a box that does not hold its triangle may be entered beyond the hit
        nd = sc.nodes[leaf[tri[r]]]
        assert E.ray_bounds32(o[r], d[r], nd["bmin"], nd["bmax"]) >= tmax[r] and bt[r] == -1
    assert (bt[k2] == -1).all() and np.array_equal(bd[k2], tmax[k2])
    k3 &= tmax > 0
    assert k3.sum() >= 8
    assert (bt[k3] != tri[k3]).all() and (btests[k3] < tests[k3]).all()


@pytest.mark.parametrize("name", ["displaced-x", "flat-x", "touching"])
def test_query_walk_differs_from_the_array_scan(rt2mod, oraclemod, name):
    sc = _by_name[name]
    o, d, _ = E.query_rays(sc, 193)
    _, tri, _, _ = oraclemod.closest_hits(sc.tris, o, d, None, "bvh", sc.nodes)
    _, scan, tests, visits = oraclemod.closest_hits(sc.tris, o, d, None, "brute")
    assert (tri != scan).sum() >= 20
    assert (tests == len(sc.tris)).all() and (visits == 0).all()


@pytest.mark.parametrize("name", sorted(_by_name))
def test_python_walk_equals_the_oracle(rt2mod, oraclemod, name):
    """Every third query ray through bvh_edge_scenes.walk (float32 numpy box
    distances): the oracle's result and counters."""
    sc = _by_name[name]
    o, d, _ = E.query_rays(sc, 193)
    pick = np.arange(0, 193, 3 if len(sc.nodes) < 100 else 12)
    dst, tri, tests, visits = oraclemod.closest_hits(sc.tris, o[pick], d[pick], None, "bvh", sc.nodes)
    for k, i in enumerate(pick):
        w = E.walk(oraclemod, sc.tris, sc.nodes, o[i], d[i])
        assert (w[0].view(np.uint32), w[1], w[2], w[3]) == (dst[k].view(np.uint32), tri[k], tests[k], visits[k]), i


def test_closest_hits_array_scan_equals_the_query_reference(rt2mod, oraclemod):
    """oracle.closest_hits("brute") against trace_rays_lib.reference on the
    1,217-triangle soup, unbounded and bounded."""
    tris = T.scene_tris("soup", 1217)
    o, d = T.scene_rays("soup", 1217, 193)
    dst, tri, _ = T.scene_ref(oraclemod, "soup", 1217, 193)
    got = oraclemod.closest_hits(tris, o, d)
    assert np.array_equal(got[0].view(np.uint32), dst.view(np.uint32)) and np.array_equal(got[1], tri)
    assert (got[2] == 1217).all() and (got[3] == 0).all()
    tmax = np.where(tri >= 0, dst * F32(0.5), F32(0)).astype(F32)
    tmax[::2] = 0
    bd, bt, _ = T.reference(oraclemod, tris, o, d, tmax)
    got = oraclemod.closest_hits(tris, o, d, T.bound_of(tmax))
    assert np.array_equal(got[0].view(np.uint32), bd.view(np.uint32)) and np.array_equal(got[1], bt)
    assert (bt[1::2] == -1).all() and (bt[::2] >= 0).any()


# ---- the scenes see a changed walk -------------------------------------------------------

MUTANTS = [
    ("skip-threshold", "if (!(dd[i] < 1e-6f && dd[i] > -1e-6f)) {", "if (!(dd[i] < 1e-5f && dd[i] > -1e-5f)) {",
     "displaced-x-jitter"),
    ("near-on-ties", "int nearA = dstA < dstB;", "int nearA = dstA <= dstB;", "touching"),
    ("stack-cap", "sp < 64", "sp < 61", "chain62-interior-0"),
    ("flat-box", "if (tMin >= tMax || tMax < 0.0f) return 1e38f;", "if (tMin > tMax || tMax < 0.0f) return 1e38f;",
     "flat-x-none"),
    ("minus-zero", "if (tMin >= tMax || tMax < 0.0f) return 1e38f;", "if (tMin >= tMax || tMax <= 0.0f) return 1e38f;",
     "touching"),
]


@pytest.mark.parametrize("what,old,new,name", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_harness_detects_a_changed_walk(rt2mod, oraclemod, tmp_path, what, old, new, name):
    src = open(ORACLE_SRC).read()
    assert old in src
    p = tmp_path / "rt_oracle_mutant.c"
    p.write_text(src.replace(old, new))
    so = str(tmp_path / f"liboracle_{what}.so")
    subprocess.run(["gcc", "-O2", "-std=c11", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fno-math-errno",
                    "-march=x86-64-v3", "-I", ORACLE_DIR, "-shared", "-o", so, str(p), "-lpthread", "-lm"], check=True)
    mutant = oraclemod.load(so)
    # the scene built for this decision: another image or another leaf-test count
    _, ref, _, ref_tests = _image(oraclemod, name)
    _, img, _, tests = _image(oraclemod, name, library=mutant)
    changed = not np.array_equal(ref.view(np.uint32), img.view(np.uint32))
    assert changed or tests != ref_tests, f"{what}: {name} renders the same"
    # and some scene's query rays: another per-ray result or counter
    differ = 0
    for sc in E.query_scenes():
        o, d, _ = E.query_rays(sc, 257)
        a = oraclemod.closest_hits(sc.tris, o, d, None, "bvh", sc.nodes)
        b = oraclemod.closest_hits(sc.tris, o, d, None, "bvh", sc.nodes, library=mutant)
        differ += int(((a[0].view(np.uint32) != b[0].view(np.uint32)) | (a[1] != b[1]) | (a[2] != b[2]) |
                       (a[3] != b[3])).sum())
    assert differ > 0, f"{what}: no query ray differs"
    # the unmutated source compiled the same way is the oracle
    if what == "skip-threshold":
        p.write_text(src)
        subprocess.run(["gcc", "-O2", "-std=c11", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fno-math-errno",
                        "-march=x86-64-v3", "-I", ORACLE_DIR, "-shared", "-o", so + ".same", str(p), "-lpthread",
                        "-lm"], check=True)
        _, img, _, tests = _image(oraclemod, name, library=oraclemod.load(so + ".same"))
        assert np.array_equal(ref.view(np.uint32), img.view(np.uint32)) and tests == ref_tests
