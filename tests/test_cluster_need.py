"""The cluster table and the need test of MfmaSpec::cluster_rows on the CPU
(include/rt2_cluster.h, csrc/host/cluster.cpp; DESIGN.md "Compact clusters").

The kernel skips a compact cluster's groups for a ray whose need bit is 0, so
the test must be conservative: for every ray, the cluster of the triangle the
reference scan (oracle.closest_hits) returns must have its bit set.  Only the
closest hit matters: the scan's result is the nearest accepted triangle,
lowest index on ties, whatever else was accepted on the way.

rt2_cluster_need is the arithmetic the kernel runs; model_need() below is the
same in numpy float32 (asserted bit for bit), so that it can be broken on
purpose: each mutant must fail a named case that the shipped test passes."""
import numpy as np
import pytest

import cluster_scenes as cs

SLACK = np.float32(1.0 + 2.0 ** -16)
DMIN = np.float32(2.0 ** -100)


@pytest.fixture(scope="module")
def scenes(rt2mod, config_scene):
    sd, _ = config_scene("B")
    tris_b = sd.triangles().copy()
    tris_s, _, ranges = cs.strips_scene()
    return {"B": (tris_b, rt2mod.cluster_table(tris_b)),
            "strips": (tris_s, cs.explicit_table(tris_s, ranges)),
            "strips_rule": (tris_s, rt2mod.cluster_table(tris_s))}


# ---------------------------------------------------------------- the table

def test_table_invariants(rt2mod, config_scene, scenes):
    sd_a, _ = config_scene("A")
    ta = rt2mod.cluster_table(sd_a.triangles())
    assert ta["n"] == 0  # two groups that both span the box: nothing compact, the kernel's old loop
    for name, (tris, t) in scenes.items():
        cs.check_table(t, tris)
        assert t["n"] >= 2, name
    # config B: the model's long compact ranges between the groups that span the scene
    tb = scenes["B"][1]
    covered = sum((int(c["g1_flags"]) & 0xffff) - int(c["g0"]) for c in tb["c"][:tb["n"]]
                  if int(c["g1_flags"]) & rt2mod.CLUSTER_COMPACT)
    assert covered >= 24
    # the rule finds the strips scene's blobs on its own
    assert cs.compact_mask(scenes["strips_rule"][1]) != 0


def test_table_degenerate_scenes(rt2mod):
    one = np.zeros(1, dtype=rt2mod.TRI_DTYPE)
    one["b"][0, 0] = one["c"][0, 1] = 1.0
    assert rt2mod.cluster_table(one)["n"] == 0
    assert rt2mod.cluster_table(np.zeros(0, dtype=rt2mod.TRI_DTYPE))["n"] == 0
    # a scene in one plane (surface area of the scene box: two faces only), 6 groups in two far-apart patches
    rng = np.random.default_rng(3)
    n = 192
    a = np.zeros((n, 3), np.float32)
    a[:, :2] = rng.uniform(0, 1, (n, 2)) + np.where(np.arange(n)[:, None] < 96, 0.0, 50.0)
    flat = cs._triangles(a, a + np.float32([0.1, 0, 0]), a + np.float32([0, 0.1, 0]))
    t = rt2mod.cluster_table(flat)
    cs.check_table(t, flat)
    assert t["n"] == 2 and cs.compact_mask(t) == 3
    # out of the filter's range or not finite: no table
    big = flat.copy()
    big["a"][5, 0] = 3e6
    assert rt2mod.cluster_table(big)["n"] == 0
    big["a"][5, 0] = np.nan
    assert rt2mod.cluster_table(big)["n"] == 0


# ------------------------------------------------------------ the need test

def model_need(t, o, d, *, margin=True, nan_needs=True, cut_near=False, tris=None):
    """rt2_cluster_need in numpy float32.  margin=False: the boxes of the
    vertices of `tris` without padding and the comparison without its slack; nan_needs=False: no
    rt2_cluster_always, and a NaN or an overflow decides like any number (a
    false comparison is a miss); cut_near=True: the "behind the origin" cut
    looks at the near distance."""
    o = np.asarray(o, np.float32)
    d = np.asarray(d, np.float32)
    n = int(t["n"])
    with np.errstate(all="ignore"):
        inv = np.float32(1.0) / d
        always = ~(np.abs(d).min(1) > DMIN) | ~(np.abs(o).max(1) <= t["far_o"])
        out_of_range = ~((np.abs(o).max(1) <= np.float32(2.0 ** 20)) & (np.abs(d).max(1) <= np.float32(1.0001)))
        bits = np.zeros(len(o), np.uint32)
        for k, c in enumerate(t["c"][:n]):
            if not int(c["g1_flags"]) & 0x10000:
                bits |= np.uint32(1 << k)
                continue
            lo, hi = c["lo"], c["hi"]
            if not margin:  # the vertices' own box
                glo, ghi = cs.group_boxes(tris)
                g0, g1 = int(c["g0"]), int(c["g1_flags"]) & 0xffff
                lo, hi = glo[g0:g1].min(0).astype(np.float32), ghi[g0:g1].max(0).astype(np.float32)
            t1, t2 = (lo - o) * inv, (hi - o) * inv
            tn = np.fmax(np.fmax(np.fmin(t1, t2)[:, 0], np.fmin(t1, t2)[:, 1]), np.fmin(t1, t2)[:, 2])
            tf = np.fmin(np.fmin(np.fmax(t1, t2)[:, 0], np.fmax(t1, t2)[:, 1]), np.fmax(t1, t2)[:, 2])
            k_slack = SLACK if margin else np.float32(1.0)
            if nan_needs:
                need = ~((tn if cut_near else tf) < 0) & ~(tf * k_slack < tn)
            else:
                need = ((tn if cut_near else tf) >= 0) & (tf * k_slack >= tn)
            bits |= np.where(need, np.uint32(1 << k), np.uint32(0))
        allbits = np.uint32((1 << n) - 1)
        if nan_needs:
            bits = np.where(always, allbits, bits)
        return np.where(out_of_range, allbits, bits)


def unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def box_points(t):
    """Corners, edge midpoints and face centres of every compact box, and the compact boxes."""
    pts, boxes = [], []
    for c in t["c"][:int(t["n"])]:
        if not int(c["g1_flags"]) & 0x10000:
            continue
        lo, hi = c["lo"].astype(np.float64), c["hi"].astype(np.float64)
        boxes.append((c["lo"], c["hi"]))
        for ix in (0, 0.5, 1):
            for iy in (0, 0.5, 1):
                for iz in (0, 0.5, 1):
                    if (ix, iy, iz) != (0.5, 0.5, 0.5):
                        pts.append(lo + (hi - lo) * np.array([ix, iy, iz]))
    return np.array(pts), boxes


def extreme_vertices(t, tris):
    """Of every compact cluster, the vertices that touch its unpadded box (two or more per axis)."""
    v = np.concatenate([tris["a"][:, :3], tris["b"][:, :3], tris["c"][:, :3]]).astype(np.float32)
    owner = np.concatenate([np.arange(len(tris))] * 3)
    out = []
    for k, c in enumerate(t["c"][:int(t["n"])]):
        if not int(c["g1_flags"]) & 0x10000:
            continue
        g0, g1 = int(c["g0"]), int(c["g1_flags"]) & 0xffff
        sel = (owner >= 32 * g0) & (owner < 32 * g1)
        vv = v[sel]
        for ax in range(3):
            out += [vv[vv[:, ax].argmin()], vv[vv[:, ax].argmax()]]
    return np.array(out, np.float32)


def cases(t, tris, seed, n_random):
    """name -> (o, d) float32 arrays."""
    rng = np.random.default_rng(seed)
    v = np.concatenate([tris["a"][:, :3], tris["b"][:, :3], tris["c"][:, :3]])
    slo, shi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
    ext = shi - slo
    out = {}

    def origins(n, inflate=0.25):
        return rng.uniform(slo - inflate * ext, shi + inflate * ext, (n, 3)).astype(np.float32)

    o = origins(n_random)
    out["random"] = (o, unit(rng.normal(size=(n_random, 3))))
    pts, boxes = box_points(t)
    m = 40
    tgt = np.repeat(pts, m, 0)
    o = origins(len(tgt), 0.5)
    out["box corners, edges, faces"] = (o, unit(tgt - o))
    # one or two zero direction components of either sign, aimed so that the others still reach a cluster
    ev = extreme_vertices(t, tris)
    tgt = np.repeat(np.concatenate([ev, pts.astype(np.float32)]), 12, 0)
    o = origins(len(tgt), 0.3)
    dd = (tgt - o).astype(np.float64)
    zero = rng.integers(1, 7, len(tgt))  # bit mask of the axes set to zero, never all three
    for ax in range(3):
        z = (zero >> ax) & 1 == 1
        o[z, ax] = tgt[z, ax]  # the ray still passes through the target
        dd[z, ax] = 0.0
    d = unit(dd)
    for ax in range(3):
        z = (zero >> ax) & 1 == 1
        d[z, ax] = np.where(rng.integers(0, 2, z.sum()) == 1, np.float32(-0.0), np.float32(0.0))
    out["zero direction components"] = (o, d)
    # origins inside the compact boxes and on their faces
    oo = []
    for lo, hi in boxes:
        p = rng.uniform(lo, hi, (300, 3)).astype(np.float32)
        face = rng.integers(0, 6, 150)
        for i, f in enumerate(face):
            p[i, f % 3] = (lo if f < 3 else hi)[f % 3]
        oo.append(p)
    o = np.concatenate(oo)
    out["origins inside and on the boxes"] = (o, unit(rng.normal(size=(len(o), 3))))
    # rays in the plane of a flat cluster (any compact box thinner than its padding allows otherwise)
    oo, dd = [], []
    for lo, hi in boxes:
        ax = int(np.argmin(hi - lo))
        mid = (lo[ax] + hi[ax]) / 2
        p = origins(200, 0.3)
        p[:, ax] = mid
        q = rng.normal(size=(200, 3))
        q[:, ax] = 0.0
        oo.append(p)
        dd.append(unit(q))
    out["in the plane of a flat cluster"] = (np.concatenate(oo), np.concatenate(dd))
    # the filter's range edges: |o| up to 2^20, |d| up to 1.0001 and down to 2^-99 / 2^-101 per component
    tgt = np.repeat(ev, 8, 0)
    far = unit(rng.normal(size=(len(tgt), 3))).astype(np.float64)
    far /= np.abs(far).max(1, keepdims=True)
    scale = np.where(np.arange(len(tgt)) % 2 == 0, 2.0 ** 20, float(t["far_o"]))
    o = (far * scale[:, None] * rng.choice([1.0, 0.999999], (len(tgt), 1))).astype(np.float32)
    o = np.clip(o, -np.float32(2.0 ** 20), np.float32(2.0 ** 20))
    d = unit(tgt.astype(np.float64) - o)
    tgt2 = np.repeat(ev, 4, 0)
    o2 = origins(len(tgt2), 0.3)
    d2 = unit(tgt2.astype(np.float64) - o2)
    s2 = rng.choice([1.0001 / 1.01, 2.0 ** -99, 2.0 ** -101, 2.0 ** -60], (len(tgt2), 1))
    d2 = (d2.astype(np.float64) / np.abs(d2).max(1, keepdims=True) * s2).astype(np.float32)
    out["range edges"] = (np.concatenate([o, o2]), np.concatenate([d, d2]))
    # hit points on, and a few ulp around, the box-defining vertices
    tgt = np.repeat(ev, 200, 0).copy()
    bump = rng.integers(-3, 4, tgt.shape)
    for _ in range(3):
        tgt = np.where(bump > 0, np.nextafter(tgt, np.float32(np.inf)), tgt)
        tgt = np.where(bump < 0, np.nextafter(tgt, np.float32(-np.inf)), tgt)
        bump -= np.sign(bump)
    o = origins(len(tgt), 0.3)
    out["hits within a few ulp of a box face"] = (o, unit(tgt.astype(np.float64) - o))
    # ... and the same targets seen from a point of the box face's own plane, one direction component 0
    tgt = np.repeat(ev, 30, 0)
    ax = np.repeat(np.arange(len(ev)) % 6 // 2, 30)
    o = origins(len(tgt), 0.3)
    dd = tgt.astype(np.float64) - o
    rows = np.arange(len(tgt))
    o[rows, ax] = tgt[rows, ax]
    dd[rows, ax] = 0.0
    out["along a box face through its vertex"] = (o, unit(dd))
    return out


def missed(oraclemod, t, tris, o, d, bits):
    """Rays whose closest hit lies in a compact cluster that `bits` leaves out."""
    _, tri, _, _ = oraclemod.closest_hits(tris, o, d)
    hit = tri >= 0
    k = cs.cluster_of_triangle(t, np.where(hit, tri, 0))
    return hit & ((bits >> k.astype(np.uint32)) & 1 == 0), int(hit.sum())


@pytest.fixture(scope="module")
def evaluated(rt2mod, oraclemod, scenes):
    """Per scene and case: the rays, the library's bits and the oracle's verdict, computed once."""
    out = {}
    for name, n_random in (("B", 100_000), ("strips", 100_000)):
        tris, t = scenes[name]
        for case, (o, d) in cases(t, tris, 7, n_random).items():
            bits = rt2mod.cluster_need(t, o, d)
            out[(name, case)] = (o, d, bits)
    return out


CASES = ["random", "box corners, edges, faces", "zero direction components", "origins inside and on the boxes",
         "in the plane of a flat cluster", "range edges", "hits within a few ulp of a box face",
         "along a box face through its vertex"]


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("scene", ["B", "strips"])
def test_need_is_conservative(oraclemod, scenes, evaluated, scene, case):
    tris, t = scenes[scene]
    o, d, bits = evaluated[(scene, case)]
    bad, hits = missed(oraclemod, t, tris, o, d, bits)
    print(f"{scene} / {case}: {len(o)} rays, {hits} hits, "
          f"{np.mean([bin(b & cs.compact_mask(t)).count('1') for b in bits[:2000]]):.2f} compact clusters needed per ray")
    assert not bad.any(), f"{bad.sum()} rays lose their hit, first: o {o[bad][0]}, d {d[bad][0]}"
    # the case is not empty-handed: outside the degenerate ones, rays do hit compact clusters
    if case not in ("in the plane of a flat cluster", "range edges"):
        assert hits > 0


@pytest.mark.parametrize("scene", ["B", "strips"])
def test_model_is_the_library(scenes, evaluated, scene):
    _, t = scenes[scene]
    for case in CASES:
        o, d, bits = evaluated[(scene, case)]
        assert np.array_equal(model_need(t, o, d), bits), case


def test_need_is_selective(scenes, evaluated):
    """Not a correctness property, but what the knob lives on: a random ray of config B needs few compact clusters."""
    _, t = scenes["B"]
    _, _, bits = evaluated[("B", "random")]
    per_ray = np.array([bin(int(b) & cs.compact_mask(t)).count("1") for b in bits[:20000]])
    assert per_ray.mean() < 0.6 * bin(cs.compact_mask(t)).count("1")


MUTANTS = {
    # without the padding and the slack, rounding alone loses hits on the vertices that define a box
    "no margin": (dict(margin=False), ["hits within a few ulp of a box face"]),
    # without the padding, a ray along a box face through its vertex multiplies 0 by infinity: NaN must need
    "NaN is a miss": (dict(margin=False, nan_needs=False), ["along a box face through its vertex"]),
    # "behind the origin" is a statement about the far distance only
    "cut on the near side": (dict(cut_near=True), ["origins inside and on the boxes"]),
}


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_mutants_fail(oraclemod, scenes, evaluated, mutant):
    kw, named = MUTANTS[mutant]
    tris, t = scenes["strips"]
    for case in named:
        o, d, _ = evaluated[("strips", case)]
        bad, _ = missed(oraclemod, t, tris, o, d, model_need(t, o, d, tris=tris, **kw))
        assert bad.any(), f"mutant '{mutant}' passes '{case}'"
    if mutant == "NaN is a miss":
        # the control: the same boxes without padding, NaN needing, lose nothing there that NaN explains
        o, d, _ = evaluated[("strips", named[0])]
        ctrl, _ = missed(oraclemod, t, tris, o, d, model_need(t, o, d, margin=False, tris=tris))
        mut, _ = missed(oraclemod, t, tris, o, d, model_need(t, o, d, tris=tris, **kw))
        assert (mut & ~ctrl).any()


# ------------------------------------------ comb scenes and the row assignment
#
# The premises of tests/test_gpu_cluster_private.py that need no GPU.

@pytest.fixture(scope="module")
def combs(rt2mod):
    """Per comb scene: the scene, its explicit table, its primary rays (numpy model of advance())."""
    out = {}
    for name in list(cs.COMB_SCENES) + ["full", "ragged"]:
        sc = cs.named_comb_scene(name)
        u = cs.comb_uniforms(sc["H"], len(sc["triangles"]))
        out[name] = (sc, sc["table"](), *cs.camera_rays_model(u))
    return out


def test_comb_need_sets(rt2mod, combs):
    """Every band's row has the needing set of its interval and every other row
    none; over the scenes the (c0, c1) the GPU tests stand on are all reached."""
    reached = set()
    for name, (sc, t, o, d) in combs.items():
        cs.check_table(t, sc["triangles"])
        assert cs.compact_mask(t) == sum(1 << bd["k"] for bd in sc["bands"])
        bits = rt2mod.cluster_need(t, o, d)
        assert np.all(bits | cs.compact_mask(t) == (1 << t["n"]) - 1)  # the walls
        for band, bd in enumerate(sc["bands"]):
            c0, c1, masks = cs.need_counts(t, o, d, bd["k"])
            want = sum(1 << x for x in range(bd["x0"], bd["x1"]))
            for row in range(sc["H"]):
                assert masks[row] == (want if row == bd["row"] else 0), (name, band, row)
            reached |= set(zip(c0.tolist(), c1.tolist()))
    print("(c0, c1) reached:", sorted(reached))
    missing = [c for c in cs.COMB_REQUIRED if c not in reached]
    assert not missing, missing
    assert any(a and b and a + b < 32 for a, b in reached)


def test_comb_ownership(oraclemod, combs):
    """The reference scan gives every owned column its evidence triangle and every other pixel wall triangle 0."""
    for name, (sc, t, o, d) in combs.items():
        _, tri, _, _ = oraclemod.closest_hits(sc["triangles"], o, d)
        want = np.full((sc["H"], cs.COMB_W), sc["wall_tri"], np.int64)
        for bd in sc["bands"]:
            assert len(bd["owned"]) == -(-(bd["x1"] - bd["x0"]) // sc["pitch"])
            want[bd["row"], bd["owned"]] = bd["evidence"]
            # every group of the cluster holds evidence (where there are as many owned columns as groups)
            assert len(set((bd["evidence"] >> 5).tolist())) == min(bd["groups"], len(bd["owned"]))
        assert np.array_equal(tri.reshape(want.shape), want), name


def test_comb_controls(rt2mod, combs):
    """A shrunk box is well-formed and leaves out exactly the victim's ray."""
    for name, band, (x0, x1), victim in cs.COMB_CONTROLS:
        sc, t, o, d = combs[name]
        bd = sc["bands"][band]
        assert victim in bd["owned"] and bd["x0"] <= x0 < x1 <= bd["x1"]
        ts = sc["table"]({band: (x0, x1)})
        k = bd["k"]
        assert np.all(ts["c"][k]["lo"] < ts["c"][k]["hi"])
        before, after = cs.need_counts(t, o, d, k)[2], cs.need_counts(ts, o, d, k)[2]
        assert before[bd["row"]] ^ after[bd["row"]] == 1 << victim
        other = np.arange(t["n"]) != k
        assert all(np.array_equal(cs.need_counts(t, o, d, k)[2], cs.need_counts(ts, o, d, k)[2])
                   for k in np.flatnonzero(other))


def check_rows(need):
    rows0, rows1, src = cs.row_model(need)
    lanes = [l for l in range(64) if need >> l & 1]
    c0 = sum(1 for l in lanes if l < 32)
    assert sorted(rows0) == list(range(32)) and sorted(rows1) == list(range(32))  # each block: a permutation
    assert src[:len(lanes)] == lanes                                           # rows 0 .. c - 1: the needing lanes
    assert all(s >= 32 for s in src[c0:])                                      # ... all others from block 1
    assert not any(s < 32 and not need >> s & 1 for s in src)                  # no filler from block 0
    assert len(set(src)) == 32


def test_row_model():
    """The row assignment of cluster_rows_frag (rk, rest, the `first` select),
    restated in cluster_scenes.row_model: for every interval of lanes and 10^4
    random masks of at most 32 bits, each block's rows are a permutation, the
    result holds the needing lanes in rows 0 .. c - 1 in lane order, and a lane
    of block 0 that does not need the cluster is never in the result."""
    n = 0
    for a in range(64):
        for b in range(a, min(a + 32, 64) + 1):
            check_rows(sum(1 << l for l in range(a, b)))
            n += 1
    rng = np.random.default_rng(11)
    for _ in range(10_000):
        c = int(rng.integers(0, 33))
        # all over the wave, or crowded into one block and a little of the other
        if rng.random() < 0.5:
            lanes = rng.choice(64, c, replace=False)
        else:
            k = int(rng.integers(0, min(c, 4) + 1))
            blk = int(rng.integers(0, 2))
            lanes = np.concatenate([32 * blk + rng.choice(32, c - k, replace=False),
                                    32 * (1 - blk) + rng.choice(32, k, replace=False)])
        check_rows(sum(1 << int(l) for l in lanes))
    assert n > 1500
    # the fillers are block 1's first lanes that do not need the cluster
    assert cs.row_model(sum(1 << l for l in range(20, 44)))[2][24:] == list(range(44, 52))
    assert cs.swept_lanes(0) == set() and cs.swept_lanes((1 << 33) - 1) == set(range(64))
