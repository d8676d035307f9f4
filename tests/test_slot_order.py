"""The slot order on the CPU (rt2_cluster_order_build; DESIGN.md "Slot order"):
the order is a deterministic permutation, its table is a table of the permuted
triangles and conservative for them, small scenes keep the index order, the
slot scan with the tie rule is the reference's index scan, and the rule's own
table is close to the best one for its order on the model rays."""
import numpy as np
import pytest

import cluster_scenes as cs
import slot_order_model as som
import slot_order_scenes as sos
import test_cluster_need as tcn


@pytest.fixture(scope="module")
def scenes(rt2mod, config_scene):
    """name -> triangles"""
    out = {"B": config_scene("B")[0].triangles(), "strips": cs.strips_scene()[0]}
    for name in ("one", "two", "full", "ragged"):
        out[name] = cs.named_comb_scene(name)["triangles"]
    return out


SCENES = ["B", "strips", "one", "two", "full", "ragged"]


@pytest.mark.parametrize("scene", SCENES)
def test_order_is_a_deterministic_permutation(rt2mod, scenes, scene):
    tris = scenes[scene]
    st, t = rt2mod.cluster_order(tris)
    st2, t2 = rt2mod.cluster_order(tris.copy())
    assert np.array_equal(np.sort(st), np.arange(len(tris)))
    assert np.array_equal(st, st2) and t.tobytes() == t2.tobytes()
    moved = not np.array_equal(st, np.arange(len(tris)))
    print(f"{scene}: {'regrouped' if moved else 'index order'}, {int(t['n'])} clusters")
    if not moved:
        assert t.tobytes() == rt2mod.cluster_table(tris).tobytes(), "the identity comes with the index-order table"
    # inside a group the triangles ascend by index
    for g in range(0, len(st), 32):
        assert np.all(np.diff(st[g:g + 32]) > 0)
    cs.check_table(t, np.ascontiguousarray(tris[st]))


def test_config_B_is_regrouped(rt2mod, scenes):
    """Config B is the scene the rule is for: it must not come out as the identity, and the scene-spanning
    triangles (the appended box's) share the one full cluster in front."""
    tris = scenes["B"]
    st, t = rt2mod.cluster_order(tris)
    assert not np.array_equal(st, np.arange(len(tris)))
    flags = [int(c["g1_flags"]) for c in t["c"][:int(t["n"])]]
    assert not flags[0] & rt2mod.CLUSTER_COMPACT and all(f & rt2mod.CLUSTER_COMPACT for f in flags[1:])
    assert rt2mod.cluster_table(tris)["n"] > 0  # rt2_cluster_table_build is untouched (its tests pin the rest)


def test_small_scenes_keep_the_index_order(rt2mod, config_scene):
    one = cs.strips_scene()[0][:1]
    for name, tris in (("A", config_scene("A")[0].triangles()), ("one triangle", one), ("empty", one[:0])):
        st, t = rt2mod.cluster_order(tris)
        assert np.array_equal(st, np.arange(len(tris))), name
        assert t.tobytes() == rt2mod.cluster_table(tris).tobytes(), name
        if name != "one triangle":
            assert t["n"] == 0, name


@pytest.mark.parametrize("scene", SCENES)
def test_slot_need_is_conservative(rt2mod, oraclemod, scenes, scene):
    """For 10^5 random rays and the box-corner, edge and face rays of tests/test_cluster_need.py: the slot cluster
    of the closest hit's triangle has its need bit set."""
    tris = scenes[scene]
    st, t = rt2mod.cluster_order(tris)
    if t["n"] == 0:
        print(f"{scene}: no compact cluster in the table, every ray sweeps every group")
        return
    perm = np.ascontiguousarray(tris[st])
    all_cases = tcn.cases(t, perm, 11, 100_000)
    for case in ("random", "box corners, edges, faces"):
        o, d = all_cases[case]
        bits = rt2mod.cluster_need(t, o, d)
        bad, hits = tcn.missed(oraclemod, t, perm, o, d, bits)
        print(f"{scene} / {case}: {len(o)} rays, {hits} hits")
        assert hits > 0 and not bad.any(), f"{bad.sum()} rays lose their hit"


# ------------------------------------------------------ the scan's tie rule

@pytest.fixture(scope="module")
def tie_eval(oraclemod):
    """The tie scene's primary rays, the reference's test of every (ray, triangle) pair and its index scan's hits."""
    sc = sos.tie_scene()
    tris = sc["triangles"]
    o, d = cs.camera_rays_model(cs.comb_uniforms(sc["H"], len(tris)))
    dst = sos.hit_distances(oraclemod, tris, o, d)
    _, ref, _, _ = oraclemod.closest_hits(tris, o, d)
    return sc, dst, ref


def test_tie_scene_premises(tie_eval):
    sc, dst, ref = tie_eval
    for name, i, j, row, col in sc["pairs"]:
        r = 64 * row + col
        assert i < j and ref[r] == i, name
        assert np.isfinite(dst[r, i]) and dst[r, i] == dst[r, j] == dst[r].min(), name
        assert np.flatnonzero(sc["slot_tri"] == i)[0] > np.flatnonzero(sc["slot_tri"] == j)[0], name


@pytest.mark.parametrize("order", ["identity", "reversed", "random", "pairs exchanged"])
def test_slot_scan_is_the_index_scan(tie_eval, order):
    sc, dst, ref = tie_eval
    n = dst.shape[1]
    st = sc["slot_tri"] if order == "pairs exchanged" else sos.orders(n)[order]
    assert np.array_equal(sos.slot_scan(dst, st), ref)


def test_strict_rule_mutant_fails(tie_eval):
    """The scan with `dst < best` alone gives every pair's pixel to the higher index under the exchanged order
    (and under the reversed one): the scene can see the rule."""
    sc, dst, ref = tie_eval
    n = dst.shape[1]
    assert np.array_equal(sos.slot_scan(dst, np.arange(n), tie_rule=False), ref)
    for st in (sc["slot_tri"], sos.orders(n)["reversed"]):
        got = sos.slot_scan(dst, st, tie_rule=False)
        for name, i, j, row, col in sc["pairs"]:
            assert got[64 * row + col] == j, f"the case '{name}' does not see the tie rule"
    wrong = np.flatnonzero(sos.slot_scan(dst, sc["slot_tri"], tie_rule=False) != ref)
    assert len(wrong) == len(sc["pairs"])


# ------------------------------------------------------------ the cost model

@pytest.mark.parametrize("dead", [0.0, 0.35])
def test_rule_table_is_near_the_best_for_its_order(rt2mod, scenes, dead):
    """On the model rays (tests/slot_order_model.py, fixed seed; all lanes live, and 35 % of them dead): the rule's
    table costs at most 1.05 x the best contiguous table of the rule's order, every price known.  The margin is
    for a rule that sees only the geometry."""
    tris, rays = som.model_rays()
    st, t = rt2mod.cluster_order(tris)
    if dead:
        rays = som.kill_lanes(rays, dead)
    perm = np.ascontiguousarray(tris[st])
    own = som.table_cost(t, rays)
    ranges, best = som.best_contiguous_table(perm, rays, t)
    index = som.table_cost(rt2mod.cluster_table(tris), rays)
    print(f"dead lanes {dead}: index order, shipped table {index:.1f}; rule's order and table {own:.1f}; "
          f"best table of the rule's order {best:.1f} {ranges}")
    assert own <= 1.05 * best
    assert own < index
