"""MfmaSpec::cluster_rows8 on the CPU: the 8-row fragment (cluster_rows_frag8,
restated in cluster8_scenes.row_model8), the hot mask from the fold's one
ballot (kt8_hot), and the premises of the comb scene that
tests/test_gpu_cluster8.py renders."""
import numpy as np
import pytest

import cluster16_scenes as c16
import cluster8_scenes as c8
import cluster_scenes as cs


def check_rows(need):
    need = int(need)
    lanes = [l for l in range(64) if need >> l & 1]
    c = len(lanes)
    assert 1 <= c <= 8
    dst0, dst1, a8 = c8.row_model8(need)
    # every ds_permute is a permutation of the 64 lanes
    assert sorted(dst0) == list(range(64)) and sorted(dst1) == list(range(64))
    for r in range(8):
        # lane r holds row r's first K-half, lane r + 16 its second: one ray's both
        assert a8[r] not in (None, -1) and a8[r + 16] not in (None, -1)
        assert a8[r][1] == 0 and a8[r + 16][1] == 1 and a8[r][0] == a8[r + 16][0]
        # lanes r + 40 and r + 56 equal lanes r and r + 16
        assert a8[r + 40] == a8[r] and a8[r + 56] == a8[r + 16]
    rows = [a8[r][0] for r in range(8)]
    assert rows[:c] == lanes, "rows 0 .. c - 1 are the needing lanes in order"
    assert all(0 <= x < 64 and not need >> x & 1 for x in rows[c:]), "rows c .. 7 are other lanes of the wave"
    assert len(set(rows)) == 8
    held = {r + o for r in range(8) for o in (0, 16, 40, 56)}
    assert all(a8[l] is None for l in range(64) if l not in held), "every other lane is zero"
    # the rows are those of the 16-row ranking
    assert rows == [x[0] for x in c16.row_model16(need)[2][:8]]
    assert c8.swept_lanes8(need) == set(rows)


def test_rows8_interval_masks():
    """Every interval [x0, x1) of at most 8 columns."""
    n = 0
    for x0 in range(64):
        for x1 in range(x0 + 1, min(64, x0 + 8) + 1):
            check_rows(sum(1 << x for x in range(x0, x1)))
            n += 1
    assert n == sum(min(8, 64 - x0) for x0 in range(64))


def test_rows8_random_masks():
    """10^4 random masks of 1 to 8 bits."""
    rng = np.random.default_rng(8)
    for _ in range(10000):
        c = int(rng.integers(1, 9))
        check_rows(sum(1 << int(x) for x in rng.choice(64, c, replace=False)))


def test_fragment_operand_placement():
    """What the product reads.  Lane l of a 16x16x32 A operand holds row
    l & 15, k-slots 8 (l >> 4) .. + 7 of 32; K-half h of a ray is its k-slots
    8 h .. 8 h + 7 of 16.  Row r < 8 must be [ray | 0] and row r + 8
    [0 | the same ray] over the 32 k-slots."""
    rng = np.random.default_rng(9)
    for _ in range(200):
        c = int(rng.integers(1, 9))
        need = sum(1 << int(x) for x in rng.choice(64, c, replace=False))
        a8 = c8.row_model8(need)[2]
        A = [[None] * 4 for _ in range(16)]  # per row, its four k-quarters
        for l in range(64):
            A[l & 15][l >> 4] = a8[l]
        for r in range(8):
            ray = A[r][0][0]
            assert A[r] == [(ray, 0), (ray, 1), None, None]
            assert A[r + 8] == [None, None, (ray, 0), (ray, 1)]


def test_hot_mask_from_every_single_bit():
    """kt8_hot for a ballot with one bit: lane l of D holds column l & 15 and
    rows 4 (l >> 4) .. + 3; rows below 8 (lanes 0..31) are triangle l & 15,
    the others triangle 16 + (l & 15).  One bit per (row, column): row 4 (l >> 4) + i for every register i."""
    for l in range(64):
        for i in range(4):
            row, col = 4 * (l >> 4) + i, l & 15
            tri = col if row < 8 else col + 16
            assert c8.hot_mask8(1 << l) == 1 << tri, (l, row, col)
    assert c8.hot_mask8(0) == 0 and c8.hot_mask8((1 << 64) - 1) == 0xffffffff
    rng = np.random.default_rng(10)
    for _ in range(1000):
        M = int(rng.integers(0, 1 << 63)) | (int(rng.integers(0, 2)) << 63)
        want = 0
        for l in range(64):
            if M >> l & 1:
                want |= 1 << ((l & 15) + (16 if l >= 32 else 0))
        assert c8.hot_mask8(M) == want


def test_comb8_scene_premises():
    """The scene's evidence sits in both triangle halves (in-group slots 0,
    15, 16 and 31 among them), its clusters have 1, 2, 3 and 5 groups and each
    one's last group carries evidence, a compact one is first and last, the
    last group is ragged with evidence in its upper half, and the needing sets
    of its rows, from rt2_cluster_need of the model's rays, are the required
    ones on both sides of the 8-ray threshold."""
    import rt2
    sc = c8.comb8_scene()
    tris = sc["triangles"]
    assert len(tris) % 32 == c8.RAGGED8 and sc["H"] <= 16
    assert sc["ranges"][0][2] and sc["ranges"][-1][2]
    assert {bd["groups"] for bd in sc["bands"]} == {1, 2, 3, 5}
    slots = set()
    for bd in sc["bands"]:
        slots |= {int(e) & 31 for e in bd["evidence"]}
        g0 = sc["ranges"][bd["k"]][0]
        assert g0 + bd["groups"] - 1 in {int(e) >> 5 for e in bd["evidence"]}, "the cluster's last group has evidence"
        if len(bd["owned"]) >= 4:
            assert {0, 15, 16, 31} <= {int(e) & 31 for e in bd["evidence"]}
        assert np.array_equal(sc["column"][bd["evidence"]], bd["owned"])
    assert {0, 15, 16, 31} <= slots
    last_group = (len(tris) - 1) >> 5
    assert any(int(e) >> 5 == last_group and 16 <= (int(e) & 31) < c8.RAGGED8 for e in sc["bands"][-1]["evidence"])
    u = cs.comb_uniforms(sc["H"], len(tris))
    o, d = cs.camera_rays_model(u)
    t = sc["table"]()
    cs.check_table(t, tris)
    reached = set()
    for bd in sc["bands"]:
        c0, c1, masks = cs.need_counts(t, o, d, bd["k"])
        assert masks[bd["row"]] == sum(1 << x for x in range(bd["x0"], bd["x1"]))
        reached.add((int(c0[bd["row"]]), int(c1[bd["row"]])))
    assert reached == set(c8.REQUIRED8), sorted(set(c8.REQUIRED8) ^ reached)
    assert rt2.MAX_CLUSTERS >= len(sc["ranges"])


@pytest.mark.parametrize("control", range(len(c8.CONTROLS8)))
def test_control_predictions(control):
    """What the row model says of each negative control, worked out before any
    render: the shrunk box's needing set, and whether the victim still rides
    (and as which row)."""
    band, shrink, victim, rides = c8.CONTROLS8[control]
    sc = c8.comb8_scene()
    bd = sc["bands"][band]
    assert victim in bd["owned"] and victim not in range(*shrink)
    mask = sum(1 << x for x in range(*shrink))
    assert 1 <= bin(mask).count("1") <= 8
    assert (victim in c8.swept_lanes8(mask)) == rides
    full = sum(1 << x for x in range(bd["x0"], bd["x1"]))
    assert victim in c8.swept_lanes8(full)
    if control == 2:  # across the threshold: 9 rays before (the 16-row form), 8 after
        assert bin(full).count("1") == 9
    if rides:
        rows = [x[0] for x in c8.row_model8(mask)[2][:8]]
        assert rows.index(victim) == (7 if control == 3 else 6)
