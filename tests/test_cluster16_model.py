"""MfmaSpec::cluster_rows16 on the CPU: the 16-row fragment's destinations
(cluster_rows_frag16, restated in cluster16_scenes.row_model16), the record
lane each lane of a 16-row product reads (kt16_record_lane), and the premises of
the comb scene that tests/test_gpu_cluster16.py renders."""
import numpy as np
import pytest

import cluster16_scenes as c16
import cluster_scenes as cs


def check_rows(need):
    need = int(need)
    lanes = [l for l in range(64) if need >> l & 1]
    c = len(lanes)
    dst0, dst1, alo, ahi = c16.row_model16(need)
    # every ds_permute is a permutation of the 64 lanes
    assert sorted(dst0) == list(range(64)) and sorted(dst1) == list(range(64))
    assert -1 not in alo[:32]
    for r in range(16):
        # lane r holds row r's first K-half, lane r + 16 its second: one ray's both
        assert alo[r][1] == 0 and alo[r + 16][1] == 1 and alo[r][0] == alo[r + 16][0]
    rows = [alo[r][0] for r in range(16)]
    assert rows[:c] == lanes, "rows 0 .. c - 1 are the needing lanes in order"
    assert all(0 <= x < 64 and not need >> x & 1 for x in rows[c:]), "rows c .. 15 are other lanes of the wave"
    assert len(set(rows)) == 16
    assert alo[32:] == [None] * 32, "lanes 32..63 of alo are zero"
    assert ahi[:32] == [None] * 32 and ahi[32:] == alo[:32], "ahi is alo with its halves exchanged"
    assert c16.swept_lanes16(need) == set(rows)


def test_rows16_interval_masks():
    """Every interval [x0, x1) of at most 16 columns."""
    n = 0
    for x0 in range(64):
        for x1 in range(x0 + 1, min(64, x0 + 16) + 1):
            check_rows(sum(1 << x for x in range(x0, x1)))
            n += 1
    assert n == sum(min(16, 64 - x0) for x0 in range(64))


def test_rows16_random_masks():
    """10^4 random masks of 1 to 16 bits."""
    rng = np.random.default_rng(16)
    for _ in range(10000):
        c = int(rng.integers(1, 17))
        check_rows(sum(1 << int(x) for x in rng.choice(64, c, replace=False)))


def test_rows16_agrees_with_the_32_row_ranking():
    """The ranking is cluster_rows_frag's: the 16 rows are the first 16 of the 32-row fragment of the same mask."""
    rng = np.random.default_rng(17)
    for _ in range(2000):
        c = int(rng.integers(1, 17))
        need = sum(1 << int(x) for x in rng.choice(64, c, replace=False))
        rows = [x[0] for x in c16.row_model16(need)[2][:16]]
        assert rows == cs.row_model(need)[2][:16]


def test_record_lane_map():
    """kt16_record_lane is a bijection of the 64 record lanes.  Record lane
    j + 32 h holds triangle j's k-slots 8 h .. 8 h + 7 (the 32x32x16 layout);
    lane l of a 16x16x32 B operand holds column l & 15, k-slots 8 (l >> 4) ..
    + 7 of 32.  Column j must hold triangle j's 16 slots in k-slots 0..15 and
    triangle j + 16's in 16..31, and a lane keeps its 16-byte slot of the
    256-byte bank row (the premise of DESIGN.md's bank-rule argument, which the
    hardware's conflict counter did not bear out: "16-row products")."""
    m = [c16.record_lane16(l) for l in range(64)]
    assert sorted(m) == list(range(64))
    for l in range(64):
        col, kq = l & 15, l >> 4          # the B operand's column and k-slot quarter
        tri, half = m[l] & 31, m[l] >> 5  # what the record lane holds
        assert tri == col + 16 * (kq >> 1) and half == (kq & 1)
        assert m[l] % 16 == l % 16


def test_comb16_scene_premises():
    """The scene's evidence sits in both triangle halves (in-group indices 0,
    15, 16 and 31 among them), its clusters have 1, 2 and 3 groups, a compact
    one is first and last, the last group is ragged, and the needing sets
    of its rows, from rt2_cluster_need of the model's rays, include the
    required ones on both sides of the 16-ray threshold."""
    import rt2
    sc = c16.comb16_scene()
    tris = sc["triangles"]
    assert len(tris) % 32 == c16.RAGGED16
    assert sc["ranges"][0][2] and sc["ranges"][-1][2]
    assert {bd["groups"] for bd in sc["bands"]} == {1, 2, 3}
    slots = set()
    for bd in sc["bands"]:
        slots |= {int(e) & 31 for e in bd["evidence"]}
        if len(bd["owned"]) >= 4:
            assert {0, 15, 16, 31} <= {int(e) & 31 for e in bd["evidence"]}
        assert np.array_equal(sc["column"][bd["evidence"]], bd["owned"])
    assert {0, 15, 16, 31} <= slots and any(s < 16 for s in slots) and any(s >= 16 for s in slots)
    u = cs.comb_uniforms(sc["H"], len(tris))
    o, d = cs.camera_rays_model(u)
    t = sc["table"]()
    cs.check_table(t, tris)
    reached = set()
    for bd in sc["bands"]:
        c0, c1, masks = cs.need_counts(t, o, d, bd["k"])
        assert masks[bd["row"]] == sum(1 << x for x in range(bd["x0"], bd["x1"]))
        reached.add((int(c0[bd["row"]]), int(c1[bd["row"]])))
    assert set(c16.REQUIRED16) <= reached, sorted(set(c16.REQUIRED16) - reached)
    assert rt2.MAX_CLUSTERS >= len(sc["ranges"])


@pytest.mark.parametrize("control", range(len(c16.CONTROLS16)))
def test_control_predictions(control):
    """What the row model says of each negative control, worked out before any
    render: the shrunk box's needing set, and whether the victim still rides."""
    band, shrink, victim = c16.CONTROLS16[control]
    sc = c16.comb16_scene()
    bd = sc["bands"][band]
    assert victim in bd["owned"] and victim not in range(*shrink)
    mask = sum(1 << x for x in range(*shrink))
    assert bin(mask).count("1") <= 16
    rides = victim in c16.swept_lanes16(mask)
    assert rides == (control >= 3)
