"""The bookkeeping of the per-ray exact episode (MfmaSpec::exact_lanes) on a
numpy model, without a GPU: the compaction against a plain sort at every hot
count 0..96 and at random masks, and the bit <-> row map with the pack and the
block swap against the definition (bit b of ray r = r passes the round's b-th
triangle)."""
import numpy as np
import pytest

import exact_lanes_model as M


def _plain(masks, gw, n_tris):
    idx = sorted(32 * (gw + j) + b for j, m in enumerate(masks) for b in range(32) if int(m) >> b & 1)
    idx = [i for i in idx if i < n_tris]
    return [idx[k:k + 32] for k in range(0, len(idx), 32)]


def test_row_map_is_a_permutation():
    rows = [M.row_of_bit(b) for b in range(32)]
    assert sorted(rows) == list(range(32))
    assert all(M.bit_of_row(M.row_of_bit(b)) == b for b in range(32))
    # the product's result layout: lane l, register i holds row 8 (i >> 2) + 4 (l >> 5) + (i & 3)
    for lane in (0, 31, 32, 63):
        for i in range(16):
            assert M.row_of_bit(i + 16 * (lane >> 5)) == 8 * (i >> 2) + 4 * (lane >> 5) + (i & 3)


@pytest.mark.parametrize("hot", range(97))
def test_compaction_every_hot_count(hot):
    rng = np.random.default_rng(hot)
    n_tris = 38 * 32
    pick = np.sort(rng.choice(n_tris, size=hot, replace=False))
    masks = [0] * 38
    for i in pick:
        masks[i >> 5] |= 1 << (i & 31)
    rounds = M.compact(masks, 0, n_tris)
    assert rounds == _plain(masks, 0, n_tris)
    assert len(rounds) == -(-hot // 32)
    assert [i for r in rounds for i in r] == [int(i) for i in pick]


@pytest.mark.parametrize("seed", range(20))
def test_compaction_random_masks(seed):
    rng = np.random.default_rng(1000 + seed)
    gw = int(rng.choice([0, 38]))
    cnt = int(rng.integers(1, 39))
    dens = rng.choice([0.02, 0.1, 0.5, 1.0])
    masks = [int(sum(1 << b for b in range(32) if rng.random() < dens)) for _ in range(cnt)]
    # the scene ends inside the window's last group, at its end, or beyond the window
    for n_tris in (32 * (gw + cnt) - 13, 32 * (gw + cnt), 32 * (gw + cnt) + 40):
        assert M.compact(masks, gw, n_tris) == _plain(masks, gw, n_tris)


def test_padding_never_listed():
    # every mask full, 1,203 triangles: the last group's 13 padding slots stay out
    rounds = M.compact([0xFFFFFFFF] * 38, 0, 32 * 38 - 13)
    flat = [i for r in rounds for i in r]
    assert flat == list(range(32 * 38 - 13))


@pytest.mark.parametrize("c", [1, 15, 16, 17, 31, 32])
@pytest.mark.parametrize("upper", [True, False])
def test_ray_masks(c, upper):
    rng = np.random.default_rng(c)
    passes = rng.random((64, c)) < 0.3
    passes[5, :] = True   # one ray with every pair
    passes[40, :] = False  # and one with none
    pm = M.ray_masks(passes, upper)
    for ray in range(64):
        want = sum(1 << s for s in range(c) if passes[ray, s])
        if ray >= 32 and not upper:
            want = 0  # lanes 32..63 hold no ray of their own
        assert int(pm[ray]) == want, f"ray {ray}"


def test_one_ray_per_triangle():
    # slot s is hit by ray 2 s + 1 alone: decodes the permutation and the swap
    passes = np.zeros((64, 32), dtype=bool)
    for s in range(32):
        passes[2 * s + 1, s] = True
    pm = M.ray_masks(passes)
    assert all(int(pm[2 * s + 1]) == 1 << s for s in range(32))
    assert all(int(pm[2 * s]) == 0 for s in range(32))


# ---- the scenes of tests/test_gpu_exact_lanes.py, on the oracle alone ----------------

def _oracle_winners(oraclemod, tris, mats, u):
    import closest_hit_scenes as S
    acc, _, segs, _ = oraclemod.render(tris, mats, u, np.arange(u.height, dtype=np.int32), 0, 1, "brute")
    return S.decode(acc), segs


@pytest.mark.parametrize("w,h", [(8, 4), (11, 3)])
def test_scene_one_ray_each(rt2mod, oraclemod, w, h):
    import exact_lanes_scenes as X
    tris, mats, u, order = X.one_ray_each(w, h)
    idx, segs = _oracle_winners(oraclemod, tris, mats, u)
    assert np.array_equal(idx.ravel(), order) and segs == w * h
    assert sorted(order.tolist()) == list(range(w * h)) and not np.array_equal(order, np.arange(w * h))


def test_scene_ties(rt2mod, oraclemod):
    import closest_hit_scenes as S
    import exact_lanes_scenes as X
    tris, mats = X.plane_fan(X.TIE_N, X.TIE_FAMILIES)
    idx, _ = _oracle_winners(oraclemod, tris, mats, S.coded_uniforms(64, 36, X.TIE_N))
    for (lo, hi), _ in X.TIE_FAMILIES:
        assert all(np.array_equal(tris[k][lo], tris[k][hi]) for k in "abc")
        assert (idx == lo).sum() >= 64 and (idx == hi).sum() == 0, (lo, hi)
    assert (idx >= 0).all()


def test_scene_one_ray_against_63(rt2mod, oraclemod):
    import exact_lanes_scenes as X
    tris, mats, u = X.one_ray_many(8, 8, 40, 5, 3)
    idx, _ = _oracle_winners(oraclemod, tris, mats, u)
    assert idx[3, 5] == 39 and (idx >= 0).sum() == 1
    tris, mats, u = X.all_rays_but_one(8, 8, 40)
    idx, _ = _oracle_winners(oraclemod, tris, mats, u)
    assert idx[0, 0] == -1 and (idx == 39).sum() == 63
