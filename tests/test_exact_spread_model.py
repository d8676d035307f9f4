"""MfmaSpec::exact_spread's bookkeeping on a model, without a GPU
(tests/exact_spread_scenes.py episode: first pair on its own lane, prefix sum,
scatter, one worker per leftover against the bound after the first pair, merge
by the minimum of (distance bits, index)) against the sequential scan in slot
order with mt_exact_slot's rule: one ray with every pattern of up to 6 pairs,
every mask of 2 rays x 6 slots, 3 x 5 and 4 x 4, 4 rays of up to 6 pairs each
by classes with every vector of counts, 10^4 random episodes with equal
distances whose lower index sits in a later slot, and what the GPU tests'
scenes are built to give."""
import itertools

import numpy as np
import pytest

import exact_spread_scenes as E

# distances of the enumeration: two equal values, so every tie pattern occurs; None = the exact test rejects
DISTS = (None, np.float32(1.0), np.float32(2.0))


def _same(pairs, slot_tri):
    want = E.scan(pairs, slot_tri)
    got, cnt = E.episode(pairs, slot_tri)
    assert got == want, (pairs, list(slot_tri), got, want)
    return cnt


def test_one_ray_every_pattern_and_order():
    """One ray, up to 6 pairs, every pattern of {rejected, 1.0, 2.0} and, up to 4 pairs, every slot order."""
    spread = 0
    for n in range(1, 7):
        orders = itertools.permutations(range(n)) if n <= 4 else [tuple(range(n)), tuple(reversed(range(n)))]
        for slot_tri in orders:
            for ds in itertools.product(DISTS, repeat=n):
                spread += _same([dict(enumerate(ds))], slot_tri)["spread"]
    assert spread > 0


# distance patterns of the mask enumerations, dist(slot, ray) (None: the exact test rejects the pair), and slot orders
PATTERNS = {
    "two_values": lambda s, k: np.float32(1.0 + (s * 5 % 3 == 0)) if (s + k) % 4 else None,  # ties and rejects
    "near_last": lambda s, k: np.float32(3.0 - 0.25 * s),  # every test improves the bound
    "all_equal": lambda s, k: np.float32(1.0) if (s + 2 * k) % 5 else None,  # the index alone decides
}
ORDERS = {"identity": lambda n: tuple(range(n)), "reversed": lambda n: tuple(reversed(range(n))),
          "rotated": lambda n: tuple((s + n // 2) % n for s in range(n))}


@pytest.mark.parametrize("pattern,order", [("two_values", "reversed"), ("two_values", "rotated"),
                                           ("near_last", "identity"), ("all_equal", "reversed")])
@pytest.mark.parametrize("rays,slots", [(2, 6), (3, 5), (4, 4)])
def test_every_mask(rays, slots, pattern, order):
    """Every subset of the slots for every ray (which ray holds which slot decides the hot list's bits, the prefix
    sum and the list's places): 2 rays x 6 slots, 3 x 5 and 4 x 4, under four combinations of a distance pattern
    and a slot order.  (4 rays x 6 slots in full is 2^24 masks per pattern; test_four_rays_up_to_six_pairs covers that size
    by classes.)"""
    slot_tri = ORDERS[order](slots)
    dist = [[PATTERNS[pattern](s, k) for s in range(slots)] for k in range(rays)]
    took = 0
    for masks in itertools.product(range(1 << slots), repeat=rays):
        pairs = [{s: dist[k][s] for s in range(slots) if m >> s & 1} for k, m in enumerate(masks)]
        took += _same(pairs, slot_tri)["spread"]
    assert took > 0


def _ray_classes(c):
    """The classes of a ray with c pairs: (p, kind) with p the position of its nearest pair among its own and
    kind: plain; tie_first / tie_last (its first / last pair lies at the nearest's distance too); rej_first (the
    exact test rejects its first pair)."""
    out = []
    for p in range(c):
        out.append((p, "plain"))
        if p != 0:
            out += [(p, "tie_first"), (p, "rej_first")]
        if p != c - 1:
            out.append((p, "tie_last"))
    return out or [(0, "none")]


def _ray_pairs(k, c, p, kind):
    """Ray k's c pairs, its j-th in slot 4 j + k (the rays' bits interleave in the hot list): the nearest at 1.0,
    the others behind it at distinct distances."""
    d = [np.float32(2.0 + 0.125 * j) for j in range(c)]
    if c:
        d[p] = np.float32(1.0)
    if kind == "tie_first":
        d[0] = np.float32(1.0)
    elif kind == "tie_last":
        d[-1] = np.float32(1.0)
    elif kind == "rej_first":
        d[0] = None
    return {4 * j + k: d[j] for j in range(c)}


@pytest.mark.parametrize("ray", range(4))
def test_four_rays_up_to_six_pairs(ray):
    """4 rays with 0..6 pairs each: every vector of the four counts (all the prefix sum and the scatter can see) x
    every class of ray `ray` (_ray_classes: where its nearest pair sits among the first pair and the leftovers, the
    ties with its first and last pair, a rejected first pair), the other rays in a class that changes from case to
    case, in identity and reversed slot order (the tie's lower index in the earlier and in the later slot).  Per
    value of `ray` 7^3 x 67 x 2 episodes.  Rw reaches 20, a ray 5 leftovers."""
    orders = [ORDERS[o](24) for o in ("identity", "reversed")]
    seen, n, rw_max = set(), 0, 0
    for others in itertools.product(range(7), repeat=3):
        for c in range(7):
            counts = list(others[:ray]) + [c] + list(others[ray:])
            for ci, (p, kind) in enumerate(_ray_classes(c)):
                pairs = []
                for k in range(4):
                    if k == ray:
                        pairs.append(_ray_pairs(k, c, p, kind))
                    else:
                        cl = _ray_classes(counts[k])
                        pairs.append(_ray_pairs(k, counts[k], *cl[(n + 3 * k + ci) % len(cl)]))
                n += 1
                for slot_tri in orders:
                    cnt = _same(pairs, slot_tri)
                    seen.update(k for k in ("spread", "small") if cnt[k])
                    rw_max = max(rw_max, cnt["leftovers"])
    assert n == 7 ** 3 * 67 and seen == {"spread", "small"} and rw_max == 20


def test_random_episodes():
    """10^4 episodes of up to 64 rays: most with up to 11 hot slots, one in twenty with up to 80 (three rounds) at
    a lower density; few distinct distances, so equal distances with the lower index in a later slot are common;
    random slot orders; the fallback rounds (no lane with two leftovers, more than 64 leftovers) occur among them."""
    rng = np.random.default_rng(20)
    seen = dict(spread=0, big=0, small=0, ties=0)
    for _ in range(10000):
        big = rng.random() < 0.05
        rays = int(rng.integers(1, 65)) if big or rng.random() < 0.3 else int(rng.integers(1, 9))
        slots = int(rng.integers(33, 81)) if big else int(rng.integers(1, 12))
        slot_tri = rng.permutation(slots)
        dens = rng.choice([0.03, 0.1, 0.25]) if big else rng.choice([0.05, 0.3, 0.9])
        vals = [None] + [np.float32(v) for v in rng.choice([0.5, 1.0, 2.0, 3.0], size=3)]
        pairs = [{int(s): vals[int(rng.integers(0, 4))] for s in np.flatnonzero(rng.random(slots) < dens)}
                 for _ in range(rays)]
        cnt = _same(pairs, slot_tri)
        for k in ("spread", "big", "small"):
            seen[k] += cnt[k]
        for pr in pairs:  # a ray's nearest distance twice, the lower index in the later slot
            d = [(v, s) for s, v in pr.items() if v is not None]
            if d:
                near = sorted(s for v, s in d if v == min(d)[0])
                seen["ties"] += any(slot_tri[b] < slot_tri[a] for a in near for b in near if b > a)
    assert all(seen.values()) and seen["ties"] > 1000, seen


def test_dropping_an_entry_is_seen():
    """The negative control's premise: with the last list entry untested, the ray whose nearest pair it is keeps its
    second nearest."""
    sc = E.stack_scene(3, 20, [3, 41])
    st = np.arange(5)
    pairs = E.pairs_of(sc, st)
    good, _ = E.episode(pairs, st)
    bad, _ = E.episode(pairs, st, drop=True)
    assert good == E.scan(pairs, st) and good[20][1] == 2 and bad[20][1] == 1
    assert [k for k in range(64) if good[k] != bad[k]] == [20]


# ---- what the GPU scenes give, from their descriptions ------------------------------

@pytest.mark.parametrize("n,want", [(1, (0, 0, 0, 0)), (2, (1, 0, 0, 1)), (3, (2, 1, 0, 0)), (33, (31, 1, 0, 0)),
                                    (40, (38, 2, 0, 0))])
def test_stack_counters(n, want):
    """(leftovers, spread rounds, Rw > 64 rounds, small rounds) of a stack of n with singles around it.  33 and 40
    cross a round of 32 hot triangles: 31 leftovers in the first; the second round's first pair is the 33rd, which
    leaves none and 7."""
    sc = E.stack_scene(n, 5, [0, 9, 33, 63])
    _, cnt = E.episode(E.pairs_of(sc, np.arange(n + 4)), np.arange(n + 4))
    assert (cnt["leftovers"], cnt["spread"], cnt["big"], cnt["small"]) == want


@pytest.mark.parametrize("left", sorted(E.FEW_LEFTOVERS))
def test_few_leftovers_counters(left):
    sc = E.stacks_scene(E.FEW_LEFTOVERS[left])
    st = np.arange(len(sc["cover"]))
    pairs = E.pairs_of(sc, st)
    got, cnt = E.episode(pairs, st)
    assert got == E.scan(pairs, st) and len(E.rounds_of(pairs)) == 1
    assert (cnt["leftovers"], cnt["spread"], cnt["big"], cnt["small"]) == (left, int(left == 3), 0, int(0 < left < 3))


@pytest.mark.parametrize("extra,rw", [(0, 62), (1, 63), (2, 64), (3, 65)])
def test_leftover_counters(extra, rw):
    sc = E.leftover_scene(extra)
    st = np.arange(len(sc["cover"]))
    pairs = E.pairs_of(sc, st)
    got, cnt = E.episode(pairs, st)
    assert got == E.scan(pairs, st)
    assert (cnt["leftovers"], cnt["spread"], cnt["big"]) == (rw, int(rw <= 64), int(rw > 64))
    assert len(E.rounds_of(pairs)) == 2


@pytest.mark.parametrize("kind,winner", [("first_loses", 0), ("first_wins", 0), ("workers", 1)])
def test_tie_scenes(kind, winner):
    """The duplicates' lower index wins in every arrangement; a scan with the strict rule alone would keep the
    earlier slot's."""
    sc, st = E.tie_scene(kind)
    pairs = E.pairs_of(sc, st)
    got, cnt = E.episode(pairs, st)
    assert got == E.scan(pairs, st) and cnt["spread"] == 1
    assert got[7][1] == winner and got[50][1] == 3 + winner
    if kind != "first_wins":  # the lower index sits in the later slot
        assert list(st).index(winner) > list(st).index(winner + (2 if kind == "first_loses" else 1))
