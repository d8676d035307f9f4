"""Scenes and a model for MfmaSpec::exact_spread (rt2_k5_resident.h
exact_window_lanes: a round's leftover exact pairs dealt out over all 64
lanes), host half of tests/test_gpu_exact_spread.py and
tests/test_exact_spread_model.py.

The model follows the kernel's bookkeeping, not its arithmetic: a (ray,
triangle) pair is a slot and the distance the exact test gives (None: the test
rejects it).  `scan` is the sequential scan in slot order with mt_exact_slot's
rule; `episode` is the kernel's: rounds of 32 hot slots, every lane's first
pair on its own lane, an exclusive prefix sum of the leftover counts, the
scatter into the list, one worker per entry against the source's bound after
its first pair, and the merge by the minimum of (distance bits, index, slot).

The scenes are one wave each: 64 x 1 images without jitter (exact_lanes_scenes.
still_uniforms), pixel p's ray alone through the triangles built on p, so the
pairs of every ray are known from the scene's description.  Triangle i has
index i and colour code i; `slot_tri` is installed through
rt2_scene_set_slot_order, the identity unless a scene says otherwise."""
import struct

import numpy as np

import closest_hit_scenes as S
import exact_lanes_scenes as X

START = 1e38  # the sweep's starting bound


def f32_bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def _accept(dst, slot, best, bi, slot_tri):
    """mt_exact_slot's rule on (best, bi): -> whether the pair is taken."""
    if dst is None or not dst <= best:
        return False
    if dst == best and (bi < 0 or slot_tri[slot] > slot_tri[bi]):
        return False
    return True


def scan(pairs, slot_tri):
    """pairs[ray] = {slot: dst or None}.  The sequential scan, slots ascending.  -> [(best, index or -1)]."""
    out = []
    for pr in pairs:
        best, bi = np.float32(START), -1
        for slot in sorted(pr):
            if _accept(pr[slot], slot, best, bi, slot_tri):
                best, bi = pr[slot], slot
        out.append((best, slot_tri[bi] if bi >= 0 else -1))
    return out


def rounds_of(pairs):
    """The episode's rounds: the wave's hot slots ascending, 32 per round."""
    hot = sorted({s for pr in pairs for s in pr})
    return [hot[k:k + 32] for k in range(0, len(hot), 32)]


def episode(pairs, slot_tri, drop=False):
    """The kernel's episode on one wave (len(pairs) <= 64 lanes).  -> ([(best, index or -1)] per ray, counters
    dict: leftovers (Rw summed), spread (rounds on the spread path), big (rounds that fell back on Rw > 64), small
    (rounds with leftovers but no lane holding two), trips (per-lane test trips the wave ran)).  drop: a spread
    round's last list entry is not tested (the negative control's arm)."""
    n = len(pairs)
    assert n <= 64
    best = [np.float32(START)] * n
    bi = [-1] * n
    cnt = dict(leftovers=0, spread=0, big=0, small=0, trips=0)
    for hot in rounds_of(pairs):
        bit_of = {s: b for b, s in enumerate(hot)}
        pm = [sorted(bit_of[s] for s in pr if s in bit_of) for pr in pairs]  # each lane's bits, ascending
        cnt["trips"] += 1
        for lane in range(n):  # the first pair on its own lane
            if pm[lane]:
                s = hot[pm[lane].pop(0)]
                if _accept(pairs[lane][s], s, best[lane], bi[lane], slot_tri):
                    best[lane], bi[lane] = pairs[lane][s], s
        r = [len(x) for x in pm]
        at = [sum(r[:lane]) for lane in range(n)]  # the exclusive prefix sum
        rw = sum(r)
        if not rw:
            continue
        cnt["leftovers"] += rw
        if rw <= 64 and max(r) >= 2:
            cnt["spread"] += 1
            lst = [None] * 64
            for lane in range(n):  # scatter
                for j, b in enumerate(pm[lane]):
                    assert lst[at[lane] + j] is None
                    lst[at[lane] + j] = (lane, b)
            assert all(e is not None for e in lst[:rw]) and all(e is None for e in lst[rw:])
            slot_key = [None] * n  # the merge slots, empty
            for w in range(rw - (1 if drop else 0)):  # worker w: entry w on a copy of the source's state
                lane, b = lst[w]
                s = hot[b]
                dst = pairs[lane][s]
                if _accept(dst, s, best[lane], bi[lane], slot_tri):
                    assert dst > 0  # positive distances order like their bits
                    key = (f32_bits(dst), slot_tri[s], s)
                    slot_key[lane] = key if slot_key[lane] is None else min(slot_key[lane], key)
            for lane in range(n):  # every published key is below the lane's own
                if slot_key[lane] is not None:
                    s = slot_key[lane][2]
                    best[lane], bi[lane] = pairs[lane][s], s
        else:
            cnt["big" if rw > 64 else "small"] += 1
            cnt["trips"] += max(r)
            for lane in range(n):
                for b in pm[lane]:
                    s = hot[b]
                    if _accept(pairs[lane][s], s, best[lane], bi[lane], slot_tri):
                        best[lane], bi[lane] = pairs[lane][s], s
    return [(best[k], slot_tri[bi[k]] if bi[k] >= 0 else -1) for k in range(n)], cnt


# ---- scenes ----------------------------------------------------------------------

W = 64


def _span_triangle(u, width, px0, px1, depth):
    """A triangle that covers the rays of pixels px0 .. px1 of a one-row image and no other's: its base 0.4 pixels
    outside both, the apex 1,000 rows up (the sides move by less than 0.001 pixels at the row)."""
    lo, hi, mid = px0 - 0.4, px1 + 0.4, 0.5 * (px0 + px1)
    pts = [(lo, -0.4), (hi, -0.4), (mid, 1000.0)]
    return [X._point(u, *X._norm(width, 1, x, y), depth) for x, y in pts]


def build(spec, width=W):
    """spec: a list of (px0, px1, depth) in index order.  -> dict: triangles, materials, uniforms (width x 1),
    cover [triangle] = (px0, px1)."""
    n = len(spec)
    u = X.still_uniforms(width, 1, n)
    tris = [_span_triangle(u, width, a, b, depth) for a, b, depth in spec]
    return dict(triangles=X._pack(u, tris), materials=S.code_materials(n), uniforms=u,
                cover=[(a, b) for a, b, _ in spec], depth=[d for _, _, d in spec], width=width)


def pairs_of(sc, slot_tri):
    """The wave's pairs from the scene's description: ray p has slot s iff s's triangle covers p; the distance
    stands for the exact test's (the depth: the order and the ties are the scene's)."""
    inv = np.empty(len(slot_tri), np.int64)
    inv[np.asarray(slot_tri)] = np.arange(len(slot_tri))
    pairs = [dict() for _ in range(sc["width"])]
    for i, (a, b) in enumerate(sc["cover"]):
        for p in range(a, b + 1):
            pairs[p][int(inv[i])] = np.float32(sc["depth"][i])
    return pairs


def stack_scene(n, px, others, near_last=True, width=W):
    """n triangles stacked on pixel px (index order = far to near when near_last, else near to far), then one
    triangle on each pixel of `others`."""
    depth = [2.0 - i / (n + 1) if near_last else 1.0 + i / (n + 1) for i in range(n)]
    return build([(px, px, d) for d in depth] + [(p, p, 1.5) for p in others], width)


def leftover_scene(extra):
    """32 triangles over pixels 10 and 11 (31 leftovers each); the first `extra` + 1 of them reach pixel 12 too
    (`extra` leftovers there): one round with 62 + extra leftovers.  Then one triangle each on pixels 40 .. 44: a
    second round without leftovers."""
    spec = [(10, 12 if i <= extra else 11, 2.0 - i / 40) for i in range(32)]
    return build(spec + [(p, p, 1.5) for p in range(40, 45)])


def stacks_scene(counts):
    """Several stacked rays: counts = {pixel: triangles on it}, the stacks one after another in index order, each
    far to near.  The round's leftovers are the sum of (count - 1)."""
    spec = []
    for px, n in counts.items():
        spec += [(px, px, 2.0 - i / (n + 1)) for i in range(n)]
    return build(spec)


# several stacked rays with 0, 1, 2 and 3 leftovers in all: only the last holds two on one lane and spreads
FEW_LEFTOVERS = {0: {3: 1, 20: 1, 21: 1, 45: 1}, 1: {3: 1, 20: 2, 21: 1, 45: 1}, 2: {3: 2, 20: 1, 21: 1, 45: 2},
                 3: {3: 2, 20: 1, 21: 3, 45: 1}}


def tie_scene(kind):
    """Three triangles on pixel 7 and three on pixel 50, two of each three the same triangle, in slot order
    [s0, s1, s2] with the indices exchanged so that the duplicate's lower index sits in the later slot:
      first_loses: s0 and s2 are the duplicates, s0 holds the higher index: the leftover wins the tie;
      first_wins:  s0 and s2 the duplicates, s0 the lower index: the first pair keeps it;
      workers:     s1 and s2 the duplicates, s1 the higher index: two leftovers tie, the later slot wins.
    The third triangle lies behind.  -> (scene, slot_tri)."""
    spec, slot_tri = [], []
    for px in (7, 50):
        base = len(spec)
        if kind == "workers":
            spec += [(px, px, 1.5), (px, px, 1.25), (px, px, 1.25)]  # indices base: far, base + 1 = base + 2
            slot_tri += [base, base + 2, base + 1]
        else:
            spec += [(px, px, 1.25), (px, px, 1.5), (px, px, 1.25)]  # base = base + 2 the duplicates
            slot_tri += [base + 2, base + 1, base] if kind == "first_loses" else [base, base + 1, base + 2]
    return build(spec), np.array(slot_tri, np.int32)
