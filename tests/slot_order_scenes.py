"""Scenes, orders and tables for the slot-order tests (tests/test_slot_order.py
on the CPU, tests/test_gpu_slot_order.py on the GPU; DESIGN.md "Slot order").

A slot order is a permutation slot_tri of the triangle indices: slot s holds
triangle slot_tri[s], slot group g the slots 32 g .. 32 g + 31.  The resident
kernel then visits a ray's surviving triangles in ascending slot, and the tie
rule (the lower index on equal distances) must leave what the ascending index
scan leaves.  The tie scene is the `one` comb scene of tests/cluster_scenes.py
with a ragged last group and six duplicated triangles; its order exchanges the
slots of each duplicate pair, so the pair's lower index sits in the later slot.
"""
import numpy as np

import cluster_scenes as cs
import rt2
from closest_hit_scenes import with_ties

RAGGED = 7
_cache = {}


def orders(n, seed=7):
    """name -> slot_tri of the fixed orders."""
    return {"identity": np.arange(n, dtype=np.int32), "reversed": np.arange(n, dtype=np.int32)[::-1].copy(),
            "random": np.random.default_rng(seed).permutation(n).astype(np.int32)}


def chunk_table(tris, slot_tri, full=(1,)):
    """A table over the slot groups of tris[slot_tri]: the groups cut into at most MAX_CLUSTERS contiguous ranges of
    nearly equal length, the vertices' boxes padded like the library's, every range compact but those in `full`."""
    perm = np.ascontiguousarray(tris[slot_tri])
    ng = (len(perm) + 31) // 32
    edges = np.unique(np.linspace(0, ng, min(ng, rt2.MAX_CLUSTERS) + 1).round().astype(int))
    ranges = [(int(a), int(b), k not in full or len(edges) == 2) for k, (a, b) in enumerate(zip(edges[:-1], edges[1:]))]
    return cs.explicit_table(perm, ranges)


def reversed_table(t, n_tris):
    """The table `t` over the index groups of a scene of whole groups, for the reversed order: the same clusters
    with the same boxes, last first."""
    assert n_tris % 32 == 0
    ng, n = n_tris // 32, int(t["n"])
    r = t.copy()
    for k in range(n):
        c = t["c"][n - 1 - k]
        g0, g1, fl = int(c["g0"]), int(c["g1_flags"]) & 0xffff, int(c["g1_flags"]) & ~0xffff
        r["c"][k] = c
        r["c"][k]["g0"], r["c"][k]["g1_flags"] = ng - g1, (ng - g0) | fl
    return r


def tie_scene():
    """The `one` comb scene with its last group cut to RAGGED triangles and the duplicate pairs below.  -> dict:
    triangles, materials, H, pairs [(name, i, j, row, column)] with i < j the duplicates (the pixel (row, column)
    sees both at one distance, and index i is the reference's hit), slot_tri (the slots of every pair exchanged)
    and table (the scene's ranges over the slot groups, boxes of the permuted vertices)."""
    if "tie" in _cache:
        return _cache["tie"]
    sc = cs.comb_scene(cs.COMB_CASES_ONE, last=RAGGED)
    n = len(sc["triangles"])
    assert n % 32 == RAGGED
    bands, ranges = sc["bands"], sc["ranges"]
    first = lambda band: 32 * ranges[bands[band]["k"]][0]  # the first triangle of a band's cluster
    ev = lambda band, q: int(bands[band]["evidence"][q])
    col = lambda band, q: int(bands[band]["owned"][q])
    wall = 5
    assert sc["wall_tri"] != wall and sc["band_of"][wall] < 0
    last_group = 32 * ((n - 1) // 32)
    # (name, source evidence (band, q), the other triangle of the pair)
    spec = [("one group", (0, 2), first(0) + 20),
            ("two groups of one cluster", (1, 0), first(1) + 32 + 20),
            ("a compact and a full cluster", (3, 1), wall),
            ("two compact clusters", (4, 0), first(6) + 20),
            ("across a round of 32 hot triangles", (2, 0), first(2) + 64 + 25),
            ("winner in the ragged last group", (5, 0), last_group + RAGGED - 1)]
    fams, pairs = [], []
    slot_tri = np.arange(n, dtype=np.int32)
    for name, (band, q), other in spec:
        e = ev(band, q)
        assert other != e
        if sc["band_of"][other] >= 0:  # the copy overwrites a filler of a comb, never evidence
            assert other not in bands[sc["band_of"][other]]["evidence"]
        fams.append([e, other])
        i, j = min(e, other), max(e, other)
        pairs.append((name, i, j, bands[band]["row"], col(band, q)))
        slot_tri[i], slot_tri[j] = j, i
    assert len({x for _, i, j, _, _ in pairs for x in (i, j)}) == 2 * len(pairs)
    assert pairs[-1][2] // 32 == (n - 1) // 32 and pairs[0][1] // 32 == pairs[0][2] // 32
    tris = with_ties(sc["triangles"], fams)
    table = cs.explicit_table(np.ascontiguousarray(tris[slot_tri]), ranges, pad=cs.COMB_PAD)
    tris.setflags(write=False)
    _cache["tie"] = dict(triangles=tris, materials=sc["materials"], H=sc["H"], pairs=pairs, slot_tri=slot_tri,
                         table=table, ranges=ranges)
    return _cache["tie"]


def hit_distances(oracle, tris, o, d):
    """dst [rays, triangles] float32 of the reference's own test of every pair (inf: no hit): one single-triangle
    scan per triangle, so equal distances are equal bits exactly where the reference's are."""
    out = np.full((len(o), len(tris)), np.inf, np.float32)
    for k in range(len(tris)):
        dst, idx, _, _ = oracle.closest_hits(tris[k:k + 1], o, d)
        out[idx == 0, k] = dst[idx == 0]
    return out


def slot_scan(dst, slot_tri, tie_rule=True):
    """The episode's scan restated: slots ascending, accept on dst < best, or (the tie rule) on dst == best and a
    lower index than the holder's.  -> the winner's index per ray, -1 for a miss.  tie_rule=False is the mutant
    with the strict rule only."""
    n_rays = dst.shape[0]
    best = np.full(n_rays, np.float32(1e38))
    bi = np.full(n_rays, -1, np.int64)  # a slot
    st = np.asarray(slot_tri, np.int64)
    for s in range(len(st)):
        t = dst[:, st[s]]
        take = t < best
        if tie_rule:
            take |= (t == best) & (bi >= 0) & (st[s] < st[np.maximum(bi, 0)])
        best = np.where(take, t, best)
        bi = np.where(take, s, bi)
    return np.where(bi >= 0, st[np.maximum(bi, 0)], -1)
