"""Models and scenes for MfmaSpec::cluster_rows16 (rt2_k5_resident.h
cluster_rows_frag16, rt2_mfma.h kt_group16; DESIGN.md "16-row products"):
tests/test_cluster16_model.py on the CPU, tests/test_gpu_cluster16.py on the
GPU.  Only numpy and the rt2 package's host half; the comb scenes' view,
triangles and boxes are tests/cluster_scenes.py's.

The comb scenes of cluster_scenes.comb_scene put the evidence of owned column
number q at in-group slot q // groups: with at most 8 owned columns (16 needing
rays at comb pitch 2) every evidence triangle sits in slots 0..7, the lower
triangle half of kt_group16, and a wrong upper half could not show.  The
builder here gives owned column q the in-group slot SLOTS16[q], in group
q % groups: slots 0, 31, 15, 16 first, then others of both halves."""
import numpy as np

import rt2
import cluster_scenes as cs
from closest_hit_scenes import _triangles, code_materials

SLOTS16 = (0, 31, 15, 16, 8, 23, 7, 24, 12)  # in-group slot of owned column number q (both triangle halves)

# (x0, x1, groups) per compact cluster in index order, ("wall", groups) the full one; the needing sets (c0, c1) of the
# rows: (1, 0), (0, 1), (16, 0), (0, 16), -, (8, 8), (15, 1), (1, 15), (17, 0), (0, 17), (9, 8), (16, 1), (16, 0).
# A compact cluster first and last, clusters of 1, 2 and 3 groups, a ragged last group (RAGGED16 of its 32 slots).
CASES16 = ((9, 10, 2), (40, 41, 1), (0, 16, 3), (32, 48, 1), ("wall", 1), (24, 40, 2), (17, 33, 3), (31, 47, 1),
           (0, 17, 2), (47, 64, 3), (23, 40, 1), (16, 33, 2), (16, 32, 2))
RAGGED16 = 20
REQUIRED16 = ((1, 0), (0, 1), (16, 0), (0, 16), (8, 8), (15, 1), (1, 15), (17, 0), (0, 17), (9, 8), (16, 1))

# The negative controls: (band, the interval its box is shrunk to, victim column); the victim owns a triangle of the
# cluster and its ray no longer needs the box.
CONTROLS16 = ((2, (1, 16), 0),      # (16, 0) -> (15, 0): row 15 is block 1's first other lane, 32
              (4, (25, 40), 24),    # (8, 8) -> (7, 8): row 15 is lane 40
              (10, (17, 33), 16),   # across the threshold, (16, 1) in the 32-row form -> (15, 1) in the 16-row form
              (4, (24, 38), 38),    # (8, 8) -> (8, 6): rows 14, 15 are lanes 38, 39: the victim rides as a filler
              (3, (33, 48), 32))    # (0, 16) -> (0, 15): row 15 is lane 32, the victim


def record_lane16(l):
    """kt16_record_lane (rt2_mfma.h): the record lane that lane l of a 16-row product reads."""
    return (l & 15) + 16 * (l >> 5) + 32 * ((l >> 4) & 1)


def row_model16(need):
    """cluster_rows_frag16 for a 64-bit need mask of at most 16 bits, restated
    lane by lane.  A fragment register a0[R] holds in lane l the k-slots of
    half l >> 5 of ray 32 R + (l & 31).  -> (dst0, dst1, alo, ahi): the 64
    ds_permute destinations of block 0's and block 1's register, and per lane
    of alo / ahi the (ray, half) it holds, None for a zero, -1 where no lane
    or more than one lane sent there."""
    need = int(need)
    bit = [(need >> l) & 1 for l in range(64)]
    c0, c1 = sum(bit[:32]), sum(bit[32:])
    assert c0 + c1 <= 16
    dst = []
    for l in range(64):  # per ray: its row, then the row's first lane (row + (row & 16))
        rk = sum(bit[:l])
        rest = ((l - rk) + (c0 if l < 32 else c1 + 2 * c0)) & 31
        row = rk if bit[l] else rest
        dst.append(row + (row & 16))
    # v_permlane32_swap(dst, dst): sw[0] = ray (l & 31)'s, sw[1] = ray 32 + (l & 31)'s; + 16 for the second K-half
    dst0 = [dst[l & 31] + 16 * (l >> 5) for l in range(64)]
    dst1 = [dst[32 + (l & 31)] + 16 * (l >> 5) for l in range(64)]

    def received(dsts, block):
        got = [[] for _ in range(64)]
        for l, t in enumerate(dsts):
            got[t].append((32 * block + (l & 31), l >> 5))
        return [g[0] if len(g) == 1 else -1 for g in got]

    x0, x1 = received(dst0, 0), received(dst1, 1)
    alo = [(x0[l] if (l & 15) < c0 else x1[l]) if l < 32 else None for l in range(64)]
    ahi = [None if l < 32 else alo[l - 32] for l in range(64)]
    return dst0, dst1, alo, ahi


def swept_lanes16(need):
    """The lanes whose rays a compact cluster's sweep holds under cluster_rows16, in a wave of 64 live rays."""
    c = bin(int(need)).count("1")
    if c == 0 or c > 16:
        return cs.swept_lanes(need)
    return {ray for ray, _ in row_model16(need)[2][:32]}


_cache = {}


def comb16_scene():
    """The comb scene of CASES16 in cluster_scenes.comb_scene's geometry and
    keys (triangles, materials, ranges, H, bands, column, band_of, wall_tri,
    table(shrink)), with the evidence slots of SLOTS16.  An evidence slot past
    the ragged last group's end moves to the cluster's group before."""
    if "s" in _cache:
        return _cache["s"]
    cases = CASES16
    H = cs.comb_height(sum(c[0] != "wall" for c in cases))
    dx, dy = cs._comb_dirs(H)
    va, vb, vc, column, band_of = [], [], [], [], []
    ranges, bands, g = [], [], 0
    for k, case in enumerate(cases):
        if case[0] == "wall":
            assert case[1] == 1
            for i in range(32):  # every triangle covers the view; triangle 0 of the group is the nearest
                z = -(cs.WALL_Z + 0.005 * i)
                va.append((-40.0, -30.0, z)), vb.append((40.0, -30.0, z)), vc.append((0.0, 50.0, z))
                column.append(-1), band_of.append(-1)
            wall_tri = 32 * g
            ranges.append((g, g + 1, False))
            g += 1
            continue
        x0, x1, groups = case
        band = len(bands)
        owned = np.arange(x0, x1, cs.COMB_PITCH)
        last = RAGGED16 if k == len(cases) - 1 else 32
        slots = 32 * (groups - 1) + last
        assert len(owned) <= len(SLOTS16)
        slot_of, evidence = [None] * slots, []
        for q in range(len(owned)):
            grp = q % groups
            if 32 * grp + SLOTS16[q] >= slots:
                grp -= 1
            s = 32 * grp + SLOTS16[q]
            assert grp >= 0 and slot_of[s] is None
            slot_of[s] = (0, q)
            evidence.append(32 * g + s)
        layer, q = 1, 0
        for s in range(slots):
            if slot_of[s] is None:
                slot_of[s] = (layer, q)
                q += 1
                if q == len(owned):
                    layer, q = layer + 1, 0
        for lay, q in slot_of:
            t = cs.COMB_Z * (1.0 + cs.COMB_LAYER * lay)
            w = cs.COMB_HALF * t / cs.COMB_Z
            p = np.array([t * dx[owned[q]], t * dy[band], -t])
            va.append(p + (-w, -w, 0)), vb.append(p + (w, -w, 0)), vc.append(p + (0, w, 0))
            column.append(int(owned[q])), band_of.append(band)
        bands.append(dict(k=k, row=band, x0=x0, x1=x1, groups=groups, owned=owned, evidence=np.array(evidence)))
        ranges.append((g, g + groups, True))
        g += groups
    a, b, c = cs._wind(*(np.array(v, np.float64).astype(np.float32) for v in (va, vb, vc)))
    tris = _triangles(a, b, c)
    assert len(tris) == 32 * (g - 1) + RAGGED16 and len(ranges) <= rt2.MAX_CLUSTERS
    mats = code_materials(len(tris))
    base = cs.explicit_table(tris, ranges, pad=cs.COMB_PAD)

    def table(shrink=None):
        t = base.copy()
        for band, bd in enumerate(bands):
            lo_c, hi_c = (shrink or {}).get(band, (bd["x0"], bd["x1"]))
            k = bd["k"]
            zn, zf = -float(t["c"][k]["hi"][2]), -float(t["c"][k]["lo"][2])
            t["c"][k]["lo"][0], t["c"][k]["hi"][0] = cs._box_x(dx, lo_c, hi_c, zn, zf)
        return t

    tris.setflags(write=False)
    mats.setflags(write=False)
    _cache["s"] = dict(triangles=tris, materials=mats, ranges=ranges, H=H, bands=bands, table=table,
                       pitch=cs.COMB_PITCH, column=np.array(column), band_of=np.array(band_of), wall_tri=wall_tri)
    return _cache["s"]
