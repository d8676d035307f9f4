"""Models and scenes for MfmaSpec::cluster_rows8 (rt2_k5_resident.h
cluster_rows_frag8, rt2_mfma.h kt_group8; DESIGN.md "8-row products"):
tests/test_cluster8_model.py on the CPU, tests/test_gpu_cluster8.py on the GPU.
Only numpy and the rt2 package's host half; the comb scenes' view, triangles
and boxes are tests/cluster_scenes.py's, the 16-row ranking is
tests/cluster16_scenes.py's.

The comb scene here has needing sets on both sides of the 8-ray threshold,
clusters of 1, 2, 3 and 5 groups (the loop takes two groups per trip) and its
evidence in both triangle halves of a group: owned column q of a cluster sits
in in-group slot SLOTS8[q] of group (q + groups - 1) % groups, so that the
cluster's last group, the odd one of the loop's remainder, carries evidence."""
import numpy as np

import rt2
import cluster_scenes as cs
import cluster16_scenes as c16
from closest_hit_scenes import _triangles, code_materials

SLOTS8 = c16.SLOTS16  # 0, 31, 15, 16, 8, ...: both triangle halves from the second owned column on

# (x0, x1, groups) per compact cluster in index order, ("wall", groups) the full one; the needing sets
# (c0, c1) of the rows: (1, 0), (0, 1), (8, 0), (0, 8), -, (4, 4), (7, 1), (1, 7), and across the threshold (9, 0),
# (0, 9), (5, 4), (8, 1).  A compact cluster first and last, clusters of 1, 2, 3 and 5 groups, a ragged last group
# (RAGGED8 of its 32 slots) with evidence at in-group slots 0 and 16, in both its halves.
CASES8 = ((9, 10, 2), (40, 41, 1), (0, 8, 3), (32, 40, 1), ("wall", 1), (28, 36, 5), (25, 33, 2), (31, 39, 3),
          (0, 9, 2), (47, 56, 1), (27, 36, 2), (24, 33, 3))
RAGGED8 = 20
REQUIRED8 = ((1, 0), (0, 1), (8, 0), (0, 8), (4, 4), (7, 1), (1, 7), (9, 0), (0, 9), (5, 4), (8, 1))

# The negative controls: (band, the interval its box is shrunk to, victim column, rides); the victim owns a triangle
# of the cluster and its ray no longer needs the box.  `rides` is the prediction, checked against the row model in
# tests/test_cluster8_model.py.
CONTROLS8 = ((2, (1, 8), 0, False),      # (8, 0) -> (7, 0): row 7 is block 1's first other lane, 32
             (4, (29, 36), 28, False),   # (4, 4) -> (3, 4): row 7 is lane 36
             (10, (25, 33), 24, False),  # across the threshold: (8, 1) in the 16-row form -> (7, 1) in the 8-row form
             (3, (33, 40), 32, True),    # (0, 8) -> (0, 7): row 7 is lane 32, the victim: it rides as a filler
             (3, (34, 40), 32, True))    # (0, 8) -> (0, 6): rows 6, 7 are lanes 32, 33: the victim rides as row 6


def row_model8(need):
    """cluster_rows_frag8 for a 64-bit need mask of at most 8 bits, restated
    lane by lane on cluster16_scenes.row_model16's permutes.  q, the 16-row
    routine's selected register, holds in lane l < 32 what alo holds there.
    a8[l] = q[l] for l < 32 with (l & 15) < 8; for l >= 32 with (l & 15) >= 8
    it is q[l - 40], which v_permlane32_swap into zero (lane l takes q[l - 32])
    and a row shift right by 8 (lane l takes lane l - 8 of its row of 16, zero
    from outside the row) deliver; zero elsewhere.  -> (dst0, dst1, a8): the
    permutes' destinations and per lane of a8 the (ray, half) it holds, None
    for a zero."""
    assert bin(int(need)).count("1") <= 8
    dst0, dst1, alo, _ = c16.row_model16(need)
    q = alo[:32]
    up = [None] * 32 + q                                                    # v_permlane32_swap(0, q)[0]
    sh = [up[l - 8] if (l & 15) >= 8 else None for l in range(64)]          # row_shr:8, bound_ctrl
    a8 = [q[l] if (l & 0x28) == 0 else sh[l] for l in range(64)]
    return dst0, dst1, a8


def hot_mask8(M):
    """kt8_hot (rt2_mfma.h): a group's hot mask from the one ballot of the
    8-row fold.  Lane l of D holds column l & 15 and rows 4 (l >> 4) .. + 3."""
    M = int(M)
    return ((M | M >> 16) & 0xffff) | ((((M >> 32) | (M >> 48)) & 0xffff) << 16)


def swept_lanes8(need):
    """The lanes whose rays a compact cluster's sweep holds under cluster_rows8 (with cluster_rows16), in a wave of
    64 live rays."""
    c = bin(int(need)).count("1")
    if c == 0 or c > 8:
        return c16.swept_lanes16(need)
    return {x[0] for x in row_model8(need)[2] if x is not None}


_cache = {}


def comb8_scene():
    """The comb scene of CASES8 in cluster_scenes.comb_scene's geometry and
    keys (triangles, materials, ranges, H, bands, column, band_of, wall_tri,
    table(shrink)), with the evidence slots of SLOTS8.  An
    evidence slot past the ragged last group's end moves to the cluster's
    group before."""
    if "s" in _cache:
        return _cache["s"]
    cases = CASES8
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
        want = SLOTS8
        band = len(bands)
        owned = np.arange(x0, x1, cs.COMB_PITCH)
        last = RAGGED8 if k == len(cases) - 1 else 32
        slots = 32 * (groups - 1) + last
        assert len(owned) <= len(want)
        slot_of, evidence = [None] * slots, []
        for q in range(len(owned)):
            grp = (q + groups - 1) % groups
            if 32 * grp + want[q] >= slots:
                grp -= 1
            s = 32 * grp + want[q]
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
    assert len(tris) == 32 * (g - 1) + RAGGED8 and len(ranges) <= rt2.MAX_CLUSTERS
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
