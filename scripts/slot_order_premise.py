"""The premise of DESIGN.md "Slot order" on the hardware (experiment build,
RT2_LIB=exp): the cluster counters of the diagnostic variants on a config at
full size, per compact cluster, and the group loop's vector instructions per
sweep they project with the listing's prices, for the index image (411, the
table of rt2_cluster_table_build) and the slot image (416, the order and table
of rt2_cluster_order_build).  A cluster's counters are taken with a table in
which it alone is compact: the need test of a cluster reads only its own box
and the wave's live rays.  Also the wall time of rt2_scene_create."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raytracing2-fork_amd"))
import torch  # noqa: E402,F401
import rt2  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="B")
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
a = ap.parse_args()
sd, spec = rt2.build_config_scene(a.config)
u = rt2.offline_uniforms(a.width, a.height, spec.bounces, spec.rays, sd.num_triangles)

t0 = time.perf_counter()
scene = rt2.Scene(sd, 0)
first_ms = (time.perf_counter() - t0) * 1e3
create_ms = []
for _ in range(5):
    t0 = time.perf_counter()
    s2 = rt2.Scene(sd, 0)
    create_ms.append(round((time.perf_counter() - t0) * 1e3, 3))
    del s2

PER_SWEEP, COMPACT, FULL, GROUP = 38.0, 31.0, 8.0, 51.5


def price32(n):
    return 28.0 + 53.0 * (n // 2) + 27.0 * (n % 2)


def price16(n):  # the kernel takes the 16-row form whenever at most 16 rays need the cluster
    return 38.0 + 31.0 * (n // 2) + 16.0 * (n % 2)


def counters(variant):
    scene.set_variant(variant)
    scene.stats(reset=True)
    scene.render_host(u, 0, 1)
    scene.stats(reset=True)  # rt2_scene_stats copies the device's counters to where rt2_scene_diag_ex reads them
    c = (C.c_ulonglong * 32)()
    rt2.lib().rt2_scene_diag_ex(scene._p, c, 32)
    return dict(skipped=int(c[25]), one_block=int(c[26]), two_blocks=int(c[27]), needing_rays=int(c[28]),
                rows16=int(c[29]))


def ranges_of(t):
    return [(int(c["g0"]), int(c["g1_flags"]) & 0xffff, bool(int(c["g1_flags"]) & rt2.CLUSTER_COMPACT))
            for c in t["c"][:int(t["n"])]]


def project(table, variant, install):
    """Per compact cluster of `table` its counters (alone compact), and the projected loop."""
    out = {"table": ranges_of(table), "clusters": []}
    loop = PER_SWEEP
    for k, (g0, g1, compact) in enumerate(ranges_of(table)):
        n = g1 - g0
        if not compact:
            loop += FULL + GROUP * n
            continue
        t = table.copy()
        for j in range(int(t["n"])):
            if j != k:
                t["c"][j]["g1_flags"] = int(t["c"][j]["g1_flags"]) & 0xffff
        install(t)
        c = counters(variant)
        cases = c["skipped"] + c["one_block"] + c["two_blocks"]
        f16, f32, f64 = c["rows16"] / cases, (c["one_block"] - c["rows16"]) / cases, c["two_blocks"] / cases
        cost = COMPACT + f16 * price16(n) + f32 * price32(n) + f64 * GROUP * n
        loop += cost
        out["clusters"].append(dict(groups=[g0, g1], counts=c, skipped=round(c["skipped"] / cases, 4),
                                    rows16=round(f16, 4), rows_17_to_32=round(f32, 4), two_blocks=round(f64, 4),
                                    needing_rays_per_case=round(c["needing_rays"] / cases, 2),
                                    valu_per_sweep=round(cost, 1)))
    install(table)
    out["whole_table_counts"] = counters(variant)
    out["projected_loop_valu_per_sweep"] = round(loop, 1)
    return out


res = {"config": a.config, "width": a.width, "height": a.height, "triangles": sd.num_triangles,
       "scene_create_ms": {"first": round(first_ms, 3), "next_5": create_ms, "median": float(np.median(create_ms))},
       "prices": {"per_sweep": PER_SWEEP, "compact_cluster": COMPACT, "full_cluster": FULL, "group_two_block": GROUP,
                  "rows32": "28 + 53 (n / 2) + 27 (n % 2)", "rows16": "38 + 31 (n / 2) + 16 (n % 2)"}}
index_table = scene.cluster_table().copy()
res["index_image_411"] = project(index_table, 411, scene.set_cluster_table)
# set_cluster_table reset the slot image: install the rule's order again
slot_tri, slot_table = rt2.cluster_order(sd.triangles())
res["slot_image_416"] = project(slot_table, 416, lambda t: scene.set_slot_order(slot_tri, t))
res["regrouped"] = not np.array_equal(slot_tri, np.arange(len(slot_tri)))
p, q = res["index_image_411"]["projected_loop_valu_per_sweep"], res["slot_image_416"]["projected_loop_valu_per_sweep"]
res["ratio"] = round(q / p, 4)
print(json.dumps(res, indent=1))
