"""The premise of DESIGN.md "8-row products" on the hardware (experiment build,
RT2_LIB=exp): the cluster counters of the diagnostic variant 419 on a config
at full size, per compact cluster of the slot image, and the group loop's
vector instructions per sweep they project with the listing's prices, with the
8-row form for the cases of 1 to 8 needing rays and without it (the form
before).  A cluster's counters are taken with a table in which it alone is
compact, as scripts/slot_order_premise.py does."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raytracing2-fork_amd"))
import torch  # noqa: E402,F401
import rt2  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="B")
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--variant", type=int, default=419)
a = ap.parse_args()
sd, spec = rt2.build_config_scene(a.config)
u = rt2.offline_uniforms(a.width, a.height, spec.bounces, spec.rays, sd.num_triangles)
scene = rt2.Scene(sd, 0)

# vector instructions of the listing (scripts/slot_order_premise.py's, and the 8-row form's: a fragment of 45, a pair
# of groups 17, a single group 9)
PER_SWEEP, COMPACT, FULL, GROUP = 38.0, 31.0, 8.0, 51.5


def price32(n):
    return 28.0 + 53.0 * (n // 2) + 27.0 * (n % 2)


def price16(n):
    return 38.0 + 31.0 * (n // 2) + 16.0 * (n % 2)


def price8(n):
    return 45.0 + 17.0 * (n // 2) + 9.0 * (n % 2)


def counters():
    scene.set_variant(a.variant)
    scene.stats(reset=True)
    scene.render_host(u, 0, 1)
    scene.stats(reset=True)  # rt2_scene_stats copies the device's counters to where rt2_scene_diag_ex reads them
    c = (C.c_ulonglong * 32)()
    rt2.lib().rt2_scene_diag_ex(scene._p, c, 32)
    return dict(skipped=int(c[25]), one_block=int(c[26]), two_blocks=int(c[27]), needing_rays=int(c[28]),
                rows16=int(c[29]), rows8=int(c[31]))


def ranges_of(t):
    return [(int(c["g0"]), int(c["g1_flags"]) & 0xffff, bool(int(c["g1_flags"]) & rt2.CLUSTER_COMPACT))
            for c in t["c"][:int(t["n"])]]


slot_tri, table = rt2.cluster_order(sd.triangles())
out = {"config": a.config, "width": a.width, "height": a.height, "triangles": sd.num_triangles,
       "variant": a.variant, "table": ranges_of(table), "clusters": [],
       "prices": {"per_sweep": PER_SWEEP, "compact_cluster": COMPACT, "full_cluster": FULL, "group_two_block": GROUP,
                  "rows32": "28 + 53 (n / 2) + 27 (n % 2)", "rows16": "38 + 31 (n / 2) + 16 (n % 2)",
                  "rows8": "45 + 17 (n / 2) + 9 (n % 2)"}}
before = after = PER_SWEEP
for k, (g0, g1, compact) in enumerate(ranges_of(table)):
    n = g1 - g0
    if not compact:
        before += FULL + GROUP * n
        after += FULL + GROUP * n
        continue
    t = table.copy()
    for j in range(int(t["n"])):
        if j != k:
            t["c"][j]["g1_flags"] = int(t["c"][j]["g1_flags"]) & 0xffff
    scene.set_slot_order(slot_tri, t)
    c = counters()
    cases = c["skipped"] + c["one_block"] + c["two_blocks"]
    f8, f16 = c["rows8"] / cases, c["rows16"] / cases
    f32, f64 = (c["one_block"] - c["rows16"]) / cases, c["two_blocks"] / cases
    rest = COMPACT + f32 * price32(n) + f64 * GROUP * n
    cost16 = rest + f16 * price16(n)
    cost8 = rest + (f16 - f8) * price16(n) + f8 * min(price8(n), price16(n))
    before += cost16
    after += cost8
    out["clusters"].append(dict(groups=[g0, g1], counts=c, skipped=round(c["skipped"] / cases, 4),
                                rows_1_to_8=round(f8, 4), rows_9_to_16=round(f16 - f8, 4),
                                rows_17_to_32=round(f32, 4), two_blocks=round(f64, 4),
                                needing_rays_per_case=round(c["needing_rays"] / cases, 2),
                                valu_per_sweep_16_row=round(cost16, 1), valu_per_sweep_8_row=round(cost8, 1)))
scene.set_slot_order(slot_tri, table)
out["whole_table_counts"] = counters()
out["projected_loop_valu_per_sweep"] = {"rows16_form": round(before, 1), "rows8_form": round(after, 1),
                                        "ratio": round(after / before, 4)}
print(json.dumps(out, indent=1))
