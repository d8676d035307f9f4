"""A/B of the surface query against the closest-hit query on the config B
scene: rt2_surface_rays (RT2_TRACE_AUTO: surface_k5r) against rt2_trace_rays
(trace_rays_k5r) and against rt2_surface_rays with RT2_TRACE_SCALAR
(surface_scalar), each arm in a fresh process per round, the arms rotating.

The two sets of 2^22 rays are those of scripts/trace_rays_ab.py: "coherent"
(the default camera's primary rays of a 2048 x 2048 image, raster order) and
"random" (uniformly random directions from points inside the scene's bounding
box).  Round 0 checks that the three arms give identical (dst, tri) on both
sets, and the two surface arms identical records (a digest per set); rounds
1.. time one query per set and arm with HIP events (the median of --reps
launches after a warm-up), and a ladder of prefixes of the random set (64 ..
2^18 rays) for the two surface arms: whether RT2_TRACE_AUTO's matrix kernel
wins at every count is read from it.

A surface record is 48 B against the hit's 8 B: 40 B more written per ray
(168 MB for 2^22 rays), plus the epilogue's loads.  The yardstick is
rt2_trace_rays in the same job; the ratio is reported, no threshold is set.

Writes Mrays/s per arm and round to profiles/surface_ab.json.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raytracing2-fork_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from trace_rays_ab import LADDER, N_RAYS, ray_sets  # noqa: E402

ARMS = ("surface", "trace", "surface_scalar")
SETS = ("coherent", "random")


def child(a):
    import torch
    import rt2
    sd, spec = rt2.build_config_scene("B")
    u = rt2.offline_uniforms(spec.width, spec.height, spec.bounces, spec.rays, sd.num_triangles)
    scene = rt2.Scene(sd, 0)
    stream = torch.cuda.current_stream()
    out = {"arm": a.arm, "n_tris": sd.num_triangles}
    surface = a.arm != "trace"
    flags = rt2.TRACE_SCALAR if a.arm == "surface_scalar" else rt2.TRACE_AUTO
    rec = rt2.SURFACE_DTYPE if surface else rt2.HIT_DTYPE
    res_buf = torch.zeros(N_RAYS * rec.itemsize, dtype=torch.uint8, device="cuda")
    query = scene.surface_device if surface else scene.trace_rays_device

    def timed(rays, n, reps):
        query(rays.data_ptr(), n, res_buf.data_ptr(), flags, stream.cuda_stream)  # warm-up
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for e0, e1 in ev:
            e0.record(stream)
            query(rays.data_ptr(), n, res_buf.data_ptr(), flags, stream.cuda_stream)
            e1.record(stream)
        torch.cuda.synchronize()
        return float(np.median([e0.elapsed_time(e1) for e0, e1 in ev]))

    for name, rays in ray_sets(rt2, sd, u).items():
        d_rays = torch.from_numpy(rays.view(np.uint8)).cuda()
        ms = timed(d_rays, N_RAYS, a.reps)
        res = {"ms": round(ms, 3), "mrays_s": round(N_RAYS / ms / 1e3, 1), "kernel": scene.last_kernel()}
        if a.check:
            h = res_buf.cpu().numpy().view(rec)
            hits = np.zeros(N_RAYS, rt2.HIT_DTYPE)
            hits["dst"], hits["tri"] = h["dst"], h["tri"]
            res["hits_sha256"] = hashlib.sha256(hits.tobytes()).hexdigest()
            res["hit_fraction"] = round(float((h["tri"] >= 0).mean()), 4)
            if surface:
                res["records_sha256"] = hashlib.sha256(h.tobytes()).hexdigest()
                res["types_seen"] = sorted(set(h["mtl_type"][h["tri"] >= 0].tolist()))
        if name == "random" and not a.check and surface:
            res["ladder"] = {}
            for n in LADDER:
                ms = timed(d_rays, n, 4 * a.reps)
                res["ladder"][str(n)] = {"us": round(ms * 1e3, 2), "mrays_s": round(n / ms / 1e3, 2)}
        out[name] = res
    print(json.dumps(out))


def run_child(arm, reps, check=False):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--arm", arm, "--reps", str(reps)] + \
          (["--check"] if check else [])
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=300)
    if r.returncode != 0:
        raise SystemExit(f"{arm} child failed with status {r.returncode}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--arm", default="surface", choices=list(ARMS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface_ab.json"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    chk = {arm: run_child(arm, 1, check=True) for arm in ARMS}
    for name in SETS:
        if len({chk[arm][name]["hits_sha256"] for arm in ARMS}) != 1:
            raise SystemExit(f"the arms' (dst, tri) differ on the {name} rays")
        if chk["surface"][name]["records_sha256"] != chk["surface_scalar"][name]["records_sha256"]:
            raise SystemExit(f"the two surface arms' records differ on the {name} rays")
    res = {"scene": "config B", "n_tris": chk["surface"]["n_tris"], "n_rays": N_RAYS, "reps": a.reps,
           "record_bytes": {"surface": 48, "trace": 8},
           "identical": {n: dict(hits_sha256=chk["surface"][n]["hits_sha256"][:16],
                                 records_sha256=chk["surface"][n]["records_sha256"][:16],
                                 hit_fraction=chk["surface"][n]["hit_fraction"],
                                 types_seen=chk["surface"][n]["types_seen"]) for n in SETS},
           "rounds": []}
    for rnd in range(a.rounds):
        order = ARMS[rnd % 3:] + ARMS[:rnd % 3]
        row = {arm: run_child(arm, a.reps) for arm in order}
        res["rounds"].append(row)
        print(f"round {rnd}: " + ", ".join(f"{arm} {n} {row[arm][n]['mrays_s']}" for arm in ARMS for n in SETS),
              file=sys.stderr)
    summary = {}
    for n in SETS:
        col = {arm: [r[arm][n]["mrays_s"] for r in res["rounds"]] for arm in ARMS}
        med = {arm: float(np.median(v)) for arm, v in col.items()}
        summary[n] = {f"{arm}_mrays_s": col[arm] for arm in ARMS}
        summary[n]["surface_over_trace"] = round(med["surface"] / med["trace"], 3)
        summary[n]["matrix_wins_every_round"] = min(col["surface"]) > max(col["surface_scalar"])
    lad = {}
    for k in map(str, LADDER):
        mx = [r["surface"]["random"]["ladder"][k]["us"] for r in res["rounds"]]
        sc = [r["surface_scalar"]["random"]["ladder"][k]["us"] for r in res["rounds"]]
        lad[k] = {"matrix_us": mx, "scalar_us": sc, "matrix_wins_every_round": max(mx) < min(sc)}
    summary["ladder_random"] = lad
    summary["matrix_loses_at"] = [int(k) for k in lad if not lad[k]["matrix_wins_every_round"]]
    res["summary"] = summary
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
