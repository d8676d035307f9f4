"""A/B of the ray query's two brute-force kernels on the config B scene:
RT2_TRACE_AUTO's matrix kernel (trace_rays_k5r) against RT2_TRACE_SCALAR
(trace_rays_scalar), each arm in a fresh process per round, the arms
alternating (scripts/gpu_run.sh: TRACE_AB=<rounds>).

Two sets of 2^22 rays: "coherent" (the default camera's primary rays of a
2048 x 2048 image, raster order) and "random" (uniformly random directions
from points inside the scene's bounding box).  Round 0 checks that both arms
give identical hits on both sets (a digest per set); rounds 1.. time one query
per set and arm with HIP events (the median of --reps launches after a
warm-up), and a ladder of prefixes of the random set (64 .. 2^18 rays): whether
RT2_TRACE_AUTO needs a small-batch threshold below which the scalar kernel
runs (rt2_trace_rays in rt2_render.hip) is read from it.  Every
round also times one rt2_render of config B and reports its own segments/s
(rt2_scene_stats), the rate the query is compared with.

Writes Mrays/s per arm and round to profiles/trace_rays_ab.json.
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

N_RAYS = 1 << 22
LADDER = [64, 256, 1024, 4096, 16384, 65536, 262144]


def ray_sets(rt2, sd, u):
    side = 2048
    assert side * side == N_RAYS
    v = lambda a: np.array([a.x, a.y, a.z], dtype=np.float64)  # noqa: E731
    x, y = np.meshgrid(np.arange(side), np.arange(side))
    px = ((x * 2 - side) / side).reshape(-1, 1)
    py = ((y * 2 - side) / side).reshape(-1, 1)
    d = v(u.viewportFront) + v(u.viewportRight) * px + v(u.viewportUp) * py  # render_basic's primary ray
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    coherent = np.zeros(N_RAYS, rt2.RAY_DTYPE)
    coherent["o"], coherent["d"] = v(u.cameraPos), d
    rng = np.random.default_rng(1)
    t = sd.triangles()
    pts = np.concatenate([t[k][:, :3] for k in "abc"]).astype(np.float64)
    lo, hi = pts.min(0), pts.max(0)
    lo, hi = lo + 0.05 * (hi - lo), hi - 0.05 * (hi - lo)
    d = rng.normal(size=(N_RAYS, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    random = np.zeros(N_RAYS, rt2.RAY_DTYPE)
    random["o"], random["d"] = rng.uniform(lo, hi, (N_RAYS, 3)), d
    return {"coherent": coherent, "random": random}


def child(a):
    import torch
    import rt2
    sd, spec = rt2.build_config_scene("B")
    u = rt2.offline_uniforms(spec.width, spec.height, spec.bounces, spec.rays, sd.num_triangles)
    scene = rt2.Scene(sd, 0)
    stream = torch.cuda.current_stream()
    out = {"arm": a.arm, "n_tris": sd.num_triangles}
    if a.arm == "render":
        acc = torch.zeros(spec.height * spec.width * 4, dtype=torch.float32, device="cuda")
        ms = []
        for i in range(2):  # a warm-up, then the timed one
            scene.stats(reset=True)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            scene.render(u, 0, spec.frames, rt2.shard(), acc.data_ptr(), 0, stream.cuda_stream)
            e1.record(stream)
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        st = scene.stats(reset=True)
        out.update(render_ms=round(ms[1], 3), segments=int(st.segments),
                   msegments_s=round(st.segments / ms[1] / 1e3, 1), kernel=scene.last_kernel())
        print(json.dumps(out))
        return
    flags = rt2.TRACE_SCALAR if a.arm == "scalar" else rt2.TRACE_AUTO
    hits = torch.zeros(N_RAYS * 8, dtype=torch.uint8, device="cuda")

    def timed(rays, n, reps):
        scene.trace_rays_device(rays.data_ptr(), n, hits.data_ptr(), flags, stream.cuda_stream)  # warm-up
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for e0, e1 in ev:
            e0.record(stream)
            scene.trace_rays_device(rays.data_ptr(), n, hits.data_ptr(), flags, stream.cuda_stream)
            e1.record(stream)
        torch.cuda.synchronize()
        return float(np.median([e0.elapsed_time(e1) for e0, e1 in ev]))

    for name, rays in ray_sets(rt2, sd, u).items():
        d_rays = torch.from_numpy(rays.view(np.uint8)).cuda()
        ms = timed(d_rays, N_RAYS, a.reps)
        res = {"ms": round(ms, 3), "mrays_s": round(N_RAYS / ms / 1e3, 1), "kernel": scene.last_kernel()}
        if a.check:
            h = hits.cpu().numpy().view(rt2.HIT_DTYPE)
            res["sha256"] = hashlib.sha256(h.tobytes()).hexdigest()
            res["hit_fraction"] = round(float((h["tri"] >= 0).mean()), 4)
        if name == "random" and not a.check:
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
    ap.add_argument("--arm", default="auto", choices=["auto", "scalar", "render"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trace_rays_ab.json"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    chk = {arm: run_child(arm, 1, check=True) for arm in ("auto", "scalar")}
    for name in ("coherent", "random"):
        if chk["auto"][name]["sha256"] != chk["scalar"][name]["sha256"]:
            raise SystemExit(f"the two arms' hits differ on the {name} rays")
    res = {"scene": "config B", "n_tris": chk["auto"]["n_tris"], "n_rays": N_RAYS, "reps": a.reps,
           "identical": {n: dict(sha256=chk["auto"][n]["sha256"][:16], hit_fraction=chk["auto"][n]["hit_fraction"])
                         for n in ("coherent", "random")},
           "rounds": []}
    for rnd in range(a.rounds):
        order = ("auto", "scalar") if rnd % 2 == 0 else ("scalar", "auto")
        row = {arm: run_child(arm, a.reps) for arm in order}
        row["render"] = run_child("render", 1)
        res["rounds"].append(row)
        print(f"round {rnd}: " + ", ".join(f"{arm} {n} {row[arm][n]['mrays_s']}" for arm in ("auto", "scalar")
                                             for n in ("coherent", "random")), file=sys.stderr)
    # AUTO stays on the matrix kernel only where every one of its rounds beats the scalar arm's fastest
    summary = {}
    for n in ("coherent", "random"):
        au = [r["auto"][n]["mrays_s"] for r in res["rounds"]]
        sc = [r["scalar"][n]["mrays_s"] for r in res["rounds"]]
        summary[n] = {"auto_mrays_s": au, "scalar_mrays_s": sc, "matrix_wins_every_round": min(au) > max(sc)}
    lad = {}
    for k in map(str, LADDER):
        au = [r["auto"]["random"]["ladder"][k]["us"] for r in res["rounds"]]
        sc = [r["scalar"]["random"]["ladder"][k]["us"] for r in res["rounds"]]
        lad[k] = {"matrix_us": au, "scalar_us": sc, "matrix_wins_every_round": max(au) < min(sc)}
    summary["ladder_random"] = lad
    wins = [int(k) for k in lad if lad[k]["matrix_wins_every_round"]]
    loses = [int(k) for k in lad if not lad[k]["matrix_wins_every_round"]]
    summary["matrix_min_rays"] = min([k for k in wins if not loses or k > max(loses)], default=None)
    summary["render_msegments_s"] = [r["render"]["msegments_s"] for r in res["rounds"]]
    res["summary"] = summary
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
