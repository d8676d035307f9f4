"""A/B of the linear render on configs B and K (1,920 x 1,080, 64 rays per
pixel, one frame; K is the L2 form of the resident kernel): rt2_render, this
build (the yardstick: the same paths, tonemapped), rt2_render_linear without
moments, rt2_render_linear with moments, and Scene.radiance_image (the query
chain that gave the linear image before), each arm in a fresh process per
round, the arms rotating.

Round 0 checks that the two linear arms and the chain give the same linear
image, bit for bit, on both configs (the linear sum of one frame is the frame's
mean; the chain's image is its samples' sum over numRaysPerPixel), and that the
sums are the same with and without moments.  Rounds 1.. time the three render
arms with HIP events around the launch (the median of --reps launches after a
warm-up; the arrays are zeroed outside the timed span) and the chain by the
wall clock around the blocking call, which ends with its copies to the host.

No ratio is fixed in advance.  The spread of the rt2_render arm from process to
process is what the linear arm's difference is read against.  Writes the times
per arm and round to profiles/linear_ab.json.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raytracing2-fork_amd"))

ARMS = ("render", "linear", "linear_moments", "chain")
CONFIGS = ("B", "K")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def child(a):
    import torch
    import rt2
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    out = {"arm": a.arm}

    def timed(prepare, launch, reps):
        prepare()
        launch()  # warm-up
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for e0, e1 in ev:
            prepare()
            e0.record(stream)
            launch()
            e1.record(stream)
        torch.cuda.synchronize()
        return [round(float(e0.elapsed_time(e1)), 3) for e0, e1 in ev]

    def wall(call, reps):
        call()  # warm-up
        t = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            t.append(round((time.perf_counter() - t0) * 1e3, 3))
        return t

    for config in CONFIGS:
        sd, spec = rt2.build_config_scene(config)
        u = rt2.offline_uniforms(spec.width, spec.height, spec.bounces, spec.rays, sd.num_triangles)
        scene = rt2.Scene(sd, 0)
        npix = spec.width * spec.height
        res = {"n_tris": sd.num_triangles}
        out[config] = res
        if a.arm == "chain":
            img = [None]

            def image():
                img[0] = scene.radiance_image(u, 0)
            t = wall(image, 1 if a.check else a.reps)
            res.update(ms=t, kernel=scene.last_kernel())
            if a.check:
                res["linear_sha256"] = sha(img[0][0])
            continue
        d_sum = torch.zeros(npix * 4, dtype=torch.float32, device="cuda")
        d_sq = torch.zeros(npix * 4, dtype=torch.float32, device="cuda")

        def zero():
            d_sum.zero_()
            d_sq.zero_()

        if a.arm == "render":
            def launch():
                scene.render(u, 0, 1, rt2.shard(), d_sum.data_ptr(), 0, sp)
        elif a.arm == "linear":
            def launch():
                scene.render_linear(u, 0, 1, rt2.shard(), d_sum.data_ptr(), 0, sp)
        else:
            def launch():
                scene.render_linear(u, 0, 1, rt2.shard(), d_sum.data_ptr(), d_sq.data_ptr(), sp)
        t = timed(zero, launch, 1 if a.check else a.reps)
        res.update(ms=t, kernel=scene.last_kernel())
        if a.check and a.arm != "render":
            res["linear_sha256"] = sha(d_sum.cpu().numpy().reshape(npix, 4)[:, :3])
            if a.arm == "linear_moments":
                res["moments_sha256"] = sha(d_sq.cpu().numpy())
    print(json.dumps(out))


def run_child(arm, reps, check=False):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--arm", arm, "--reps", str(reps)] + \
          (["--check"] if check else [])
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit(f"{arm} child failed with status {r.returncode}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--arm", default="linear", choices=list(ARMS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linear_ab.json"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    chk = {arm: run_child(arm, 1, check=True) for arm in ARMS[1:]}
    identical = {}
    for config in CONFIGS:
        h = {arm: chk[arm][config]["linear_sha256"] for arm in ARMS[1:]}
        if len(set(h.values())) != 1:
            raise SystemExit(f"the linear images differ on config {config}: {h}")
        identical[config] = dict(linear_sha256=h["linear"][:16], moments_sha256=chk["linear_moments"][config]
                                 ["moments_sha256"][:16], kernel=chk["linear"][config]["kernel"],
                                 chain_kernel=chk["chain"][config]["kernel"])
    res = {"scene": "configs B and K, 1,920 x 1,080, 64 rays per pixel, one frame",
           "n_tris": {c: chk["linear"][c]["n_tris"] for c in CONFIGS}, "reps": a.reps, "identical": identical,
           "not_measured": ["counters (no rocprofv3 run)", "BVH traversal", "more than one GPU", "several frames per call",
                            "scenes beyond configs B and K"],
           "rounds": []}
    for rnd in range(a.rounds):
        k = rnd % len(ARMS)
        order = ARMS[k:] + ARMS[:k]
        row = {arm: run_child(arm, a.reps) for arm in order}
        res["rounds"].append(row)
        print(f"round {rnd}: " + "; ".join(f"{arm} {[float(np.median(row[arm][c]['ms'])) for c in CONFIGS]}"
                                          for arm in ARMS), file=sys.stderr)
    summary = {}
    for config in CONFIGS:
        med = {arm: [float(np.median(r[arm][config]["ms"])) for r in res["rounds"]] for arm in ARMS}
        m = {arm: float(np.median(med[arm])) for arm in ARMS}
        summary[config] = {
            **{f"{arm}_ms": med[arm] for arm in ARMS},
            "kernels": {arm: res["rounds"][0][arm][config]["kernel"] for arm in ARMS},
            "render_spread": round((max(med["render"]) - min(med["render"])) / m["render"], 4),
            "linear_over_render": round(m["linear"] / m["render"], 4),
            "moments_over_linear": round(m["linear_moments"] / m["linear"], 4),
            "chain_over_linear": round(m["chain"] / m["linear"], 3),
        }
    res["summary"] = summary
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
