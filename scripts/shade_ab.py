"""A/B of the preview shading query on the config B scene: rt2_shade_rays with
RT2_TRACE_AUTO (shade_rays_k5r) against rt2_shade_rays with RT2_TRACE_SCALAR
(shade_rays_scalar) and against rt2_render with basicShading = 1 and one frame
(render_basic, the kernel the project had before the query: the yardstick),
each arm in a fresh process per round, the arms rotating.

Two workloads: the 2^22 coherent rays of scripts/trace_rays_ab.py (the two
query arms), and a 1,920 x 1,080 view (the query arms through the chain
Scene.preview issues, rt2_camera_rays then rt2_shade_rays on one stream; the
render arm on the same uniforms).  Settings: the shadow ray off and on,
max_bounce 1 and the scene's offline default.  Round 0 checks that the two
query arms give identical records on the rays and that all three arms give the
same image; rounds 1.. time each with HIP events (the median of --reps launches
after a warm-up), and a ladder of prefixes of the random ray set (64 .. 2^18
rays, the shadow ray on, the default bounce limit) for the two query arms:
where RT2_TRACE_AUTO's matrix kernel wins in every round is read from it.

No ratio is fixed in advance.  Writes the times per arm and round to
profiles/shade_ab.json.
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

ARMS = ("shade", "shade_scalar", "render")
VIEW = (1920, 1080)
LIGHT = (0.0, 8.0, 2.0)


def settings(spec):
    return [(shadow, mb) for shadow in (0, 1) for mb in (1, spec.bounces)]


def child(a):
    import torch
    import rt2
    sd, spec = rt2.build_config_scene("B")
    u = rt2.offline_uniforms(spec.width, spec.height, spec.bounces, spec.rays, sd.num_triangles)
    scene = rt2.Scene(sd, 0)
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    out = {"arm": a.arm, "n_tris": sd.num_triangles, "default_bounces": spec.bounces}
    flags = rt2.TRACE_SCALAR if a.arm == "shade_scalar" else rt2.TRACE_AUTO

    def timed(launch, reps):
        launch()  # warm-up
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for e0, e1 in ev:
            e0.record(stream)
            launch()
            e1.record(stream)
        torch.cuda.synchronize()
        return float(np.median([e0.elapsed_time(e1) for e0, e1 in ev]))

    # the view: the uniforms of a 1,920 x 1,080 default camera
    vu = rt2.camera_uniforms(rt2.default_camera(*VIEW),
                             rt2.offline_uniforms(VIEW[0], VIEW[1], spec.bounces, 1, sd.num_triangles))
    vu.basicShading = 1
    vu.basicShadingLightPosition = rt2.Vec4(LIGHT[0], LIGHT[1], LIGHT[2], 1.0)
    npix = VIEW[0] * VIEW[1]
    d_view_rays = torch.zeros(npix * rt2.RAY_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_img = torch.zeros(npix * 16, dtype=torch.uint8, device="cuda")
    out["view"] = {}
    for shadow, mb in settings(spec):
        vu.basicShadingShadow, vu.maxBounceCount = shadow, mb
        if a.arm == "render":
            def launch():
                d_img.zero_()
                scene.render(vu, 0, 1, rt2.shard(), d_img.data_ptr(), 0, sp)
        else:
            def launch():
                scene.camera_rays_device(vu, rt2.shard(), d_view_rays.data_ptr(), sp)
                scene.shade_rays_device(d_view_rays.data_ptr(), npix, d_img.data_ptr(), LIGHT, bool(shadow), mb, flags,
                                        sp)
        ms = timed(launch, a.reps)
        res = {"ms": round(ms, 3), "mpix_s": round(npix / ms / 1e3, 1), "kernel": scene.last_kernel()}
        if a.check:
            img = d_img.cpu().numpy().view(np.float32).reshape(-1, 4)[:, :3]
            res["rgb_sha256"] = hashlib.sha256(np.ascontiguousarray(img).tobytes()).hexdigest()
        out["view"][f"s{shadow}b{mb}"] = res
    if a.arm == "render":
        print(json.dumps(out))
        return
    # the caller's rays
    d_out = torch.zeros(N_RAYS * rt2.SHADED_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    sets = ray_sets(rt2, sd, u)
    d_rays = torch.from_numpy(sets["coherent"].view(np.uint8)).cuda()
    out["coherent"] = {}
    for shadow, mb in settings(spec):
        def launch(n=N_RAYS, rays=d_rays):
            scene.shade_rays_device(rays.data_ptr(), n, d_out.data_ptr(), LIGHT, bool(shadow), mb, flags, sp)
        ms = timed(launch, a.reps)
        res = {"ms": round(ms, 3), "mrays_s": round(N_RAYS / ms / 1e3, 1), "kernel": scene.last_kernel()}
        if a.check:
            rec = d_out.cpu().numpy().view(rt2.SHADED_DTYPE)
            res["records_sha256"] = hashlib.sha256(rec.tobytes()).hexdigest()
            res["segments_per_ray"] = round(float(rec["segments"].mean()), 3)
        out["coherent"][f"s{shadow}b{mb}"] = res
    if not a.check:
        d_rand = torch.from_numpy(sets["random"].view(np.uint8)).cuda()
        out["ladder"] = {}
        for n in LADDER:
            ms = timed(lambda: scene.shade_rays_device(d_rand.data_ptr(), n, d_out.data_ptr(), LIGHT, True, spec.bounces,
                                                       flags, sp), 4 * a.reps)
            out["ladder"][str(n)] = {"us": round(ms * 1e3, 2), "mrays_s": round(n / ms / 1e3, 2)}
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
    ap.add_argument("--arm", default="shade", choices=list(ARMS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shade_ab.json"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    chk = {arm: run_child(arm, 1, check=True) for arm in ARMS}
    keys = list(chk["shade"]["coherent"])
    for k in keys:
        if chk["shade"]["coherent"][k]["records_sha256"] != chk["shade_scalar"]["coherent"][k]["records_sha256"]:
            raise SystemExit(f"the two query arms' records differ on the coherent rays, {k}")
        if len({chk[arm]["view"][k]["rgb_sha256"] for arm in ARMS}) != 1:
            raise SystemExit(f"the arms' images differ, {k}")
    res = {"scene": "config B", "n_tris": chk["shade"]["n_tris"], "n_rays": N_RAYS, "view": list(VIEW),
           "reps": a.reps, "light": list(LIGHT), "default_bounces": chk["shade"]["default_bounces"],
           "settings": {k: "shadow %s, max_bounce %s" % tuple(k[1:].split("b")) for k in keys},
           "identical": {k: dict(records_sha256=chk["shade"]["coherent"][k]["records_sha256"][:16],
                                 view_rgb_sha256=chk["shade"]["view"][k]["rgb_sha256"][:16],
                                 segments_per_ray=chk["shade"]["coherent"][k]["segments_per_ray"]) for k in keys},
           "rounds": []}
    for rnd in range(a.rounds):
        order = ARMS[rnd % 3:] + ARMS[:rnd % 3]
        row = {arm: run_child(arm, a.reps) for arm in order}
        res["rounds"].append(row)
        print(f"round {rnd}: " + ", ".join(f"{arm} view {k} {row[arm]['view'][k]['ms']} ms" for arm in ARMS for k in keys),
              file=sys.stderr)
    summary = {"coherent": {}, "view": {}}
    for k in keys:
        col = {arm: [r[arm]["coherent"][k]["ms"] for r in res["rounds"]] for arm in ARMS[:2]}
        summary["coherent"][k] = {f"{arm}_ms": col[arm] for arm in col}
        summary["coherent"][k]["scalar_over_matrix"] = round(float(np.median(col["shade_scalar"]) /
                                                                   np.median(col["shade"])), 3)
        summary["coherent"][k]["matrix_wins_every_round"] = max(col["shade"]) < min(col["shade_scalar"])
        col = {arm: [r[arm]["view"][k]["ms"] for r in res["rounds"]] for arm in ARMS}
        summary["view"][k] = {f"{arm}_ms": col[arm] for arm in col}
        summary["view"][k]["render_over_matrix"] = round(float(np.median(col["render"]) / np.median(col["shade"])), 3)
        summary["view"][k]["matrix_wins_every_round"] = max(col["shade"]) < min(min(col["shade_scalar"]),
                                                                               min(col["render"]))
    lad = {}
    for k in map(str, LADDER):
        mx = [r["shade"]["ladder"][k]["us"] for r in res["rounds"]]
        sc = [r["shade_scalar"]["ladder"][k]["us"] for r in res["rounds"]]
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
