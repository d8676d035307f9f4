"""A/B of the occlusion query on the config B scene: rt2_trace_rays AUTO (the
closest-hit kernel a caller had to use before: the baseline), the product's
rt2_occluded on AUTO and on RT2_TRACE_SCALAR, and every A/B arm of
occluded_k5r in the experiment build (rt2_scene_set_occluded_arm; build it with
`make EXPERIMENTS=1`).  Each arm runs in a fresh process per round, the arms'
order reversed from round to round.

Four sets of 2^22 rays, made once by a first child process and read from a
temporary directory by the others:
  shadow   from the default camera's primary hit points toward the light's
           centroid, tmax just short of it
  ao       cosine-weighted hemisphere directions from those points about the
           surface normal, tmax = 5 % of the scene's diagonal
  open     the shadow set's unoccluded rays, repeated
  blocked  the shadow set's occluded rays, repeated
Round 0 checks that every arm gives the same bytes on every set (and that
rt2_trace_rays' tri >= 0 are those bytes); rounds 1.. time one query per set
and arm with HIP events (the median of --reps launches after a warm-up), and a
ladder of prefixes of the shadow set (64 .. 2^18 rays) for the baseline, the
product and the scalar arm: whether AUTO needs a small-batch threshold is read
from it.

Writes ms per arm, set and round to profiles/occluded_ab.json, with the choice
rule of DESIGN.md "Occlusion queries" evaluated on them.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raytracing2-fork_amd"))

N_RAYS = 1 << 22
LADDER = [64, 256, 1024, 4096, 16384, 65536, 262144]
SETS = ("shadow", "ao", "open", "blocked")
# arm -> (library, rt2_scene_set_occluded_arm, what it is)
ARMS = {
    "trace_rays": ("product", 0, "rt2_trace_rays AUTO (trace_rays_k5r): the baseline"),
    "occluded": ("product", 0, "rt2_occluded AUTO, the shipped spec"),
    "scalar": ("product", 0, "rt2_occluded RT2_TRACE_SCALAR"),
    "w38": ("exp", 1, "window 38, no Y, the episode per ray (no exit inside the resident stretch: the control)"),
    "w12": ("exp", 2, "window 12, no Y, per ray"),
    "w6": ("exp", 3, "window 6, no Y, per ray"),
    "w12y": ("exp", 4, "window 12, Y from the second window on, per ray"),
    "w6y": ("exp", 5, "window 6, Y from the second window on, per ray"),
    "w3": ("exp", 6, "window 3, no Y, per ray"),
    "v38": ("exp", 7, "window 38, no Y, the episode per wave (the control of the per-wave form)"),
    "v12": ("exp", 8, "window 12, no Y, per wave"),
    "v6": ("exp", 9, "window 6, no Y, per wave"),
    "v3": ("exp", 10, "window 3, no Y, per wave"),
}
LADDER_ARMS = ("trace_rays", "occluded", "scalar")


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def make_sets(rt2, scene, sd, u, out_dir):
    side = 2048
    assert side * side == N_RAYS
    v = lambda a: np.array([a.x, a.y, a.z], dtype=np.float64)  # noqa: E731
    x, y = np.meshgrid(np.arange(side), np.arange(side))
    px = ((x * 2 - side) / side).reshape(-1, 1)
    py = ((y * 2 - side) / side).reshape(-1, 1)
    d = _unit(v(u.viewportFront) + v(u.viewportRight) * px + v(u.viewportUp) * py)  # render_basic's primary ray
    o = np.broadcast_to(v(u.cameraPos), d.shape)
    dst, tri = scene.trace_rays(o, d)
    hit = np.flatnonzero(tri >= 0)
    pick = np.resize(hit, N_RAYS)  # the hit pixels in raster order, repeated to 2^22
    t = sd.triangles()
    a, b, c = (t[k][:, :3].astype(np.float64) for k in "abc")
    nrm = _unit(np.cross(b - a, c - a))
    lights = np.flatnonzero(sd.materials()["materialType"][t["materialIndex"]] == rt2.LIGHT)
    light = np.concatenate([a[lights], b[lights], c[lights]]).mean(0)
    pts = np.concatenate([a, b, c])
    diag = float(np.linalg.norm(pts.max(0) - pts.min(0)))
    p = o[pick] + d[pick] * dst[pick, None].astype(np.float64)
    n = nrm[tri[pick]]
    n = np.where((np.einsum("ij,ij->i", n, d[pick]) > 0)[:, None], -n, n)  # toward the camera's side
    p = p + n * (1e-4 * diag)
    rng = np.random.default_rng(2)
    sets = {}
    to = light - p
    dist = np.linalg.norm(to, axis=1)
    sh = np.zeros(N_RAYS, rt2.RAY_DTYPE)
    sh["o"], sh["d"], sh["tmax"] = p, to / dist[:, None], dist * 0.999
    sets["shadow"] = sh
    # cosine-weighted: n + a uniform point of the unit sphere
    ao = np.zeros(N_RAYS, rt2.RAY_DTYPE)
    ao["o"], ao["d"], ao["tmax"] = p, _unit(n + 0.999 * _unit(rng.normal(size=(N_RAYS, 3)))), 0.05 * diag
    sets["ao"] = ao
    occ = scene.occluded(sh["o"], sh["d"], sh["tmax"], rt2.TRACE_SCALAR)
    assert occ.any() and (~occ).any(), "the shadow set needs both kinds of rays"
    sets["open"] = sh[np.resize(np.flatnonzero(~occ), N_RAYS)]
    sets["blocked"] = sh[np.resize(np.flatnonzero(occ), N_RAYS)]
    for name, rays in sets.items():
        np.save(os.path.join(out_dir, name + ".npy"), rays)
    return {"primary_hit_fraction": round(len(hit) / N_RAYS, 4), "shadow_occluded_fraction": round(float(occ.mean()), 4),
            "light": [round(float(x), 4) for x in light], "ao_tmax": round(0.05 * diag, 4)}


def child(a):
    import torch
    import rt2
    sd, spec = rt2.build_config_scene("B")
    u = rt2.offline_uniforms(spec.width, spec.height, spec.bounces, spec.rays, sd.num_triangles)
    scene = rt2.Scene(sd, 0)
    if a.arm == "make_sets":
        print(json.dumps(make_sets(rt2, scene, sd, u, a.sets)))
        return
    lib, arm_id, _ = ARMS[a.arm]
    assert (os.environ.get("RT2_LIB") == "exp") == (lib == "exp")
    if lib == "exp" and rt2.lib().rt2_scene_set_occluded_arm(scene._p, arm_id) != 0:
        raise SystemExit("rt2_scene_set_occluded_arm failed")
    stream = torch.cuda.current_stream()
    out = {"arm": a.arm, "n_tris": sd.num_triangles}
    flags = rt2.TRACE_SCALAR if a.arm == "scalar" else rt2.TRACE_AUTO
    buf = torch.zeros(N_RAYS * 8, dtype=torch.uint8, device="cuda")

    def launch(rays, n):
        if a.arm == "trace_rays":
            scene.trace_rays_device(rays.data_ptr(), n, buf.data_ptr(), flags, stream.cuda_stream)
        else:
            scene.occluded_device(rays.data_ptr(), n, buf.data_ptr(), flags, stream.cuda_stream)

    def timed(rays, n, reps):
        launch(rays, n)  # warm-up
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for e0, e1 in ev:
            e0.record(stream)
            launch(rays, n)
            e1.record(stream)
        torch.cuda.synchronize()
        return float(np.median([e0.elapsed_time(e1) for e0, e1 in ev]))

    for name in SETS:
        rays = np.load(os.path.join(a.sets, name + ".npy"))
        d_rays = torch.from_numpy(rays.view(np.uint8)).cuda()
        ms = timed(d_rays, N_RAYS, a.reps)
        res = {"ms": round(ms, 3), "mrays_s": round(N_RAYS / ms / 1e3, 1), "kernel": scene.last_kernel()}
        if a.check:
            h = buf.cpu().numpy()
            occ = (h.view(rt2.HIT_DTYPE)["tri"] >= 0) if a.arm == "trace_rays" else h[:N_RAYS].astype(bool)
            if a.arm != "trace_rays" and (h[:N_RAYS] > 1).any():
                raise SystemExit("a result byte is neither 0 nor 1")
            res["sha256"] = hashlib.sha256(np.packbits(occ).tobytes()).hexdigest()
            res["occluded_fraction"] = round(float(occ.mean()), 4)
        elif name == "shadow" and a.arm in LADDER_ARMS:
            res["ladder_us"] = {str(n): round(timed(d_rays, n, 4 * a.reps) * 1e3, 2) for n in LADDER}
        out[name] = res
    print(json.dumps(out))


def run_child(arm, sets, reps, check=False):
    env = dict(os.environ)
    env.pop("RT2_LIB", None)
    if arm in ARMS and ARMS[arm][0] == "exp":
        env["RT2_LIB"] = "exp"
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--arm", arm, "--reps", str(reps), "--sets", sets] + \
          (["--check"] if check else [])
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=300, env=env)
    if r.returncode != 0:
        raise SystemExit(f"{arm} child failed with status {r.returncode}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def summarise(res):
    """The choice rule: among the arms that on `open` are no slower than
    trace_rays beyond the spread of trace_rays' own rounds, the fastest on
    `shadow` (medians over the rounds)."""
    ms = {arm: {s: [r[arm][s]["ms"] for r in res["rounds"]] for s in SETS} for arm in ARMS}
    base = ms["trace_rays"]
    spread = max(base["open"]) - min(base["open"])
    limit = float(np.median(base["open"])) + spread
    matrix = [arm for arm in ARMS if arm not in ("trace_rays", "scalar", "occluded")]
    tie = [arm for arm in matrix if float(np.median(ms[arm]["open"])) <= limit]
    best = min(tie, key=lambda arm: float(np.median(ms[arm]["shadow"])), default=None)
    return {
        "ms": ms,
        "open_limit_ms": round(limit, 3), "trace_rays_open_spread_ms": round(spread, 3),
        "arms_within_open_limit": tie, "fastest_of_them_on_shadow": best,
        "shipped_blocked_every_round_faster_than_trace_rays_fastest": max(ms["occluded"]["blocked"]) < min(base["blocked"]),
        "shipped_open_within_limit": float(np.median(ms["occluded"]["open"])) <= limit,
        "ladder_us": {arm: {str(n): [r[arm]["shadow"]["ladder_us"][str(n)] for r in res["rounds"]] for n in LADDER}
                      for arm in LADDER_ARMS},
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--arm", default="occluded", choices=list(ARMS) + ["make_sets"])
    ap.add_argument("--sets", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "occluded_ab.json"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    with tempfile.TemporaryDirectory() as sets:
        info = run_child("make_sets", sets, 1)
        print("sets:", json.dumps(info), file=sys.stderr)
        chk = {arm: run_child(arm, sets, 1, check=True) for arm in ARMS}
        for s in SETS:
            if len({chk[arm][s]["sha256"] for arm in ARMS}) != 1:
                raise SystemExit(f"the arms' results differ on the {s} rays: " +
                                 ", ".join(f"{arm} {chk[arm][s]['occluded_fraction']}" for arm in ARMS))
        res = {"scene": "config B", "n_tris": chk["occluded"]["n_tris"], "n_rays": N_RAYS, "reps": a.reps,
               "arms": {arm: ARMS[arm][2] for arm in ARMS}, "sets": info,
               "identical": {s: dict(sha256=chk["occluded"][s]["sha256"][:16],
                                     occluded_fraction=chk["occluded"][s]["occluded_fraction"]) for s in SETS},
               "rounds": []}
        for rnd in range(a.rounds):
            order = list(ARMS) if rnd % 2 == 0 else list(ARMS)[::-1]
            row = {arm: run_child(arm, sets, a.reps) for arm in order}
            res["rounds"].append(row)
            print(f"round {rnd}: " + ", ".join(f"{arm} " + "/".join(str(row[arm][s]["ms"]) for s in SETS)
                                                 for arm in ARMS), file=sys.stderr)
    res["summary"] = summarise(res)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res["summary"].items() if k not in ("ms", "ladder_us")}))


if __name__ == "__main__":
    main()
