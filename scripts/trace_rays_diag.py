"""Experiment build (make EXPERIMENTS=1): the resident query kernel's diagnostic counters on the two ray sets of
scripts/trace_rays_ab.py (config B's scene), its y_first arm with and without bounds, and the render's own counters
(variant 350) beside them; one process, one JSON document on stdout (kept: profiles/trace_rays_diag.json)."""
import ctypes as C, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts")); sys.path.insert(0, os.path.join(ROOT, "raytracing2-fork_amd"))
os.environ["RT2_LIB"] = "exp"
import numpy as np, torch, rt2
import trace_rays_ab as A
L = rt2.lib()
L.rt2_scene_set_query_arm.argtypes = [C.c_void_p, C.c_int]
sd, spec = rt2.build_config_scene("B")
u = rt2.offline_uniforms(spec.width, spec.height, spec.bounces, spec.rays, sd.num_triangles)
scene = rt2.Scene(sd, 0)
stream = torch.cuda.current_stream()
hits = torch.zeros(A.N_RAYS * 8, dtype=torch.uint8, device="cuda")
def diag():
    scene.stats(reset=False)
    c = (C.c_ulonglong * 32)(); L.rt2_scene_diag_ex(scene._p, c, 32)
    g = max(c[2], 1)
    return dict(segments=c[1], wave_groups=c[2], hot_per_group=round(c[3] / g, 4), exact_per_group=round(c[4] / g, 4),
                clocks_per_group=dict(setup=round(c[13] / g, 1), products=round(c[14] / g, 1), exact=round(c[15] / g, 1),
                                      sweep=round(c[16] / g, 1)))
def timed(rays, arm, reps=5):
    assert L.rt2_scene_set_query_arm(scene._p, arm) == 0
    scene.trace_rays_device(rays.data_ptr(), A.N_RAYS, hits.data_ptr(), 0, 0)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(stream); scene.trace_rays_device(rays.data_ptr(), A.N_RAYS, hits.data_ptr(), 0, 0); b.record(stream)
    torch.cuda.synchronize()
    return round(float(np.median([a.elapsed_time(b) for a, b in ev])), 3)
out = {}
for name, rays in A.ray_sets(rt2, sd, u).items():
    d = torch.from_numpy(rays.view(np.uint8)).cuda()
    r = {"ms_product": timed(d, 0), "ms_yfirst": timed(d, 2)}
    scene.stats(reset=True); r["ms_diag"] = timed(d, 1, 1); r["diag"] = diag(); scene.stats(reset=True)
    # bounded: tmax = half the distance of each hit (every ray then misses)
    timed(d, 0, 1); h = hits.cpu().numpy().view(rt2.HIT_DTYPE)
    rb = rays.copy(); rb["tmax"] = np.where(h["tri"] >= 0, h["dst"] * np.float32(0.5), 0)
    db = torch.from_numpy(rb.view(np.uint8)).cuda()
    r["bounded_ms_product"] = timed(db, 0); a0 = hits.clone()
    r["bounded_ms_yfirst"] = timed(db, 2); r["bounded_same"] = bool(torch.equal(a0, hits))
    out[name] = r
    print(name, json.dumps(r), file=sys.stderr, flush=True)
# the render's own counters (350 = 353 with the diagnostic clocks), a quarter-size image
scene.set_variant(350)
u2 = rt2.offline_uniforms(960, 540, spec.bounces, spec.rays, sd.num_triangles)
scene.stats(reset=True); scene.render_host(u2, 0, 1); out["render_350"] = diag()
print(json.dumps(out, indent=1))
