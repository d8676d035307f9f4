"""Matrix-filter survivor statistics (diagnostic variants 350 / 390 / 368 = the
resident kernel 391 with the default window and per group, and the tile stream
370, plus counters; experiment build, RT2_LIB=exp): per (wave, 32-triangle
group) sweep, how often a pair passes the filter (the wave enters the exact
phase) and how many (wave, triangle) exact tests follow; for the resident
kernel also its phase clocks and, per exact episode, the (ray, triangle) pairs,
the busiest ray's pairs and the rounds of 32 hot triangles (350: counted on
the exact quantities; 402, the per-ray episode MfmaSpec::exact_lanes: what
it ran; 422, MfmaSpec::exact_spread: the rounds' leftover pairs)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raytracing2-fork_amd"))
import torch  # noqa: E402,F401
import rt2  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="B")
ap.add_argument("--variants", default="391,350")
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
a = ap.parse_args()
sd, spec = rt2.build_config_scene(a.config)
u = rt2.offline_uniforms(a.width, a.height, spec.bounces, spec.rays, sd.num_triangles)
scene = rt2.Scene(sd, 0)
res = {"config": a.config, "width": a.width, "height": a.height, "triangles": sd.num_triangles}
imgs = {}


def name_of(v):
    return rt2.lib().rt2_variant_name(v).decode()


for v in [int(x) for x in a.variants.split(",")]:
    scene.set_variant(v)
    scene.render_host(u, 0, 1)  # warm
    scene.stats(reset=True)
    t = time.perf_counter()
    img = scene.render_host(u, 0, 1)
    dt = time.perf_counter() - t
    st = scene.stats(reset=False)
    c = (C.c_ulonglong * 32)()
    rt2.lib().rt2_scene_diag_ex(scene._p, c, 32)
    scene.stats(reset=True)
    imgs[v] = img
    groups, hot, exact = c[2], c[3], c[4]
    res[name_of(v)] = dict(
        ms=round(dt * 1e3, 1), segments=st.segments, wave_groups=groups,
        hot_group_rate=hot / max(groups, 1), exact_tests_per_group=exact / max(groups, 1),
        exact_tests_per_hot_group=exact / max(hot, 1),
        wave_triangle_exact_rate=exact / max(32 * groups, 1))
    life = c[17]
    if life and name_of(v).startswith(("mfmar/", "mfmarl2/")):
        # the resident kernel's phase clocks (rt2_k5_resident.h): shares of the waves' life, and of the exact phase
        # its three parts (the wait for an episode's first triangle, the tests, the Y rebuilds)
        setup, filt, ex, load, reb, episodes = c[13], c[14], c[15], c[18], c[19], c[20]
        sweeps = groups / max((sd.num_triangles + 31) // 32, 1)
        res[name_of(v)].update(
            life_share=dict(setup=round(setup / life, 4), products=round(filt / life, 4), exact=round(ex / life, 4),
                            outside_sweep=round(1 - c[16] / life, 4)),
            product_clocks_per_group=round(filt / max(groups, 1), 1),
            exact_clocks_per_hot_group=round(ex / max(hot, 1), 1),
            episodes_per_sweep=round(episodes / max(sweeps, 1), 2),
            exact_clocks_per_episode=dict(first_load_wait=round(load / max(episodes, 1), 1),
                                          tests=round((ex - load - reb) / max(episodes, 1), 1),
                                          y_rebuild=round(reb / max(episodes, 1), 1),
                                          whole=round(ex / max(episodes, 1), 1)))
        # PathDiag (rt2_path.h): the work outside the sweep per wave-segment (a wave's sweep): rnd_dir calls (one per
        # material kind the wave's hits have) and the trips of their rejection loops, advance's new-ray and
        # new-frame blocks
        rd_calls, rd_trips, new_ray, new_px = c[21], c[22], c[23], c[24]
        if rd_calls:
            res[name_of(v)].update(
                outside_sweep=dict(wave_segments=int(sweeps), rnd_dir_calls=rd_calls, rnd_dir_trips=rd_trips,
                                   rnd_dir_calls_per_wave_segment=round(rd_calls / max(sweeps, 1), 4),
                                   rnd_dir_trips_per_call=round(rd_trips / rd_calls, 3),
                                   rnd_dir_trips_per_wave_segment=round(rd_trips / max(sweeps, 1), 3),
                                   new_ray_blocks_per_wave_segment=round(new_ray / max(sweeps, 1), 4),
                                   new_frame_blocks_per_wave_segment=round(new_px / max(sweeps, 1), 4)))
        # ClusterDiag (MfmaSpec::cluster_rows diag: 411, 416, 419): the (wave, compact cluster) cases of the sweeps;
        # rows8 (the cases of 1 to 8 needing rays) is counted by 419 alone
        cases = c[25] + c[26] + c[27]
        if cases:
            res[name_of(v)].update(
                cluster_rows=dict(skipped=int(c[25]), one_block=int(c[26]), two_blocks=int(c[27]),
                                  needing_rays=int(c[28]), rows16=int(c[29]), rows8=int(c[31]),
                                  needing_rays_per_case=round(c[28] / cases, 2),
                                  rows16_share=round(c[29] / cases, 4), rows8_share=round(c[31] / cases, 4)))
        # MfmaDiag::xl: per episode, the (ray, triangle) pairs that pass the filter's U, -V, X conditions, the
        # largest count of one ray (what a per-lane test loop runs; exact_lanes arms: its iterations) and the
        # rounds of 32 hot triangles
        pairs, ksum, rounds, kmax = c[8], c[9], c[10], c[11]
        if rounds:
            res[name_of(v)].update(
                lanes=dict(hot_triangles_per_episode=round(exact / max(episodes, 1), 2),
                           pairs_per_episode=round(pairs / max(episodes, 1), 2),
                           pairs_per_hot_triangle=round(pairs / max(exact, 1), 2),
                           k_per_episode=round(ksum / max(episodes, 1), 2), k_max=kmax,
                           rounds_per_episode=round(rounds / max(episodes, 1), 3)))
        # SpreadDiag (MfmaSpec::exact_spread diag: 422): per round of an episode, the pairs left after every lane's first
        # (Rw), the rounds that dealt them out over the wave, and those that fell back on Rw > 64; the rest of the
        # rounds had no leftover, or no lane with two
        left, packed = c[5], c[12]
        if rounds and (left or packed):
            sp, big = packed & ((1 << 40) - 1), packed >> 40
            res[name_of(v)].update(
                spread=dict(leftovers_per_round=round(left / rounds, 2), leftovers_per_spread_round=round(left / max(sp, 1), 2),
                            spread_round_share=round(sp / rounds, 4), over_64_round_share=round(big / rounds, 6),
                            other_round_share=round(1 - (sp + big) / rounds, 4)))
vs = list(imgs)
res["bit_identical"] = all(bool((imgs[v] == imgs[vs[0]]).all()) for v in vs[1:])
print(json.dumps(res, indent=1))
