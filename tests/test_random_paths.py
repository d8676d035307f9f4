"""The CPU oracle's random paths against tests/random_path_model.py, a float64
restatement of compute.glsl that carries the shader's draw stream, on the
scenes of tests/random_scenes.py (DESIGN.md "Random paths").  No GPU and no
reference tree is needed.

  - the value of a draw, and the frame at which a jitter draw is exactly 1.0;
  - premises: the model's signatures show every use of a draw reached (they
    fail, never skip);
  - the caps on what the comparison rule may exclude;
  - every scene under the rule of random_path_model.assert_image, in brute
    mode, `open_box` through the BVH walk too, with the segment counts.
"""
import numpy as np
import pytest

import random_path_model as rm
import random_scenes as rs
from test_shading_model import bound_textures, scene_data, to_uniforms

SCENES = rs.all_scenes()


def oracle_image(oraclemod, rt2mod, scene, mode="brute", rows=None):
    """-> (mean image over the frames (rows, W, 3), segments)."""
    u = to_uniforms(rt2mod, scene["uniforms"])
    tris, mats, nodes = scene["triangles"], scene["materials"], None
    if mode == "bvh":
        sd = scene_data(rt2mod, scene)
        tris, nodes = sd.triangles(), sd.nodes()
    first, count = scene["frames"]
    rows = np.arange(u.height, dtype=np.int32) if rows is None else np.asarray(rows, np.int32)
    oraclemod.set_textures(bound_textures(scene))
    try:
        acc, _, segs, _ = oraclemod.render(tris, mats, u, rows, first, count, mode, nodes=nodes)
    finally:
        oraclemod.set_textures([])
    return acc[..., :3] / np.float32(count), segs


# --- draws --------------------------------------------------------------------------

def _python_draws(seed, n):
    """compute.glsl:148-152 in Python integers -> the n values of `result`."""
    out = []
    for _ in range(n):
        seed = (seed * 747796405 + 2891336453) % 2 ** 32
        r = (((seed >> ((seed >> 28) + 4)) ^ seed) * 277803737) % 2 ** 32
        out.append((r >> 22) ^ r)
    return out


def test_draw_is_one_is_rederived(oraclemod):
    """The committed frame: the seed from the shader's formula, the generator
    in Python integers, the model's value of the draw and the oracle's."""
    k = rs.DRAW_IS_ONE
    assert rm.frame_term_wraps(k["frame"]) and k["draw"] in (2, 3)
    seed = (k["x"] + k["y"] * rs.W + k["frame"] * 968824447) % 2 ** 32
    assert int(rm.first_seed(k["x"], k["y"], rs.W, k["frame"])) == seed
    bits = _python_draws(seed, k["draw"])
    assert bits[-1] == k["bits"] >= 2 ** 32 - 128
    assert all(b < 2 ** 32 - 128 for b in bits[:-1])
    assert float(rm.draw_value(bits[-1])) == 1.0
    assert float(rm.draw_value(2 ** 32 - 129)) == 1.0 - 2.0 ** -24
    got = oraclemod.pcg_sequence(seed, k["draw"])
    assert [g[0] for g in got] == bits and got[-1][1] == 1.0
    model = rm.model_for(SCENES["draw_is_one"])
    assert model.drew_one[0, k["y"], k["x"]] and not model.excluded[k["y"], k["x"]]
    assert model.draws[0, k["y"], k["x"]] == 3 and int(model.drew_one.sum()) == 1


@pytest.mark.parametrize("name", ["probability_is_one", "roulette_is_one"])
def test_comparison_against_a_draw_of_one(name):
    """The two committed frames at which a comparison meets a draw of 1.0: the
    probability draw (1.0 > 1.0: not a specular bounce, where every other pixel
    of the image has one) and the roulette's (1.0 > 1.0 with p = 1: survived)."""
    k = rs.PROBABILITY_IS_ONE if name == "probability_is_one" else rs.ROULETTE_IS_ONE
    seed = (k["x"] + k["y"] * rs.W + k["frame"] * 968824447) % 2 ** 32
    bits = _python_draws(seed, k["draw"])
    assert bits[-1] >= 2 ** 32 - 128 and all(b < 2 ** 32 - 128 for b in bits[:-1])
    model = rm.model_for(SCENES[name])
    first = model.signature[0, :, :, 0, 0]                                   # (H, W, NF): ray 0, bounce 1
    assert (first[..., rm.F_BRANCH] == rm.SPECULAR).all(), "the floor fills the image"
    here = first[k["y"], k["x"]]
    assert model.drew_one[0, k["y"], k["x"]] and int(model.drew_one.sum()) == 1
    assert not model.excluded[k["y"], k["x"]] and not model.guarded[k["y"], k["x"]]
    assert k["draw"] == 3 + 3 * here[rm.F_CAND] + (1 if name == "probability_is_one" else 2) and here[rm.F_CAND] < 3
    specular = first[..., rm.F_SPECBOUNCE] == 1
    if name == "probability_is_one":
        assert not specular[k["y"], k["x"]] and specular.sum() == specular.size - 1
        assert here[rm.F_ROULETTE] in (rm.RL_KILLED, rm.RL_BELOW_ONE)          # p = 0.8, the floor's colour
    else:
        assert specular.all() and here[rm.F_ROULETTE] == rm.RL_ONE
        assert model.signature[0, k["y"], k["x"], 0, 1, rm.F_END] == rm.END_SKY


def test_draw_values_equal_the_oracles():
    """round24(r) * 2^-32 on integers against the oracle's float, draw for draw:
    equal bits, among them draws that a division by 2^32 - 1 in a wider format
    would round the other way (r at a tie of the 24-bit rounding, rounded down)."""
    import oracle
    n, seed = 1 << 16, 20241020
    got = oracle.pcg_sequence(seed, n)
    bits = np.array(_python_draws(seed, n), np.uint64)
    assert np.array_equal(bits, np.array([g[0] for g in got], np.uint64))
    value = rm.draw_value(bits)
    assert np.array_equal(value, np.array([g[1] for g in got], np.float64))
    assert np.array_equal(value, (bits.astype(np.float32) * np.float32(2.0 ** -32)).astype(np.float64))
    state = np.array([seed], np.uint64)
    assert [int(rm.draw_bits(state, np.array([0]))[0]) for _ in range(64)] == [int(b) for b in bits[:64]]
    wider = (bits.astype(np.float64) / 4294967295.0).astype(np.float32).astype(np.float64)
    assert (wider != value).sum() >= 20


# --- premises -------------------------------------------------------------------------

PREMISES = [
    ("candidates_1", "diffuse_floor/b2"), ("candidates_2", "diffuse_floor/b2"),
    ("candidates_3_or_more", "diffuse_floor/b2"), ("candidates_3_or_more", "diffuse_floor/b3"),
    ("candidates_2", "specular_mix"), ("candidates_3_or_more", "open_box"),
    ("specular_bounce", "specular_mix"), ("specular_declined", "specular_mix"),
    ("killed_at_bounce_1", "diffuse_floor/b2"), ("killed_at_bounce_1", "checker_floor"),
    ("killed_at_a_later_bounce", "glass_tinted"), ("killed_at_a_later_bounce", "open_box"),
    ("survived_below_one", "diffuse_floor/b2"), ("survived_below_one", "diffuse_floor/b3"),
    ("survived_below_one", "specular_mix"), ("survived_below_one", "texture_floor"),
    ("survived_below_one", "glass_tinted"), ("survived_below_one", "open_box"),
    ("survived_at_one", "specular_mix"), ("survived_at_one", "checker_floor"),
    ("survived_at_one", "edge_after_scatter"),
    ("scatter_discarded", "edge_after_scatter"), ("edge_pass_through", "edge_after_scatter"),
    ("checker_black", "checker_floor"), ("checker_white", "checker_floor"), ("texture_sampled", "texture_floor"),
    ("glass_refracted", "glass_tinted"), ("ended_on_light", "jitter_defocus_ramp"), ("ended_on_light", "open_box"),
    ("ended_in_sky", "jitter_sky/r1"), ("ended_in_sky", "jitter_sky/r3"), ("ended_in_sky", "defocus_sky"),
    ("ended_in_sky", "diffuse_floor/b3"), ("cut_at_limit", "open_box"), ("sky_below_horizon", "jitter_sky/r3"),
]


@pytest.mark.parametrize("cls,name", PREMISES, ids=[f"{c}-{n}" for c, n in PREMISES])
def test_premise_branch_is_reached(cls, name):
    n = rm.model_for(SCENES[name]).compared(cls)
    assert n >= 20, f"{name}: only {n} compared pixel-frames take the branch {cls}"


def test_premise_frame_term_wraps():
    """Frames 5, 6, 7: the seed's frame term is past 2^32; frame 0 is there too."""
    wrapped = [n for n, s in SCENES.items() if all(rm.frame_term_wraps(s["frames"][0] + k)
                                                   for k in range(s["frames"][1]))]
    for name in ("jitter_sky/r3", "diffuse_floor/b3", "specular_mix", "glass_tinted", "open_box", "draw_is_one"):
        assert name in wrapped and (~rm.model_for(SCENES[name]).excluded).sum() * SCENES[name]["frames"][1] >= 20
    assert not rm.frame_term_wraps(0) and SCENES["jitter_sky/r1"]["frames"] == (0, 1)
    assert 5 * 968824447 >= 2 ** 32 > 4 * 968824447


def test_premise_draw_counts():
    """What a sample consumes: three draws per ray where nothing is hit; on the
    diffuse floor 3 + 3 * candidates + 1; more where the edge-highlight quad
    drew a direction it dropped than beside it."""
    for name in ("jitter_sky/r1", "jitter_sky/r3", "defocus_sky"):
        m = rm.model_for(SCENES[name])
        assert (m.draws == 3 * SCENES[name]["uniforms"]["numRaysPerPixel"]).all()
    m = rm.model_for(SCENES["diffuse_floor/b3"])
    s = m.signature[:, :, :, 0]
    floor = s[..., 0, rm.F_BRANCH] == rm.DIFFUSE
    assert floor.sum() >= 20 and (s[floor][:, 1, rm.F_TRI] < 0).all()       # the second segment never hits
    few = floor & (s[..., 0, rm.F_CAND] < 3)
    assert (m.draws[few] == 3 + 3 * s[few][:, 0, rm.F_CAND] + 1).all()
    m = rm.model_for(SCENES["edge_after_scatter"])
    s = m.signature
    passed = (s[..., rm.F_DISCARDED] == 1).any(-1)                          # (F, H, W, rays)
    assert (s[passed][:, 1, rm.F_BRANCH] == rm.BR_PASS).all() and (s[passed][:, 1, rm.F_CAND] >= 1).all()
    assert (s[passed][:, 1, rm.F_ROULETTE] == rm.RL_ONE).all() and (s[passed][:, 2, rm.F_END] == rm.END_SKY).all()
    all_pass, none_pass = passed.all(-1), ~passed.any(-1)
    assert all_pass.sum() >= 20 and none_pass.sum() >= 20
    assert m.draws[all_pass].min() >= m.draws[none_pass].min() + 4 * 3


# --- oracle vs model --------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(SCENES))
def test_oracle_matches_model(rt2mod, oraclemod, name):
    scene = SCENES[name]
    model = rm.model_for(scene)
    frac = rm.assert_exclusions(model)
    img, segs = oracle_image(oraclemod, rt2mod, scene)
    worst = rm.assert_image(model, img, "oracle, brute")
    print(f"{name}: max error {worst:.2e}, largest bound {model.bound[~model.excluded].max():.2e}, excluded {frac:.2%}")
    if not model.excluded.any():
        assert segs == int(model.segments.sum())


def test_oracle_bvh_matches_model(rt2mod, oraclemod):
    scene = SCENES["open_box"]
    model = rm.model_for(scene)
    img, segs = oracle_image(oraclemod, rt2mod, scene, "bvh")
    rm.assert_image(model, img, "oracle, bvh")
    if not model.excluded.any():
        assert segs == int(model.segments.sum())
