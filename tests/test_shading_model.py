"""The CPU oracle's shade() against tests/shading_model.py, an independent
float64 restatement of compute.glsl, on the RNG-free scenes of
tests/shading_scenes.py (DESIGN.md "Shading model").  No GPU and no reference
tree is needed.

  - premises: the model's signatures show every branch of the scene table
    reached (they fail, never skip, when a scene stops exercising a branch);
  - every scene under the comparison rule of shading_model.assert_image, in
    brute mode, `composite` through the BVH walk too;
  - the 8-bit accumulator of the emissive ramp.
"""
import numpy as np
import pytest

import shading_model as sm
import shading_scenes as ss

SCENES = ss.all_scenes()
COMPOSITES = ["composite", "composite/n1217", "composite/n8193"]


def to_uniforms(rt2mod, un):
    u = rt2mod.Uniforms()
    for k, v in un.items():
        setattr(u, k, rt2mod.Vec4(*v, 0.0) if isinstance(v, tuple) else v)
    return u


def scene_data(rt2mod, scene):
    """The scene as a SceneData with its BVH built (triangles() is then in the BVH's order)."""
    sd = rt2mod.SceneData()
    for m in scene["materials"]:
        sd.add_material(rt2mod.Material.from_buffer_copy(m.tobytes()))
    sd.add_triangles(scene["triangles"])
    sd.build_bvh()
    return sd


def bound_textures(scene):
    return [t for t in scene["textures"] if t is not None]


def oracle_image(oraclemod, rt2mod, scene, mode="brute", with_acc8=False):
    """-> (mean image (H, W, 3), acc8 or None, segments)."""
    u = to_uniforms(rt2mod, scene["uniforms"])
    tris, mats, nodes = scene["triangles"], scene["materials"], None
    if mode == "bvh":
        sd = scene_data(rt2mod, scene)
        tris, nodes = sd.triangles(), sd.nodes()
    first, count = scene["frames"]
    oraclemod.set_textures(bound_textures(scene))
    try:
        acc, acc8, segs, _ = oraclemod.render(tris, mats, u, np.arange(u.height, dtype=np.int32), first, count, mode,
                                              nodes=nodes, with_acc8=with_acc8)
    finally:
        oraclemod.set_textures([])
    return acc[..., :3] / np.float32(count), acc8, segs


def texture_classes(model):
    """The per-texture signature classes of the `textures` scene."""
    out = {}
    for index, (w, h) in ss.TEXTURE_SHAPES.items():
        for k, mask in model.texture_class(index, w, h).items():
            out[f"texture{index}_{k}"] = mask
    return out


def expected_segments(scene, model):
    return int(model.segments.sum()) * scene["uniforms"]["numRaysPerPixel"] * scene["frames"][1]


# --- premises -----------------------------------------------------------------------

PREMISES = [
    ("sky_below_horizon", "sky_horizon"), ("sky_sun_side", "sky_sun"), ("sky_sun_side", "sky_horizon"),
    ("sky_opposite_side", "sky_horizon"), ("sky_opposite_side", "sky_up"),
    ("glass_refracted_in", "glass_slab/b12"), ("glass_toggled_back", "glass_slab/b12"),
    ("glass_total_internal_reflection", "glass_tir/b12"), ("glass_entry_reflection", "glass_low_index/b12"),
    ("glass_refracted_in", "glass_low_index/b12"),
    ("cut_at_limit_1", "glass_slab/b1"), ("cut_at_limit_2", "glass_slab/b2"), ("cut_at_limit_3", "glass_slab/b3"),
    ("cut_at_limit_1", "glass_tir/b1"), ("cut_at_limit_1", "glass_low_index/b1"),
    ("edge_pass_through", "edge_highlight_mirror"),
    ("checker_black", "checker/s0.75"), ("checker_white", "checker/s0.75"), ("checker_black", "checker/s8"),
    ("checker_white", "checker/s8"), ("checker_guard", "checker/s0"), ("checker_guard", "checker/s-1"),
    ("texel_negative_column", "textures"), ("texel_negative_row", "textures"),
    ("texture0_column_wrap", "textures"), ("texture0_row_wrap", "textures"), ("texture1_column_wrap", "textures"),
    ("texture1_sampled", "textures"), ("texture2_sampled", "textures"), ("texture3_sampled", "textures"),
    ("texture_rule_negative", "textures"), ("texture_rule_beyond", "textures"), ("texture_rule_magenta", "textures"),
    ("texture_rule_unbound", "textures"),
    ("glass_toggled_back", "composite"), ("checker_black", "composite"), ("checker_white", "composite"),
    ("texture0_sampled", "composite"),
]


@pytest.mark.parametrize("cls,name", PREMISES, ids=[f"{c}-{n}" for c, n in PREMISES])
def test_premise_branch_is_reached(cls, name):
    model = sm.model_for(SCENES[name])
    classes = model.classes()
    classes.update(texture_classes(model))
    n = int((classes[cls] & ~model.excluded).sum())
    assert n >= 20, f"{name}: only {n} compared pixels take the branch {cls}"


def test_premise_edge_highlight_scenes():
    """Through the mirror the marked quad is passed at bounce 2 and the light
    behind it arrives unattenuated; seen directly it attenuates and scatters."""
    m = sm.model_for(SCENES["edge_highlight_mirror"])
    passed = m.any_bounce(sm.F_BRANCH, sm.BR_PASS) & ~m.excluded
    assert (m.signature[passed][:, 1, sm.F_BRANCH] == sm.BR_PASS).all()
    assert (m.signature[passed][:, 2, sm.F_END] == sm.END_LIGHT).all()
    d = sm.model_for(SCENES["edge_highlight_direct"])
    direct = (d.signature[:, :, 0, sm.F_BRANCH] == sm.DIFFUSE) & ~d.excluded
    assert direct.sum() >= 20 and not d.any_bounce(sm.F_BRANCH, sm.BR_PASS).any()
    assert (d.signature[direct][:, 1, sm.F_END] == sm.END_SCATTER).all()


def test_premise_glass_face_is_hit_three_times():
    """The re-hits at about 1e-3 and 1e-6 of the first distance: three bounces
    on one face, insideGlass true, false, true."""
    m = sm.model_for(SCENES["glass_slab/b12"])
    s = m.signature[~m.excluded & (m.signature[:, :, 0, sm.F_BRANCH] == sm.GLASS)]
    assert len(s) >= 20
    assert (s[:, 0, sm.F_TRI] == s[:, 1, sm.F_TRI]).all() and (s[:, 1, sm.F_TRI] == s[:, 2, sm.F_TRI]).all()
    assert (s[:, :3, sm.F_INSIDE] == (1, 0, 1)).all() and (s[:, 3, sm.F_TRI] != s[:, 2, sm.F_TRI]).all()


def test_premise_ramp_rows():
    """Every strength of the ramp fills at least one whole row of pixels."""
    for r in (1, 3, 4):
        scene = SCENES[f"emissive_ramp/r{r}"]
        m = sm.model_for(scene)
        first = m.signature[:, :, 0, sm.F_TRI]
        mat = np.where(first >= 0, scene["triangles"]["materialIndex"][np.maximum(first, 0)], -1)
        for k, strength in enumerate(ss.RAMP_STRENGTHS):
            rows = ((mat == k) & ~m.excluded).all(1)
            assert rows.any(), f"strength {strength:g} fills no row"
            assert scene["materials"]["emissionStrength"][k] == np.float32(strength)


def test_model_refuses_random_paths():
    """A scene cannot slip a random walk through."""
    def one_quad(**material):
        b = ss._Builder()
        kind = material.pop("kind")
        ss._pixel_rect(b, -3.0, 8, 6, -1, 9, -1, 7, b.material(kind, **material))
        return b
    cases = {
        "diffuse under the sky": one_quad(kind=ss.DIFFUSE, color=(1.0, 0.5, 0.5)).scene("x", 8, 6, 4, 1, True),
        "survival 0.5": one_quad(kind=ss.GLASS, color=(0.5, 0.4, 0.3), ior=1.5).scene("x", 8, 6, 4, 1, True),
        "half specular": one_quad(kind=ss.SPECULAR, smooth=1.0, prob=0.5).scene("x", 8, 6, 4, 1, True),
    }
    b = one_quad(kind=ss.DIFFUSE, color=(1.0, 0.5, 0.5))
    b.box(10.0, b.light(*ss.BOX_EMISSION))
    b.quad((-1, -1, 5), (2, 0, 0), (0, -2, 0), b.light((1, 1, 1), 2.0))  # a second emitter the scatter can reach
    cases["two emitters"] = b.scene("x", 8, 6, 4, 1, False)
    jitter = one_quad(kind=ss.LIGHT, emission=(1, 1, 1), strength=1.0).scene("x", 8, 6, 4, 1, True)
    jitter["uniforms"]["pixelRight"] = (0.01, 0.0, 0.0)
    cases["jitter"] = jitter
    for what, scene in cases.items():
        with pytest.raises(sm.NotDeterministic):
            sm.Model(scene)
            pytest.fail(f"{what}: accepted")


def test_texture_unpack_rules():
    """gl_texels against hand-written rows: 7 x 2 RGB is read with 24-byte rows
    and zeros past the buffer; two channels give r, g, 0; one gives r, r, r."""
    img = np.arange(42, dtype=np.uint8).reshape(2, 7, 3)
    t = sm.gl_texels(img) * 255.0
    assert np.array_equal(t[0].reshape(-1), np.arange(21))
    assert np.array_equal(t[1].reshape(-1), np.concatenate([np.arange(24, 42), np.zeros(3)]))
    assert np.array_equal(sm.gl_texels(np.array([[[10, 20]]], np.uint8))[0, 0] * 255.0, (10, 20, 0))
    assert np.array_equal(sm.gl_texels(np.array([[[7]]], np.uint8))[0, 0] * 255.0, (7, 7, 7))


# --- oracle vs model ---------------------------------------------------------------------

MEASURED = {}  # scene -> (max error over the compared pixels, excluded fraction), printed with -s


@pytest.mark.parametrize("name", sorted(SCENES))
def test_oracle_matches_model(rt2mod, oraclemod, name):
    scene = SCENES[name]
    model = sm.model_for(scene)
    frac = sm.assert_exclusions(model, texture_classes(model))
    img, _, segs = oracle_image(oraclemod, rt2mod, scene)
    worst = sm.assert_image(model, img, "oracle, brute")
    MEASURED[name] = (worst, frac)
    print(f"{name}: max error {worst:.2e}, largest bound {model.bound[~model.excluded].max():.2e}, excluded {frac:.2%}")
    if not model.excluded.any():
        assert segs == expected_segments(scene, model)


@pytest.mark.parametrize("name", COMPOSITES)
def test_oracle_bvh_matches_model(rt2mod, oraclemod, name):
    scene = SCENES[name]
    model = sm.model_for(scene)
    img, _, segs = oracle_image(oraclemod, rt2mod, scene, "bvh")
    sm.assert_image(model, img, "oracle, bvh")
    if not model.excluded.any():
        assert segs == expected_segments(scene, model)


def expected_acc8(model, frames):
    """(acc8 the model predicts, mask of the channels where it is decided):
    floor(clamp(value) * 255 + 0.5) per frame, wherever the value is further
    than the pixel's bound from a rounding step."""
    q = np.clip(model.value, 0.0, 1.0) * 255.0 + 0.5
    decided = np.abs(q - np.round(q)) > model.bound[..., None] * 255.0
    decided &= ~model.excluded[..., None]
    return np.floor(q).astype(np.uint32) * np.uint32(frames), decided


@pytest.mark.parametrize("rays", [1, 3, 4])
def test_ramp_8bit_accumulator(rt2mod, oraclemod, rays):
    scene = SCENES[f"emissive_ramp/r{rays}"]
    model = sm.model_for(scene)
    _, acc8, _ = oracle_image(oraclemod, rt2mod, scene, with_acc8=True)
    want, decided = expected_acc8(model, scene["frames"][1])
    assert decided.mean() > 0.9
    assert np.array_equal(acc8[..., :3][decided], want[decided])
    assert (acc8[..., 3] == scene["frames"][1]).all()
    assert len(np.unique(want[decided])) >= 24  # 16 strengths x 3 channels, less the saturated ends
