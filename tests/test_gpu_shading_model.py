"""The HIP kernels' shade() on the RNG-free scenes of tests/shading_scenes.py:
every image meets the comparison rule of tests/shading_model.py against the
independent float64 model (not only the oracle), equals the CPU oracle's bit
for bit, and traces the number of segments the model's path lengths give.
Each scene runs on the automatic kernel, the scalar kernel (variant 136) and
the BVH traversal; `composite` also at the paddings that select the resident
kernel's L2 continuation and the tile-stream kernel.
"""
import numpy as np
import pytest

import shading_model as sm
from test_gpu_parity import AUTO_RES_L2, AUTO_RES_L2_SLAB, AUTO_TILES, _last_variant, assert_exact
from test_shading_model import (SCENES, bound_textures, expected_acc8, expected_segments, oracle_image, scene_data,
                                to_uniforms)

pytestmark = pytest.mark.gpu
SCALAR = 136


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return torch


_refs = {}


def _oracle(oraclemod, rt2mod, scene, mode):
    """One oracle image per (scene, traversal), shared by the tests and left unchanged."""
    key = (scene["name"], mode)
    if key not in _refs:
        img, _, segs = oracle_image(oraclemod, rt2mod, scene, mode)
        img.setflags(write=False)
        _refs[key] = (img, segs)
    return _refs[key]


def _render(rt2mod, scene, how, rgb8=False):
    """-> (render_host's result, segments, the kernel's name)."""
    gpu = rt2mod.Scene(scene_data(rt2mod, scene), 0)
    if how == "bvh":
        gpu.set_traversal("bvh")
    elif how == "scalar":
        gpu.set_variant(SCALAR)
    gpu.set_textures(bound_textures(scene))
    first, count = scene["frames"]
    out = gpu.render_host(to_uniforms(rt2mod, scene["uniforms"]), first, count, rgb8=rgb8)
    return out, gpu.stats(reset=True).segments, _last_variant(rt2mod, gpu)


@pytest.mark.parametrize("how", ["auto", "scalar", "bvh"])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_kernel_matches_model_and_oracle(rt2mod, oraclemod, torch_cuda, name, how):
    scene = SCENES[name]
    model = sm.model_for(scene)
    img, segs, kernel = _render(rt2mod, scene, how)
    worst = sm.assert_image(model, img, f"GPU, {how}")
    print(f"{name} {how} [{kernel}]: max error {worst:.2e}, largest bound {model.bound[~model.excluded].max():.2e}")
    ref, ref_segs = _oracle(oraclemod, rt2mod, scene, "bvh" if how == "bvh" else "brute")
    assert_exact(img, ref, f"{name} {how}")
    assert segs == ref_segs
    if not model.excluded.any():
        assert segs == expected_segments(scene, model)
    if how == "auto" and name == "composite/n1217":
        assert kernel in (AUTO_RES_L2, AUTO_RES_L2_SLAB)
    if how == "auto" and name == "composite/n8193":
        assert kernel == AUTO_TILES


@pytest.mark.parametrize("rays", [1, 3, 4])
def test_ramp_8bit_average(rt2mod, torch_cuda, rays):
    """The 8-bit accumulator on the GPU: the average over the frames is
    floor(clamp(value) * 255 + 0.5) wherever the model decides the rounding."""
    scene = SCENES[f"emissive_ramp/r{rays}"]
    model = sm.model_for(scene)
    (img, rgb8), _, _ = _render(rt2mod, scene, "auto", rgb8=True)
    sm.assert_image(model, img, "GPU, rgb8 render")
    want, decided = expected_acc8(model, 1)
    assert decided.mean() > 0.9
    assert np.array_equal(rgb8[decided], want[decided].astype(np.uint8))
