"""The HIP kernels' random paths on the scenes of tests/random_scenes.py: every
image meets the comparison rule of tests/random_path_model.py against the
float64 model that carries the shader's draw stream (not only the oracle),
equals the CPU oracle's bit for bit, and traces the oracle's number of
segments (the model's, where the rule excludes no pixel).  Each scene runs on
the automatic kernel, the scalar kernel (variant 136) and the BVH traversal.
One scene is also rendered as a slab of rows from a first frame other than 0,
with and without the frame split: the global row and the first frame in the
seed.
"""
import numpy as np
import pytest

import random_path_model as rm
from test_gpu_parity import _last_variant, assert_exact
from test_random_paths import SCENES, oracle_image
from test_shading_model import bound_textures, scene_data, to_uniforms

pytestmark = pytest.mark.gpu
SCALAR = 136


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return torch


_refs = {}


def _oracle(oraclemod, rt2mod, scene, mode, rows=None):
    """One oracle image per (scene, traversal, rows), shared by the tests and left unchanged."""
    key = (scene["name"], mode, None if rows is None else tuple(rows))
    if key not in _refs:
        img, segs = oracle_image(oraclemod, rt2mod, scene, mode, rows)
        img.setflags(write=False)
        _refs[key] = (img, segs)
    return _refs[key]


def _render(rt2mod, scene, how, shard=None, frame_split=None):
    """-> (the mean image, segments, the kernel's name)."""
    gpu = rt2mod.Scene(scene_data(rt2mod, scene), 0)
    if how == "bvh":
        gpu.set_traversal("bvh")
    elif how == "scalar":
        gpu.set_variant(SCALAR)
    if frame_split is not None:
        gpu.set_frame_split(frame_split)
    gpu.set_textures(bound_textures(scene))
    first, count = scene["frames"]
    u = to_uniforms(rt2mod, scene["uniforms"])
    out = gpu.render_host(u, first, count) if shard is None else gpu.render_host(u, first, count, shard)
    return out, gpu.stats(reset=True).segments, _last_variant(rt2mod, gpu)


@pytest.mark.parametrize("how", ["auto", "scalar", "bvh"])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_kernel_matches_model_and_oracle(rt2mod, oraclemod, torch_cuda, name, how):
    scene = SCENES[name]
    model = rm.model_for(scene)
    img, segs, kernel = _render(rt2mod, scene, how)
    ref, ref_segs = _oracle(oraclemod, rt2mod, scene, "bvh" if how == "bvh" else "brute")
    oracle_worst = float(np.where(model.excluded, 0.0, np.abs(ref.astype(np.float64) - model.value).max(-1)).max())
    worst = rm.assert_image(model, img, f"GPU, {how}")
    print(f"{name} {how} [{kernel}]: max error {worst:.2e} (oracle {oracle_worst:.2e}), largest bound "
          f"{model.bound[~model.excluded].max():.2e}")
    assert_exact(img, ref, f"{name} {how}")
    assert segs == ref_segs
    if not model.excluded.any():
        assert segs == int(model.segments.sum())


@pytest.mark.parametrize("frame_split", [False, True])
def test_slab_from_frame_5(rt2mod, oraclemod, torch_cuda, frame_split):
    """Rows of the second of three ranks, tiles of 2 rows, frames 5, 6, 7:
    the seed takes the row's number in the whole image and first frame +
    frame."""
    scene = SCENES["diffuse_floor/b3"]
    assert scene["frames"] == (5, 3)
    model = rm.model_for(scene)
    sh = rt2mod.shard(2, 1, 3)
    rows = rt2mod.shard_row_ids(scene["uniforms"]["height"], sh)
    assert 0 < len(rows) < scene["uniforms"]["height"] and rows[0] != 0
    img, segs, kernel = _render(rt2mod, scene, "auto", sh, frame_split)
    worst = rm.assert_image(model, img, f"GPU, slab, frame split {frame_split}", rows)
    print(f"slab rows {rows.tolist()} [{kernel}] frame split {frame_split}: max error {worst:.2e}")
    ref, ref_segs = _oracle(oraclemod, rt2mod, scene, "brute", rows)
    assert_exact(img, ref, f"slab, frame split {frame_split}")
    assert segs == ref_segs
    if not model.excluded[rows].any():
        assert segs == int(model.segments[:, rows].sum())
