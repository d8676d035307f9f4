"""The pinned arithmetic of DESIGN.md §Numerics on the device: every operation
of rt2_device_numerics (numerics_kernel: the functions of rt2_math.h and
rt2_pinned_math.h that the render and query kernels call, compiled in their
translation unit with their flags) on the input sets of
tests/numerics_cases.py, one launch per operation.

The device equals the oracle (oracle_numerics) in every bit, any NaN equal to
any NaN, and it is held to what the oracle is held to in
tests/test_numerics_cases.py: the exact reference in every bit for the IEEE
operations and the composed forms, the documented bounds for the
transcendentals.  rt2_resolve_tonemap and the 8-bit resolve are checked through
their public entry points.  Every input is a plain float.
"""
import numpy as np
import pytest

import numerics_cases as N

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch  # loads torch's HIP runtime first: librt2 then shares it
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.cuda.set_device(0)
    return torch


_out = {}


def _device(rt2mod):
    """One launch per operation: the result is kept for the tests that share it."""
    def run(op, rows):
        key = (op, rows.shape, rows.ctypes.data if not rows.flags.writeable else None)
        if key[2] is None:
            return rt2mod.device_numerics(op, rows)
        if key not in _out:
            _out[key] = rt2mod.device_numerics(op, rows)
        return _out[key]
    return run


def _oracle(oraclemod):
    return lambda op, rows: oraclemod.numerics(op, rows)


@pytest.mark.parametrize("op", N.ALL_OPS)
def test_device_equals_the_oracle(rt2mod, oraclemod, torch_cuda, op):
    rows = N.inputs(op)
    dev, host = _device(rt2mod)(op, rows), oraclemod.numerics(op, rows)
    bad = N.mismatches(op, dev, host)
    assert len(bad) == 0, (f"{op}: {len(bad)} of {len(rows)} rows differ; row {bad[0]}: in "
                           f"{[hex(x) for x in rows[bad[0]]]} device {[hex(x) for x in dev[bad[0]]]} "
                           f"oracle {[hex(x) for x in host[bad[0]]]}")


@pytest.mark.parametrize("op", N.ALL_OPS)
def test_device_against_the_reference(rt2mod, torch_cuda, op):
    failure, measured = N.check_op(op, _device(rt2mod))
    if measured is not None:
        print(f"\n{op}: measured maximum {measured:.4g}")
    assert failure is None, failure


def test_opposite_zeros(rt2mod, oraclemod, torch_cuda):
    """max(+0, -0) = +0 and min(+0, -0) = -0 in either
    order, on the device's fmaxf / fminf as in the header's explicit host form."""
    z = np.array([[N.PZERO, N.NZERO], [N.NZERO, N.PZERO], [N.PZERO, N.PZERO], [N.NZERO, N.NZERO]], np.uint32)
    for op, want in (("fmax", [N.PZERO, N.PZERO, N.PZERO, N.NZERO]), ("fmin", [N.NZERO, N.NZERO, N.PZERO, N.NZERO])):
        assert rt2mod.device_numerics(op, z)[:, 0].tolist() == want, op
        assert oraclemod.numerics(op, z)[:, 0].tolist() == want, op
    rows = np.array([[N.NZERO, N.PZERO, N.ONE], [N.PZERO, N.NZERO, N.ONE], [N.NZERO, N.bits(-1.0), N.PZERO]], np.uint32)
    assert rt2mod.device_numerics("clamp", rows)[:, 0].tolist() == [N.PZERO, N.PZERO, N.NZERO]
    nan = np.array([[N.QNAN, N.ONE], [N.ONE, N.QNAN]], np.uint32)
    assert (rt2mod.device_numerics("fmax", nan)[:, 0] == N.ONE).all()
    assert (rt2mod.device_numerics("fmin", nan)[:, 0] == N.ONE).all()


@pytest.mark.parametrize("frames", [1, 3])
def test_resolve_tonemap(rt2mod, oraclemod, torch_cuda, frames):
    """rt2_resolve_tonemap on a caller's own sums, out-of-range ones included:
    the oracle's srgb1(aces1(sum / frames)) in every bit, alpha 1; the exact
    aces1 under it, pow's bound above it, and include/rt2.h's out-of-range
    values."""
    torch = torch_cuda
    x = N.inputs("aces1")[:, 0]
    n = len(x)
    lin = np.zeros((n, 4), np.uint32)
    lin[:, 0], lin[:, 1], lin[:, 2], lin[:, 3] = x, x[::-1], np.roll(x, 7), N.QNAN     # alpha is not read
    d = torch.from_numpy(lin.view(np.float32).copy()).cuda()
    out = torch.empty_like(d)
    rt2mod.resolve_tonemap(d.data_ptr(), n, frames, out.data_ptr(), 0)
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    assert (got[:, 3] == N.ONE).all()
    fr = np.full(n, N.bits(float(frames)), np.uint32)
    for ch, col in enumerate((x, x[::-1], np.roll(x, 7))):
        mean = oraclemod.numerics("div", np.stack([col, fr], 1))[:, :1]
        tone = oraclemod.numerics("aces1", mean)[:, :1]
        want = oraclemod.numerics("srgb1", tone)[:, :1]
        assert len(N.mismatches("srgb1", got[:, ch:ch + 1], want)) == 0, ch
    # channel 0 against the exact reference: aces1 of the exact mean, then pow within its bound
    tone = [N.aces1(N.f_div(int(u), N.bits(float(frames)))) for u in x]
    true = np.array([N.val(t) for t in tone]) ** N.val(N.SRGB_EXPONENT)
    err = np.abs(N.f64(got[:, 0]) - true)
    print(f"\nresolve_tonemap, frames {frames}: max |error| {err.max():.3e}")
    assert err.max() <= 1e-6
    # in place, and the documented values out of range
    rt2mod.resolve_tonemap(d.data_ptr(), n, frames, d.data_ptr(), 0)
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy().view(np.uint32), got)
    by_input = dict(zip(x.tolist(), got[:, 0].tolist()))
    for u in (N.QNAN, N.INF, N.NINF, N.MAX_FIN, N.MAX_FIN | N.SIGN, N.NZERO, N.PZERO):
        assert by_input[u] == N.PZERO, hex(u)
    assert by_input[N.bits(1e6)] == N.ONE and by_input[N.bits(-1e6)] == N.ONE


@pytest.mark.parametrize("frames", [1, 3])
def test_resolve_rgb8(rt2mod, oraclemod, config_scene, torch_cuda, frames):
    """The 8-bit resolve of a blocking render: u8(min(255, float(sum) / frames))
    of the oracle's unorm8 sums, by rt2_resolve_rgb8_reference and by the exact
    division."""
    sd, spec = config_scene("A")
    u = rt2mod.offline_uniforms(48, 32, spec.bounces, 2, sd.num_triangles)
    _, out8 = rt2mod.Scene(sd, 0).render_host(u, 5, frames, rgb8=True)
    _, acc8, _, _ = oraclemod.render(sd.triangles(), sd.materials(), u, np.arange(u.height, dtype=np.int32), 5, frames,
                                     "brute", with_acc8=True)
    assert np.array_equal(out8, rt2mod.resolve_rgb8_reference(acc8, frames))
    exact = [min(255, int(N.val(N.f_div(N.f_from_uint(int(q)), N.bits(float(frames))))))
             for q in acc8[..., :3].reshape(-1)]
    assert np.array_equal(out8.reshape(-1), np.array(exact, np.uint8))
    assert out8.min() < 64 and out8.max() > 128          # not a flat image
