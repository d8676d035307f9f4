"""The short reciprocal rcp_variant(x, 3) of rt2_math.h (v_rcp_f32 + 5 FMA)
against IEEE 1.0f / x on the device, over EVERY float bit pattern of the two
ranges a guarded use in the render path would admit:

  [1e-10, 2^100]  det in mt_exact and texture_color (rt2_sweep.h, rt2_path.h)
  [2^-24, 1]      pr in shade's Russian roulette (rt2_path.h)

Bar: 0 mismatches.  This is the exhaustive check rt2_math.h cites.  (The
render path itself keeps the IEEE division there: the guarded short form was
measured slower, DESIGN.md "Tried and measured".)
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _bits(x) -> int:
    return int(np.float32(x).view(np.uint32))


RANGES = {
    "det": (np.float32(1e-10), np.float32(2.0 ** 100)),
    "pr": (np.float32(2.0 ** -24), np.float32(1.0)),
}


@pytest.mark.parametrize("name", list(RANGES))
def test_rcp_variant3_is_ieee_on_every_pattern(rt2mod, name):
    lo, hi = RANGES[name]
    blo, bhi = _bits(lo), _bits(hi)
    assert blo < bhi  # positive floats: bit order is value order
    mism = C.c_ulonglong(12345)
    first = C.c_uint32(0)
    rc = rt2mod.lib().rt2_device_rcp_check(blo, bhi, 3, C.byref(mism), C.byref(first))
    assert rc == 0
    n = bhi - blo + 1
    print(f"{name}: {n} patterns [{lo!r}, {hi!r}], {mism.value} mismatches")
    assert mism.value == 0, f"{name}: {mism.value} of {n} patterns differ, first 0x{first.value:08x}"


def test_check_sees_a_wrong_reciprocal(rt2mod):
    """The bare v_rcp_f32 (variant 0, <= 1 ulp) is not IEEE: the check must count its misses."""
    mism = C.c_ulonglong(0)
    first = C.c_uint32(0)
    blo, bhi = _bits(1.0), _bits(2.0)
    assert rt2mod.lib().rt2_device_rcp_check(blo, bhi, 0, C.byref(mism), C.byref(first)) == 0
    assert 0 < mism.value < bhi - blo + 1
    assert blo <= first.value <= bhi
