"""rnd_dir (rt2_math.h) accepts a candidate on dot(p, p) < 1 instead of the
reference's length(p) = sqrt(dot(p, p)) < 1.  The two agree for every binary32
s >= 0 because the correctly rounded square root is monotone, sqrt(1) = 1 and
sqrt(1 - 2^-24) rounds below 1.  Checked here on every float of [0.25, 4) (2^25
patterns around the threshold) and on zero, denormals, the largest finite
float and infinity.  numpy's float32 sqrt is the IEEE correctly rounded one,
as is the device's (-fhip-fp32-correctly-rounded-divide-sqrt)."""
import numpy as np


def _agree(s):
    assert s.dtype == np.float32
    r = np.sqrt(s)
    assert r.dtype == np.float32
    return np.array_equal(r < np.float32(1.0), s < np.float32(1.0))


def test_every_float_of_quarter_to_four():
    lo, hi = np.float32(0.25).view(np.uint32), np.float32(4.0).view(np.uint32)
    assert int(hi) - int(lo) == 2 ** 25
    one = int(np.float32(1.0).view(np.uint32))
    step = 2 ** 22
    for b in range(int(lo), int(hi), step):
        s = np.arange(b, b + step, dtype=np.uint32).view(np.float32)
        assert _agree(s), f"mismatch in patterns [0x{b:08x}, 0x{b + step:08x})"
        # the split is at 1.0 exactly: every s below it is accepted, none from it on
        assert np.array_equal(s < np.float32(1.0), np.arange(b, b + step, dtype=np.int64) < one)


def test_edge_values():
    tiny = np.array([0, 1, 2, 0x007FFFFF, 0x00800000], np.uint32).view(np.float32)  # +0, denormals, smallest normal
    s = np.concatenate([tiny, np.float32([np.finfo(np.float32).max, np.inf, 1.0, np.nextafter(np.float32(1), np.float32(0)),
                                          np.nextafter(np.float32(1), np.float32(2))])]).astype(np.float32)
    assert _agree(s)
    assert np.sqrt(np.nextafter(np.float32(1), np.float32(0))) < np.float32(1.0)
    assert np.sqrt(np.float32(1.0)) == np.float32(1.0)
