"""Inputs and an independent reference for the pinned arithmetic of DESIGN.md
§Numerics (tests/test_numerics_cases.py on the CPU oracle,
tests/test_gpu_numerics.py on the device).

The reference shares no code and no arithmetic with the oracle or the kernels:

- `round_fraction` rounds an exact rational to binary32, ties to even, with
  denormals, overflow and signed zero; `f_add`, `f_sub`, `f_mul`, `f_div`,
  `f_fma` apply it to the exact result of the operation on two or three bit
  patterns, and `f_sqrt` to `math.isqrt` of the scaled operand plus a sticky
  bit.  Plain Python integers throughout: no numpy float32, no C.
- the composed forms (`dot`, `cross`, `normalize`, `reflect`, `mix`,
  `smoothstep`, `clamp`, `refract_`, `aces1`, `rnd`, `rnd_dir`) are written
  from the text of DESIGN.md §Numerics and the GLSL 4.30 definitions on top of
  those operations — a second reading, in the manner of tests/shading_model.py.
- the transcendentals are measured against float64 libm, the error in ulps of
  the true value (2^-149 is the ulp below 2^-126); `sky` takes its acos and exp
  from float64 libm at the binary32 operands and everything else exactly, and
  carries the bound derived at `SKY_ABS_TOL`.

Everything is moved as binary32 bit patterns (Python ints, numpy uint32
arrays), so that NaNs, zero signs and RNG states survive.  A row has up to 9
operand words; vectors take words 0-2 and 3-5, a trailing scalar word 6.
"""
import math
import struct
from fractions import Fraction

import numpy as np

SIGN = 0x80000000
PZERO, NZERO = 0x00000000, 0x80000000
INF, NINF, QNAN = 0x7F800000, 0xFF800000, 0x7FC00000
ONE, TWO, HALF, THREE = 0x3F800000, 0x40000000, 0x3F000000, 0x40400000
MIN_DEN, MAX_DEN, MIN_NORM, MAX_FIN = 0x00000001, 0x007FFFFF, 0x00800000, 0x7F7FFFFF


# ---------------------------------------------------------------------------
# bit patterns
# ---------------------------------------------------------------------------
def bits(x: float) -> int:
    """The binary32 nearest to a Python float (struct rounds ties to even);
    used for constants written in decimal, as a C compiler rounds a literal."""
    try:
        return struct.unpack("<I", struct.pack("<f", x))[0]
    except OverflowError:
        return NINF if x < 0 else INF


def val(u: int) -> float:
    """The value of a bit pattern (float64 holds every binary32 exactly)."""
    return struct.unpack("<f", struct.pack("<I", u))[0]


def is_nan(u: int) -> bool:
    return (u & 0x7FFFFFFF) > INF


def is_inf(u: int) -> bool:
    return (u & 0x7FFFFFFF) == INF


def is_zero(u: int) -> bool:
    return (u & 0x7FFFFFFF) == 0


def dec(u: int):
    """(m, e) of a finite bit pattern: its value is m * 2^e, m a signed integer."""
    ex, fr = (u >> 23) & 0xFF, u & 0x7FFFFF
    m, e = (fr, -149) if ex == 0 else (fr | 0x800000, ex - 150)
    return (-m if u & SIGN else m), e


def neg(u: int) -> int:
    return u ^ SIGN


def lt(a: int, b: int) -> bool:
    """a < b as IEEE compares (false with a NaN; -0 == +0)."""
    if is_nan(a) or is_nan(b):
        return False
    return val(a) < val(b)


# ---------------------------------------------------------------------------
# the exact rounding
# ---------------------------------------------------------------------------
def _rn(sign: int, num: int, den: int) -> int:
    """num / den > 0 (integers) to the nearest binary32, ties to even, with the
    sign bit `sign` (0 or SIGN)."""
    e = num.bit_length() - den.bit_length()          # floor(log2(num / den)) or one more
    if (num << max(-e, 0)) < (den << max(e, 0)):
        e -= 1
    q = max(e, -126) - 23                            # the exponent of the last kept bit
    n2, d2 = (num, den << q) if q >= 0 else (num << -q, den)
    k, r = divmod(n2, d2)
    if 2 * r > d2 or (2 * r == d2 and (k & 1)):
        k += 1
    # k < 2^23 only for q = -149 (a denormal); k = 2^24 carries into the exponent
    u = k if k < 0x800000 else ((q + 150) << 23) + (k - 0x800000)
    return sign | (INF if u >= INF else u)


def round_fraction(x: Fraction, zero_sign: int = 0) -> int:
    """A rational to binary32, ties to even; an exact zero takes zero_sign."""
    if x == 0:
        return zero_sign
    return _rn(SIGN if x < 0 else 0, abs(x.numerator), x.denominator)


def _rn_dyadic(m: int, e: int, zero_sign: int) -> int:
    """m * 2^e (m signed) to binary32."""
    if m == 0:
        return zero_sign
    s, m = (SIGN, -m) if m < 0 else (0, m)
    return _rn(s, m << e, 1) if e >= 0 else _rn(s, m, 1 << -e)


def f_mul(a: int, b: int) -> int:
    if is_nan(a) or is_nan(b):
        return QNAN
    s = (a ^ b) & SIGN
    if is_inf(a) or is_inf(b):
        return QNAN if is_zero(a) or is_zero(b) else s | INF
    (ma, ea), (mb, eb) = dec(a), dec(b)
    return _rn_dyadic(abs(ma * mb), ea + eb, 0) | s


def f_fma(a: int, b: int, c: int) -> int:
    """a * b + c with one rounding."""
    if is_nan(a) or is_nan(b) or is_nan(c):
        return QNAN
    sp = (a ^ b) & SIGN
    if is_inf(a) or is_inf(b):
        if is_zero(a) or is_zero(b) or (is_inf(c) and (c & SIGN) != sp):
            return QNAN
        return sp | INF
    if is_inf(c):
        return c
    (ma, ea), (mb, eb), (mc, ec) = dec(a), dec(b), dec(c)
    mp, ep = ma * mb, ea + eb
    e = min(ep, ec)
    # an exact zero sum: the common sign of two zeros, +0 otherwise (round to nearest)
    return _rn_dyadic((mp << (ep - e)) + (mc << (ec - e)), e, sp if sp == (c & SIGN) else 0)


def f_add(a: int, b: int) -> int:
    return f_fma(a, ONE, b)       # a * 1 is exact, signs included


def f_sub(a: int, b: int) -> int:
    return f_add(a, QNAN if is_nan(b) else neg(b))


def f_div(a: int, b: int) -> int:
    if is_nan(a) or is_nan(b):
        return QNAN
    s = (a ^ b) & SIGN
    if is_inf(a):
        return QNAN if is_inf(b) else s | INF
    if is_inf(b):
        return s
    if is_zero(b):
        return QNAN if is_zero(a) else s | INF
    if is_zero(a):
        return s
    (ma, ea), (mb, eb) = dec(a), dec(b)
    d = ea - eb
    return _rn(s, abs(ma) << max(d, 0), abs(mb) << max(-d, 0))


def f_sqrt(a: int) -> int:
    if is_nan(a) or a == NZERO or a == PZERO or a == INF:
        return QNAN if is_nan(a) else a
    if a & SIGN:
        return QNAN
    m, e = dec(a)
    k = 64 + ((e - 64) & 1)                    # e - k even; m << k has more than 64 bits
    n = m << k
    r = math.isqrt(n)                          # more than 32 bits: the half bit lies inside r
    return _rn_dyadic(2 * r + (r * r != n), (e - k) // 2 - 1, 0)   # the sticky bit below it


def f_from_uint(r: int) -> int:
    """(float)r for an unsigned integer r."""
    return _rn_dyadic(r, 0, 0)


# ---------------------------------------------------------------------------
# min / max / clamp as the pinned header defines them:
# IEEE 754-2019 minimumNumber / maximumNumber — a NaN operand is ignored,
# -0 < +0.
# ---------------------------------------------------------------------------
def f_max(a: int, b: int) -> int:
    if is_nan(a):
        return QNAN if is_nan(b) else b
    if is_nan(b):
        return a
    if is_zero(a) and is_zero(b):
        return a & b
    return b if lt(a, b) else a


def f_min(a: int, b: int) -> int:
    if is_nan(a):
        return QNAN if is_nan(b) else b
    if is_nan(b):
        return a
    if is_zero(a) and is_zero(b):
        return a | b
    return b if lt(b, a) else a


def clamp(x: int, lo: int, hi: int) -> int:
    return f_min(f_max(x, lo), hi)          # GLSL 4.30 §8.3: min(max(x, minVal), maxVal)


# ---------------------------------------------------------------------------
# the composed forms (GLSL 4.30 §8.3 and §8.5)
# ---------------------------------------------------------------------------
def dot(a, b) -> int:
    return f_fma(a[2], b[2], f_fma(a[1], b[1], f_mul(a[0], b[0])))


def cross(a, b):
    return (f_fma(a[1], b[2], neg(f_mul(a[2], b[1]))), f_fma(a[2], b[0], neg(f_mul(a[0], b[2]))),
            f_fma(a[0], b[1], neg(f_mul(a[1], b[0]))))


def length(a) -> int:
    return f_sqrt(dot(a, a))


def normalize(a):
    n = length(a)
    return tuple(f_div(x, n) for x in a)


def reflect(i, n):
    """I - 2 * dot(N, I) * N, the scalar 2 * dot first."""
    s = f_mul(TWO, dot(n, i))
    return tuple(f_sub(x, f_mul(y, s)) for x, y in zip(i, n))


def mix(x, y, a: int):
    """x * (1 - a) + y * a."""
    w = f_sub(ONE, a)
    return tuple(f_add(f_mul(p, w), f_mul(q, a)) for p, q in zip(x, y))


def smoothstep(e0: int, e1: int, x: int) -> int:
    t = clamp(f_div(f_sub(x, e0), f_sub(e1, e0)), PZERO, ONE)
    return f_mul(f_mul(t, t), f_sub(THREE, f_mul(TWO, t)))


def refract_(i, n, eta: int):
    """The shader's own refract_: k = 1 - eta^2 (1 - dot(N,I)^2); total
    reflection (k < 0) reflects and reports 0, otherwise
    eta * I - (eta * dot(N,I) + sqrt(k)) * N and 1."""
    d = dot(n, i)
    k = f_sub(ONE, f_mul(f_mul(eta, eta), f_sub(ONE, f_mul(d, d))))
    if lt(k, PZERO):
        return reflect(i, n) + (0,)
    s = f_add(f_mul(eta, d), f_sqrt(k))
    return tuple(f_sub(f_mul(x, eta), f_mul(y, s)) for x, y in zip(i, n)) + (1,)


ACES = tuple(bits(c) for c in (2.51, 0.03, 2.43, 0.59, 0.14))


def aces1(x: int) -> int:
    """clamp((x (a x + b)) / (x (c x + d) + e), 0, 1), each operation rounded."""
    a, b, c, d, e = ACES
    num = f_mul(x, f_add(f_mul(a, x), b))
    den = f_add(f_mul(x, f_add(f_mul(c, x), d)), e)
    return clamp(f_div(num, den), PZERO, ONE)


SRGB_EXPONENT = f_div(ONE, bits(2.2))       # the shader's 1.0 / 2.2, in binary32


def pcg_step(state: int):
    """PCG-RXS-M-XS: (new state, the 32-bit draw)."""
    state = (state * 747796405 + 2891336453) & 0xFFFFFFFF
    r = (((state >> ((state >> 28) + 4)) ^ state) * 277803737) & 0xFFFFFFFF
    return state, (r >> 22) ^ r


def rnd(state: int):
    """(value bits, new state): float(draw) / 2^32, so 1.0 is reachable."""
    state, r = pcg_step(state)
    return f_div(f_from_uint(r), bits(4294967296.0)), state


def rnd_dir(state: int):
    """randomDirection: up to 100 candidates in [-1, 1)^3, the first of length
    < 1 normalised -> (x, y, z, new state, trips)."""
    for trip in range(1, 101):
        p = []
        for _ in range(3):
            v, state = rnd(state)
            p.append(f_sub(f_mul(v, TWO), ONE))
        if lt(length(p), ONE):
            return normalize(p) + (state, trip)
    return (PZERO, PZERO, PZERO, state, 100)


def rnd_dir_s(state: int) -> int:
    """dot(p, p) of the first candidate."""
    p = []
    for _ in range(3):
        v, state = rnd(state)
        p.append(f_sub(f_mul(v, TWO), ONE))
    return dot(p, p)


def pcg_state_for_draw(r: int) -> int:
    """The state whose next draw is r: the output permutation and the LCG step inverted."""
    w = r ^ (r >> 22)
    w = (w * pow(277803737, -1, 1 << 32)) & 0xFFFFFFFF
    k = (w >> 28) + 4                       # the shift leaves the top 4 bits alone
    s = w
    for _ in range(8):
        s = w ^ (s >> k)
    s0 = ((s - 2891336453) * pow(747796405, -1, 1 << 32)) & 0xFFFFFFFF
    assert pcg_step(s0)[1] == r
    return s0


# ---------------------------------------------------------------------------
# sky (getEnvironmentalLight): every product, sum, mix, smoothstep and clamp
# exactly as above; acos and exp from float64 libm at the binary32 operands.
# ---------------------------------------------------------------------------
def _acos_libm(u: int) -> int:
    if is_nan(u) or not -1.0 <= val(u) <= 1.0:
        return QNAN
    return bits(math.acos(val(u)))


def _exp_libm(u: int) -> int:
    if is_nan(u):
        return QNAN
    x = val(u)
    return bits(math.exp(x)) if x < 700.0 else INF


def _v(*c):
    return tuple(bits(x) for x in c)


def _muls(v, s):
    return tuple(f_mul(x, s) for x in v)


def _addv(a, b):
    return tuple(f_add(x, y) for x, y in zip(a, b))


def sky(d):
    sun = normalize(_v(0.6, 0.3, -0.2))
    sun_dot = dot(d, sun)
    horizon = d[1]
    zenith, orange, yellow = _v(0.15, 0.25, 0.65), _v(1.2, 0.4, 0.1), _v(1.0, 0.8, 0.3)
    blue, ground, centre = _v(0.3, 0.4, 0.7), _v(0.2, 0.15, 0.1), _v(15.0, 15.0, 10.0)
    s2o = f_mul(f_add(dot(d, tuple(neg(x) for x in sun)), ONE), HALF)
    if lt(s2o, HALF):
        hc = mix(orange, yellow, f_mul(s2o, TWO))
    else:
        hc = mix(yellow, blue, f_mul(f_sub(s2o, HALF), TWO))
    base = mix(hc, zenith, smoothstep(bits(-0.2), bits(0.8), horizon))
    angle = _acos_libm(clamp(sun_dot, bits(-1.0), ONE))
    na = QNAN if is_nan(angle) else neg(angle)
    g = [f_mul(_exp_libm(f_mul(na, bits(c))), bits(w)) if w != 1.0 else _exp_libm(f_mul(na, bits(c)))
         for c, w in ((600.0, 1.0), (150.0, 0.3), (60.0, 0.1), (15.0, 0.03))]
    glow = f_add(f_add(f_add(g[0], g[1]), g[2]), g[3])
    final = _addv(base, _muls(centre, glow))
    if lt(horizon, PZERO):
        final = mix(ground, final, smoothstep(bits(-0.1), PZERO, horizon))
        gs = f_mul(_exp_libm(f_mul(na, bits(15.0))), bits(0.2))
        final = _addv(final, _muls(_muls(centre, gs), bits(0.05)))
    return final


# |sky - this reference| per channel.  The pinned acos is within 3 ulp of the
# true angle and the reference's within 1/2, so the two exp arguments t = -c *
# angle differ by at most (3.5 + 1) * 2^-23 |t|; |t| e^-|t| <= 1/e bounds the
# effect on a glow term at 4.5 * 2^-23 / e = 2.0e-7, the pinned exp adds 3 ulp
# of a value <= 1 (3.6e-7) and the reference 1/2 ulp (6e-8): 6.2e-7 per unit
# weight.  The weights sum to 1.43 and the three sums round once each on both
# sides (6 * 2^-24 * 1.43 = 5.1e-7), so the total glow differs by at most
# 1.4e-6, and 15 * glow by 2.1e-5.  The remaining steps (one sum with the base
# colour, the ground mix with a weight in [0, 1], the ground glow of at most
# 0.15 * 6.2e-7) are the same exact operations on both sides applied to values
# below 23.1, and add at most 3 ulp(23.1) = 5.7e-6.
SKY_ABS_TOL = 2.7e-5


# ---------------------------------------------------------------------------
# error measures for the transcendentals
# ---------------------------------------------------------------------------
def ulp_error(got, true):
    """|got - true| in ulps of the true value, 2^-149 the ulp below 2^-126;
    `got` uint32 patterns, `true` float64.  A true NaN or infinity, and a NaN or
    infinity got for a finite value, count as inf unless the classes match (an
    overflow to infinity is measured as 2^128)."""
    g = np.asarray(got, np.uint32).view(np.float32).astype(np.float64)
    t = np.asarray(true, np.float64)
    t = np.where(np.abs(t) >= (2.0 - 2.0 ** -24) * 2.0 ** 127, np.copysign(np.inf, t), t)   # rounds to infinity
    with np.errstate(all="ignore"):
        e = np.floor(np.log2(np.abs(t)))
        e = np.where(np.isfinite(e), np.maximum(e, -126.0), -126.0)
        gg = np.where(np.isinf(g), np.copysign(2.0 ** 128, g), g)
        tt = np.where(np.isinf(t), np.copysign(2.0 ** 128, t), t)
        out = np.abs(gg - tt) / 2.0 ** (e - 23.0)
    both_nan = np.isnan(g) & np.isnan(t)
    out[both_nan] = 0.0
    out[np.isnan(g) ^ np.isnan(t)] = np.inf
    out[np.isinf(t) & (g == t)] = 0.0
    out[np.isinf(t) & (g != t)] = np.inf
    return out


def f64(u):
    return np.asarray(u, np.uint32).view(np.float32).astype(np.float64)


# ---------------------------------------------------------------------------
# input sets: functions returning (n, k) uint32 bit patterns
# ---------------------------------------------------------------------------
def _u32(rows):
    a = np.asarray(rows, dtype=np.uint64).astype(np.uint32)
    return a.reshape(len(a), -1)


def _both_signs(a):
    a = np.asarray(a, np.uint32)
    return np.concatenate([a, a | np.uint32(SIGN)])


def _near(u: int, k: int):
    """The k bit patterns below u, u and the k above (same sign, no wrap)."""
    return [u + j for j in range(-k, k + 1) if 0 <= (u & 0x7FFFFFFF) + j <= INF]


POW2 = [(e + 127) << 23 if e >= -126 else 1 << (e + 149) for e in range(-149, 128)]
SPECIALS = np.array(sorted(set(
    [p | s for s in (0, SIGN) for p in (PZERO, MIN_DEN, MAX_DEN, MIN_NORM, ONE - 1, ONE, ONE + 1, MAX_FIN, INF)]
    + [QNAN] + POW2 + [p | SIGN for p in POW2[::8]])), dtype=np.uint32)


def _cross2(a, b):
    return np.stack([np.repeat(a, len(b)), np.tile(b, len(a))], 1)


def _rng(seed):
    return np.random.default_rng(seed)


def _rand_finite(rng, n, lo_exp=1, hi_exp=254):
    """n random bit patterns with biased exponents in [lo_exp, hi_exp], either sign."""
    return (rng.integers(0, 2, n, dtype=np.uint64) << 31 | rng.integers(lo_exp, hi_exp + 1, n, dtype=np.uint64) << 23
            | rng.integers(0, 1 << 23, n, dtype=np.uint64)).astype(np.uint32)


def binary_inputs():
    """add, sub, fmin, fmax: the specials crossed with each other."""
    return _cross2(SPECIALS, SPECIALS)


def denormal_product_rows():
    """(a, b, shift): a * b = n * 2^-(149 + shift), among them the exact
    halfway cases n = q * 2^shift + 2^(shift - 1)."""
    rng = _rng(11)
    rows = []
    for s in range(1, 6):
        for i in range(600):
            q = int(rng.integers(0, 1 << (23 - s)))
            n = (q << s) + (1 << (s - 1)) if i % 2 == 0 else int(rng.integers(1, 1 << 24))
            j = int(rng.integers(s, 60))            # n * 2^-j times 2^(j - 149 - s)
            rows.append((round_fraction(Fraction(n, 1 << j)), POW2[(j - 149 - s) + 149], s))
    return rows


def mul_inputs():
    rng = _rng(12)
    half = np.array([(a, b) for a, b, _ in denormal_product_rows()], np.uint32)
    small = np.stack([_rand_finite(rng, 8000, 30, 70), _rand_finite(rng, 8000, 35, 75)], 1)   # products near 2^-149
    return np.concatenate([_cross2(SPECIALS, SPECIALS), half, half[:, ::-1], small])


def div_inputs():
    rng = _rng(13)
    # a / c = n * 2^-(149 + s): the same numerators over the power of two c = 1 / b, where it is finite
    half = np.array([(a, f_div(ONE, b)) for a, b, _ in denormal_product_rows() if not is_inf(f_div(ONE, b))],
                    np.uint32)
    den = rng.integers(1, 1 << 23, (6000, 2), dtype=np.uint64).astype(np.uint32)                # denormal / denormal
    den_norm = np.stack([den[:3000, 0], _rand_finite(rng, 3000, 100, 254)], 1)                  # denormal / large
    small = np.stack([_rand_finite(rng, 6000, 1, 60), _rand_finite(rng, 6000, 120, 200)], 1)    # denormal quotients
    return np.concatenate([_cross2(SPECIALS, SPECIALS), half, den, den_norm, den_norm[:, ::-1], small])


def rcp_inputs():
    rng = _rng(14)
    return _u32(np.concatenate([SPECIALS, _rand_finite(rng, 20000), _both_signs(np.arange(1, 1 << 23, 1 << 11)),
                                np.arange(0x7E800000 - 64, 0x7E800000 + 64)]))   # 1/x turning denormal at 2^126


def fma_double_rounding_rows():
    """Triples where rounding a*b+c to float64 and then to binary32 differs
    from the single rounding.  c = X with an odd significand and ulp u; a * b =
    +-(u/2)(1 - k^2 2^-46) from a = (u/2)(1 + k 2^-23), b = 1 - k 2^-23.  The sum
    lies k^2 2^-47 u inside the midpoint between X and its neighbour, less than
    half a float64 ulp of X (2^-30 u) for k <= 256, so float64 rounds it onto the
    midpoint and the second rounding takes the even neighbour, while the single
    rounding returns X."""
    rng = _rng(21)
    rows = []
    for i in range(3000):
        ex = int(rng.integers(40, 230))
        X = (ex << 23) | int(rng.integers(0, 1 << 22)) << 1 | 1
        k = int(rng.integers(1, 257))
        j = int(rng.integers(-8, 9))                   # a * 2^j, b * 2^-j: the same product
        a = (((ex - 24 + j) << 23) | k)                # 2^(ex - 127 - 24 + j) (1 + k 2^-23)
        b = ((ONE - 2 * k) - (j << 23))                # (1 - k 2^-23) 2^-j
        sx, sp = (SIGN if i & 1 else 0), (SIGN if i & 2 else 0)
        rows.append((a | sp, b, X | sx))
    return rows


def fma_cancellation_rows():
    """Triples with c = -RN(a * b): the fused result is the product's rounding
    error, the unfused one is 0 (or differs wherever the product is inexact)."""
    rng = _rng(22)
    a = _rand_finite(rng, 3000, 60, 190)
    b = _rand_finite(rng, 3000, 60, 190)
    return [(int(x), int(y), neg(f_mul(int(x), int(y)))) for x, y in zip(a, b)]


def fma_inputs():
    rng = _rng(23)
    sp = SPECIALS[rng.integers(0, len(SPECIALS), (12000, 3))]
    few = np.array([p | s for s in (0, SIGN) for p in (PZERO, MIN_DEN, MIN_NORM, ONE, MAX_FIN, INF)] + [QNAN],
                   np.uint32)
    cube = np.stack(np.meshgrid(few, few, few, indexing="ij"), -1).reshape(-1, 3)
    rand = np.stack([_rand_finite(rng, 6000, 100, 150) for _ in range(3)], 1)
    return np.concatenate([_u32(fma_double_rounding_rows()), _u32(fma_cancellation_rows()), sp, cube, rand])


def sqrt_inputs():
    rng = _rng(31)
    squares = [f_from_uint(n * n) for n in range(1, 4096)]
    sq = [v for s in squares for v in _near(s, 1)]
    scaled = [s - (j << 24) for s in squares[:1024] for j in (20, 55)]      # n^2 * 4^-j
    one = np.arange(ONE - (1 << 16), ONE + (1 << 16) + 1)
    stride = np.arange(bits(0.25), bits(4.0), 1531)
    den = np.concatenate([np.arange(0, 1 << 23, 1 << 10), [1, 2, 3, MAX_DEN, MIN_NORM, MIN_NORM + 1]])
    return _u32(np.concatenate([SPECIALS, sq, scaled, one, stride, den, _rand_finite(rng, 4000)]))


LOG2E = bits(1.44269504088896341)
EXP_HI, EXP_LO = bits(88.7228317), bits(-103.972076)


def exp_rint_ties():
    """Arguments x with RN(x * log2(e)) an exact half-integer, the ties of the
    rint in rt2pm_expf: for each k + 1/2 in the function's range, the binary32
    around (k + 1/2) / log2(e) that the product maps onto it."""
    out = []
    for k in range(-150, 128):
        h = bits(k + 0.5)
        x0 = bits((k + 0.5) / 1.44269504088896341)
        out += [x for x in _near(x0, 3) if f_mul(x, LOG2E) == h]
    return out


def exp_inputs():
    lo_band, hi_band = bits(-103.98), bits(-87.3)           # exp(x) denormal or just normal
    return _u32(np.concatenate([
        SPECIALS, _near(EXP_HI, 8), _near(EXP_LO, 8), np.arange(hi_band, lo_band, 61), exp_rint_ties(),
        _both_signs(np.arange(0, 1 << 23, 1 << 12)), _both_signs(np.arange(bits(1e-6), bits(88.0), 9973)),
        np.arange(bits(-87.5), bits(-87.2), 3)]))            # the result crossing 2^-126


def log_inputs():
    m = bits(0.70710678)
    around = [(u & 0x7FFFFF) | (e << 23) for u in _near(m, 6) for e in (1, 2, 64, 126, 127, 128, 200, 254)]
    # the subnormal rescale's own 0.7071: 0.70710678 * 2^-126 * 2^-j
    around += [((u & 0x7FFFFF) | 0x800000) >> j for u in _near(m, 6) for j in (1, 2, 9)]
    return _u32(np.concatenate([
        SPECIALS, np.arange(1, 1 << 23, 509), _near(MIN_NORM, 6), around, _near(ONE, 8), [PZERO, NZERO, INF],
        [bits(-1.0), bits(-1e-40), NINF], np.arange(bits(0.5), bits(2.0), 2039), np.arange(MIN_NORM, MAX_FIN, 104729)]))


def acos_inputs():
    one_side = np.concatenate([ONE - np.arange(0, 65), _near(HALF, 8), [PZERO, 1, 2, MAX_DEN, MIN_NORM],
                               ONE + np.arange(1, 4), np.arange(0, 1 << 23, 1 << 12),
                               np.arange(bits(1e-4), ONE, 2719)])
    return _u32(np.concatenate([_both_signs(one_side), SPECIALS]))


SINCOS_DOMAIN = 8192.0


def sincos_inputs():
    pts = [PZERO, NZERO]
    for k in range(1, int(SINCOS_DOMAIN * 4 / math.pi)):
        c = bits(k * math.pi / 4)
        near = _near(c, 2)
        pts += near if k % 8 else near + [u | SIGN for u in near]
    pts = [u for u in pts if abs(val(u)) < SINCOS_DOMAIN]
    return _u32(np.concatenate([pts, _both_signs(np.arange(0, 1 << 23, 1 << 12)),
                                _both_signs(np.arange(0, bits(2 * math.pi), 40009)), [QNAN]]))


def pow_inputs():
    x = np.concatenate([[PZERO, ONE - 1, ONE, 1, 2, MAX_DEN, MIN_NORM], np.arange(0, 1 << 23, 1 << 11),
                        np.arange(0, ONE, 32749)])
    return np.stack([x.astype(np.uint32), np.full(len(x), SRGB_EXPONENT, np.uint32)], 1)


def aces_overflow_points():
    """The smallest binary32 at which x * (2.51 x + 0.03) and x * (2.43 x + 0.59)
    overflow: found by bisection on the exact reference."""
    out = []
    for a, b in ((ACES[0], ACES[1]), (ACES[2], ACES[3])):
        lo, hi = bits(1e18), bits(1e20)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if is_inf(f_mul(mid, f_add(f_mul(a, mid), b))) else (mid, hi)
        out.append(hi)
    return out


def aces_inputs():
    """aces1 / srgb1(aces1) / the tonemap resolve: one word per row."""
    edges = [u for p in aces_overflow_points() for u in _near(p, 8)]
    return _u32(np.concatenate([
        [PZERO, NZERO, INF, NINF, QNAN, bits(1e6), bits(-1e6), MAX_FIN, MAX_FIN | SIGN, bits(1e30), MIN_DEN, MAX_DEN,
         MIN_NORM], edges,
        [u | SIGN for u in edges], [bits(-x) for x in (1e-45, 1e-40, 1e-30, 1e-6, 1e-3, 0.0119, 0.012, 0.02, 0.5, 5.0)],
        np.arange(0, 1 << 23, 1 << 13), np.arange(0, bits(16.0) + 1, 54013)]))


def clamp_inputs():
    z = [PZERO, NZERO]
    few = [PZERO, NZERO, MIN_DEN, MIN_DEN | SIGN, HALF, ONE, ONE | SIGN, ONE + 1, TWO, INF, NINF, QNAN]
    rows = [(x, lo, hi) for x in few for lo in few for hi in few]
    rows += [(x, lo, ONE) for x in z for lo in z] + [(x, bits(-1.0), hi) for x in z for hi in z]
    return _u32(rows)


def minmax_zero_rows():
    """The rows of binary_inputs() that are zeros of opposite sign."""
    b = binary_inputs()
    return np.flatnonzero(((b[:, 0] | b[:, 1]) == SIGN) & ((b[:, 0] & b[:, 1]) == 0))


def _vec_pool(rng, n):
    """n vectors: ordinary, tiny (|v|^2 underflows), huge (|v|^2 overflows),
    axis-aligned, zero, and with special components."""
    kinds = [(100, 150), (1, 30), (225, 254), (0, 0)]
    out = np.zeros((n, 3), np.uint32)
    for i in range(n):
        lo, hi = kinds[i % 4]
        v = _rand_finite(rng, 3, lo, hi) if hi else rng.integers(0, 1 << 23, 3, dtype=np.uint64).astype(np.uint32)
        if i % 7 == 0:
            v[rng.integers(0, 3)] = PZERO if i % 2 else NZERO                  # a zero component
        if i % 11 == 0:
            keep = rng.integers(0, 3)
            v = np.array([v[k] if k == keep else (PZERO, NZERO)[(i + k) & 1] for k in range(3)], np.uint32)
        if i % 13 == 0:
            v[rng.integers(0, 3)] = SPECIALS[rng.integers(0, len(SPECIALS))]
        if i % 97 == 0:
            v[:] = (PZERO, NZERO)[i & 1]
        out[i] = v
    return out


def vector_inputs(seed=41, n=6000):
    """(n, 7): two vectors and a scalar, for dot / cross / length / normalize /
    reflect / mix."""
    rng = _rng(seed)
    a, b = _vec_pool(rng, n), _vec_pool(rng, n)
    # like against like too, so that products neither all vanish nor all overflow
    b[::3] = np.roll(a, 1, 0)[::3] ^ (rng.integers(0, 2, (len(a[::3]), 3), dtype=np.uint64) << 31).astype(np.uint32)
    s = _rand_finite(rng, n, 110, 135)
    s[::5] = np.array([PZERO, ONE, NZERO, ONE - 1, ONE + 1, INF, QNAN, HALF], np.uint32)[np.arange(len(s[::5])) % 8]
    return np.concatenate([a, b, s[:, None]], 1)


def unit_vector_inputs(seed=42, n=4000):
    """(n, 7): unit I and N (rounded) and a scalar in [0, 2): the operands the
    shader gives reflect, refract_ and mix."""
    rng = _rng(seed)
    v = rng.standard_normal((n, 2, 3))
    v /= np.sqrt((v * v).sum(-1, keepdims=True))
    s = rng.uniform(0.0, 2.0, n)
    s[::4] = np.resize([0.0, 1.0, 0.5, 1.0 / 1.5], len(s[::4]))
    rows = [[bits(float(x)) for x in v[i].reshape(-1)] + [bits(float(s[i]))] for i in range(n)]
    return _u32(rows)


def refract_inputs():
    """Unit vectors, plus rows with k just below, at and just above 0: N = +z,
    I in the xz plane at the critical angle of eta = 1.5 and its neighbours."""
    rows = [tuple(r) for r in unit_vector_inputs(43, 3000)]
    eta = bits(1.5)
    for j in range(-40, 41):
        c = bits(math.sqrt(1.0 - 1.0 / 2.25)) + j          # cos of the critical angle, +- j ulp
        sx = bits(math.sqrt(max(0.0, 1.0 - val(c) ** 2)))
        for sg in (0, SIGN):
            rows.append((sx, PZERO, c | sg, PZERO, PZERO, ONE, eta))
    rows += [tuple(r) for r in vector_inputs(44, 1500)]
    return _u32(rows)


def smoothstep_inputs():
    rows = []
    for e0, e1 in ((bits(-0.2), bits(0.8)), (bits(-0.1), PZERO), (PZERO, ONE), (ONE, PZERO), (ONE, ONE),
                   (MIN_DEN, MAX_DEN), (bits(-1e30), bits(3e38))):
        xs = _near(e0, 4) + _near(e1, 4) + [PZERO, NZERO, INF, NINF, QNAN, MAX_FIN, MAX_FIN | SIGN]
        lo, hi = sorted((val(e0), val(e1)))
        xs += [bits(lo + (hi - lo) * t / 400.0) for t in range(-40, 441)]
        rows += [(e0, e1, x) for x in xs]
    return _u32(rows)


def sky_inputs():
    """(n, 3) directions: the sun's own and its neighbourhood (sunDot inside and
    outside +-1 by scaling), the horizon terms' edges in dir.y, sunAngle across
    the band where exp(-600 sunAngle) is denormal, unit and non-unit random
    directions, NaN and infinite components."""
    rng = _rng(51)
    sun = np.array([0.6, 0.3, -0.2])
    sun /= math.sqrt(float(sun @ sun))
    sunb = normalize(_v(0.6, 0.3, -0.2))
    e1 = np.cross(sun, [0.0, 1.0, 0.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(sun, e1)
    rows = [sunb, tuple(neg(x) for x in sunb)]
    for s in (1.0 - 2e-7, 1.0 - 6e-8, 1.0 + 6e-8, 1.0 + 2e-7, 1.0 + 1e-6, 1.5, 0.5, 1e-20, 1e20, 3e38):
        for sg in (1.0, -1.0):
            rows.append(_v(*(sg * s * sun)))
    for j in range(-6, 7):                                    # the sun's components +- ulps
        rows += [(sunb[0] + j, sunb[1], sunb[2]), (sunb[0], sunb[1] - j, sunb[2] + j)]
    for t in np.concatenate([np.linspace(0.0, 0.01, 200), np.linspace(0.14, 0.18, 1200), np.linspace(0.0, math.pi, 1500)]):
        ph = rng.uniform(0, 2 * math.pi)
        rows.append(_v(*(math.cos(t) * sun + math.sin(t) * (math.cos(ph) * e1 + math.sin(ph) * e2))))
    for y in (-0.1, 0.0, 0.8, -0.2):                          # dir.y at the edges of the two smoothsteps
        for u in _near(bits(y), 5) + ([NZERO, MIN_DEN, MIN_DEN | SIGN] if y == 0.0 else []):
            x = math.sqrt(max(0.0, 1.0 - val(u) ** 2))
            rows += [(bits(x), u, PZERO), (bits(-0.6 * x), u, bits(0.8 * x))]
    v = rng.standard_normal((3000, 3))
    v /= np.sqrt((v * v).sum(-1, keepdims=True))
    rows += [_v(*r) for r in v] + [_v(*(r * 10.0 ** rng.uniform(-3, 3))) for r in v[:600]]
    for bad in (QNAN, INF, NINF):
        for k in range(3):
            rows.append(tuple(bad if i == k else bits(0.5) for i in range(3)))
    rows += [(PZERO, PZERO, PZERO), (NZERO, NZERO, NZERO)]
    return _u32(rows)


# rnd_dir's acceptance edge: states whose first candidate has s = dot(p, p)
# equal to 1 - 2^-24 (the last accepted), 1 and 1 + 2^-23 (the first two
# rejected).  Found by edge_state_search(); each is re-derived by the exact
# reference in tests/test_numerics_cases.py.
EDGE_STATES = {
    ONE - 1: (0x1716F43, 0x1C6F584, 0x1ED15DD, 0x21A4AC3),
    ONE: (0xD29F5E, 0x1E012EA, 0x277FB13),
    ONE + 1: (0x410E34, 0x18CDA09, 0x1B86DAF),
}


def edge_state_search(first=0, count=3 << 24):   # pragma: no cover - the tool that produced EDGE_STATES
    """States first .. first + count whose first candidate has a float64
    estimate of s within 1e-6 of 1, each decided by rnd_dir_s()."""
    found = {k: [] for k in EDGE_STATES}
    for base in range(first, first + count, 1 << 22):
        s0 = np.arange(base, base + (1 << 22), dtype=np.uint64) & np.uint64(0xFFFFFFFF)
        st, s = s0.copy(), 0.0
        for _ in range(3):
            st = (st * np.uint64(747796405) + np.uint64(2891336453)) & np.uint64(0xFFFFFFFF)
            r = (((st >> ((st >> np.uint64(28)) + np.uint64(4))) ^ st) * np.uint64(277803737)) & np.uint64(0xFFFFFFFF)
            r = ((r >> np.uint64(22)) ^ r).astype(np.float64)
            s = s + (r / 2.0 ** 31 - 1.0) ** 2
        for i in np.flatnonzero(np.abs(s - 1.0) < 1e-6):
            k = rnd_dir_s(int(s0[i]))
            if k in found:
                found[k].append(int(s0[i]))
    return found


def long_trip_states(count=60000, trips=8):
    """States among 0 .. count - 1 whose direction needs at least `trips`
    candidates (a float64 pre-filter; the premise test counts the trips exactly)."""
    s0 = np.arange(count, dtype=np.uint64)
    st = s0.copy()
    alive = np.ones(count, bool)
    for _ in range(trips - 1):
        s = 0.0
        for _ in range(3):
            st = (st * np.uint64(747796405) + np.uint64(2891336453)) & np.uint64(0xFFFFFFFF)
            r = (((st >> ((st >> np.uint64(28)) + np.uint64(4))) ^ st) * np.uint64(277803737)) & np.uint64(0xFFFFFFFF)
            r = ((r >> np.uint64(22)) ^ r).astype(np.float64)
            s = s + (r / 2.0 ** 31 - 1.0) ** 2
        alive &= s > 1.0 + 1e-6
    return [int(x) for x in s0[alive]]


DRAW_ZERO = [0]
DRAW_ONE = [0xFFFFFFFF, 0xFFFFFF80, 0xFFFFFFC1]            # r >= 2^32 - 128 rounds to 2^32
DRAW_BELOW_ONE = [0xFFFFFF7F, 0xFFFFFE81, 0xFFFFFF00]      # rounds to 2^32 - 256: 1 - 2^-24


def rnd_inputs():
    sp = [pcg_state_for_draw(r) for r in DRAW_ZERO + DRAW_ONE + DRAW_BELOW_ONE + [1, 127, 128, 0x80000000, 0x01000001]]
    return _u32(np.concatenate([sp, np.arange(0, 20000), _rng(61).integers(0, 1 << 32, 10000, dtype=np.uint64)]))


def rnd_dir_inputs():
    edge = [s for v in EDGE_STATES.values() for s in v]
    # a draw of exactly 0, 1.0 or 1 - 2^-24 as a candidate's first component
    sp = [pcg_state_for_draw(r) for r in DRAW_ZERO + DRAW_ONE + DRAW_BELOW_ONE]
    return _u32(np.concatenate([edge, sp, long_trip_states(), np.arange(0, 6000),
                                _rng(62).integers(0, 1 << 32, 4000, dtype=np.uint64)]))


# ---------------------------------------------------------------------------
# the operations: name -> (input set, reference) for the bit-exact ones
# ---------------------------------------------------------------------------
def _scalar(fn, k):
    return lambda row: (fn(*[int(x) for x in row[:k]]),)


def _vec2(fn):
    def run(row):
        r = fn(tuple(int(x) for x in row[0:3]), tuple(int(x) for x in row[3:6]))
        return r if isinstance(r, tuple) else (r,)
    return run


def _vec2s(fn):
    return lambda row: fn(tuple(int(x) for x in row[0:3]), tuple(int(x) for x in row[3:6]), int(row[6]))


def _vec1(fn):
    def run(row):
        r = fn(tuple(int(x) for x in row[0:3]))
        return r if isinstance(r, tuple) else (r,)
    return run


def _vectors():
    return np.concatenate([vector_inputs(), unit_vector_inputs()])


# Operations the exact reference decides in every bit: name -> (inputs, row -> result words).
EXACT_OPS = {
    "div": (div_inputs, _scalar(f_div, 2)),
    "rcp": (rcp_inputs, _scalar(lambda a: f_div(ONE, a), 1)),
    "sqrt": (sqrt_inputs, _scalar(f_sqrt, 1)),
    "fma": (fma_inputs, _scalar(f_fma, 3)),
    "mul": (mul_inputs, _scalar(f_mul, 2)),
    "add": (binary_inputs, _scalar(f_add, 2)),
    "sub": (binary_inputs, _scalar(f_sub, 2)),
    "fmin": (binary_inputs, _scalar(f_min, 2)),
    "fmax": (binary_inputs, _scalar(f_max, 2)),
    "clamp": (clamp_inputs, _scalar(clamp, 3)),
    "dot": (_vectors, _vec2(dot)),
    "cross": (_vectors, _vec2(cross)),
    "length": (_vectors, _vec1(length)),
    "normalize": (_vectors, _vec1(normalize)),
    "reflect": (_vectors, _vec2(reflect)),
    "refract": (refract_inputs, _vec2s(refract_)),
    "mix": (_vectors, _vec2s(mix)),
    "smoothstep": (smoothstep_inputs, _scalar(smoothstep, 3)),
    "aces1": (aces_inputs, _scalar(aces1, 1)),
    "rnd": (rnd_inputs, lambda row: rnd(int(row[0]))),
    "rnd_dir": (rnd_dir_inputs, lambda row: rnd_dir(int(row[0]))[:4]),
}
# Words of the result that are no floats (compared as integers, never as NaNs).
RAW_WORDS = {"refract": (3,), "rnd": (1,), "rnd_dir": (3,)}

# The transcendentals: name -> (inputs, float64 reference of the operand columns, bound, "ulp" or "abs").
# exp, log, acos: 3 ulp; sin / cos: 1e-7 absolute
# (tests/test_oracle_kat.py); pow(x, 1/2.2) on [0, 1]: 1e-6 absolute.
def _true_exp(x):
    with np.errstate(all="ignore"):
        return np.exp(x[:, 0])


def _true_log(x):
    with np.errstate(all="ignore"):
        return np.where(x[:, 0] == 0.0, -np.inf, np.log(x[:, 0]))


def _true_acos(x):
    with np.errstate(all="ignore"):
        return np.arccos(x[:, 0])


def _true_pow(x):
    with np.errstate(all="ignore"):
        return np.where(x[:, 0] == 0.0, 0.0, np.power(x[:, 0], x[:, 1]))


TRANSCENDENTALS = {
    "exp": (exp_inputs, _true_exp, 3.0, "ulp"),
    "log": (log_inputs, _true_log, 3.0, "ulp"),
    "acos": (acos_inputs, _true_acos, 3.0, "ulp"),
    "cos": (sincos_inputs, lambda x: np.cos(x[:, 0]), 1e-7, "abs"),
    "sin": (sincos_inputs, lambda x: np.sin(x[:, 0]), 1e-7, "abs"),
    "pow": (pow_inputs, _true_pow, 1e-6, "abs"),
}

ALL_OPS = list(EXACT_OPS) + list(TRANSCENDENTALS) + ["srgb1", "sky"]

_cache = {}


def inputs(op):
    """The input rows of an operation, computed once."""
    if ("in", op) not in _cache:
        if op in EXACT_OPS:
            r = EXACT_OPS[op][0]()
        elif op in TRANSCENDENTALS:
            r = TRANSCENDENTALS[op][0]()
        elif op == "srgb1":
            r = pow_inputs()[:, :1]
        else:
            r = sky_inputs()
        r = np.ascontiguousarray(r, np.uint32)
        r.setflags(write=False)
        _cache["in", op] = r
    return _cache["in", op]


def reference(op):
    """The exact reference's result words for inputs(op), (n, k) uint32, computed once."""
    if ("ref", op) not in _cache:
        fn = sky_rows if op == "sky" else EXACT_OPS[op][1]
        r = np.array([fn(row) for row in inputs(op)], dtype=np.uint64).astype(np.uint32)
        r.setflags(write=False)
        _cache["ref", op] = r
    return _cache["ref", op]


def sky_rows(row):
    return sky(tuple(int(x) for x in row[:3]))


def mismatches(op, got, want):
    """Rows where `got` (n, 4) differs from `want` (n, k <= 4) in a bit; any NaN
    equals any NaN in the float words."""
    got, want = np.asarray(got, np.uint32)[:, :want.shape[1]], np.asarray(want, np.uint32)
    same = got == want
    nan = ((got & 0x7FFFFFFF) > INF) & ((want & 0x7FFFFFFF) > INF)
    for k in range(want.shape[1]):
        if k not in RAW_WORDS.get(op, ()):
            same[:, k] |= nan[:, k]
    return np.flatnonzero(~same.all(1))


def transcendental_error(op, got):
    """(errors, bound) of result word 0 against float64 libm."""
    fn, bound, kind = TRANSCENDENTALS[op][1:]
    x = f64(inputs(op))
    with np.errstate(all="ignore"):
        true = fn(x)
    if kind == "ulp":
        return ulp_error(got[:, 0], true), bound
    g = f64(got[:, 0])
    err = np.abs(g - true)
    err[np.isnan(g) & np.isnan(true)] = 0.0
    err[np.isnan(g) ^ np.isnan(true)] = np.inf
    return err, bound


def sky_error(got):
    """max |got - reference| per row over the three channels; rows where the
    classes (NaN, infinity) differ count as inf."""
    g, r = f64(got[:, :3]), f64(reference("sky"))
    with np.errstate(all="ignore"):
        err = np.abs(g - r)
    err[np.isnan(g) & np.isnan(r)] = 0.0
    err[np.isinf(g) & (g == r)] = 0.0
    err[np.isnan(err)] = np.inf
    return err.max(1)


def check_op(op, run):
    """Holds one operation of an implementation to the reference: run(op, rows)
    -> (n, 4) uint32.  Returns (failure text or None, the measured maximum or
    None): every bit for the IEEE operations and the composed forms, the
    documented bound for the transcendentals, SKY_ABS_TOL for sky; srgb1 must be
    pow(x, 1 / 2.2) of the same implementation in every bit."""
    rows = inputs(op)
    out = run(op, rows)
    assert out.shape == (len(rows), 4)
    if op in EXACT_OPS:
        bad = mismatches(op, out, reference(op))
        if len(bad) == 0:
            return None, None
        i = int(bad[0])
        return (f"{op}: {len(bad)} of {len(rows)} rows differ from the exact reference; row {i}: in "
                f"{[hex(x) for x in rows[i]]} got {[hex(x) for x in out[i]]} want "
                f"{[hex(x) for x in reference(op)[i]]}"), None
    if op == "srgb1":
        pw = run("pow", pow_inputs())
        bad = mismatches(op, out, pw[:, :1])
        return (f"srgb1: {len(bad)} rows differ from pow(x, 1/2.2)" if len(bad) else None), None
    if op == "sky":
        err = sky_error(out)
        i = int(err.argmax())
        worst = float(err[i])
        return (None if worst <= SKY_ABS_TOL else
                f"sky: |error| {worst:.3e} > {SKY_ABS_TOL} at {[hex(x) for x in rows[i]]}"), worst
    err, bound = transcendental_error(op, out)
    i = int(err.argmax())
    worst = float(err[i])
    return (None if worst <= bound else
            f"{op}: error {worst:.4g} > {bound} ({TRANSCENDENTALS[op][3]}) at {[hex(x) for x in rows[i]]}"), worst


def bit_differences(op, run_a, run_b):
    """The rows of inputs(op) on which two implementations differ in a bit (any NaN equals any NaN)."""
    rows = inputs(op)
    return mismatches(op, run_a(op, rows), run_b(op, rows))
