"""The pinned arithmetic of DESIGN.md §Numerics on the CPU: the premises of the
input sets of tests/numerics_cases.py, the oracle's own functions
(oracle_numerics) against the exact reference, and the sensitivity of those
inputs to the defects they are there for.

The oracle equals the exact reference in every bit on the IEEE operations and
the composed forms, and stays inside the documented bounds on the
transcendentals.  Measured maxima over the input sets (printed by
test_oracle_against_the_reference, `pytest -s`):

    exp   0.923 ulp            log   0.748 ulp          acos  1.214 ulp
    cos   7.49e-8 absolute     sin   7.48e-8 absolute   pow   5.32e-8 absolute
    sky   1.91e-6 absolute (bound SKY_ABS_TOL = 2.7e-5)

Mutated builds of the oracle, compiled beside it the way
tests/test_bvh_edge_scenes.py builds its own: `-ffp-contract=fast` and a `dot`
summed in the other order fail the exact reference; an unfused RT2PM_FMA
differs from the oracle in bits on every pinned function, which is the check
tests/test_gpu_numerics.py applies to the device; an unchanged rebuild passes
everything.
"""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import numerics_cases as N

ORACLE_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle")
ORACLE_SRC = os.path.join(ORACLE_DIR, "rt_oracle.c")
GCC = ["gcc", "-O3", "-std=c11", "-fPIC", "-fno-fast-math", "-fno-math-errno", "-march=x86-64-v3", "-I", ORACLE_DIR,
       "-shared"]


# ---------------------------------------------------------------------------
# the exact rounding itself
# ---------------------------------------------------------------------------
def test_round_fraction_edges():
    R, F = N.round_fraction, Fraction
    tiny = F(1, 1 << 149)
    assert R(F(0)) == N.PZERO and R(F(0), N.SIGN) == N.NZERO
    assert R(tiny) == 1 and R(-tiny) == N.SIGN | 1
    assert R(tiny / 2) == 0 and R(tiny / 2 + F(1, 1 << 200)) == 1         # the tie goes to even, just above does not
    assert R(tiny * 3 / 2) == 2 and R(tiny * 5 / 2) == 2 and R(tiny * 7 / 2) == 4
    assert R(F(1, 1 << 126)) == N.MIN_NORM and R(F(1, 1 << 126) - tiny) == N.MAX_DEN
    assert R(F(1, 1 << 126) - tiny / 2) == N.MIN_NORM                        # a tie onto the first normal
    top = F(2) ** 128
    assert R(top - F(2) ** 104) == N.MAX_FIN
    assert R(top - F(2) ** 103) == N.INF and R(top - F(2) ** 103 - 1) == N.MAX_FIN   # the overflow threshold is a tie
    assert R(-top) == N.NINF
    assert R(1 + F(1, 1 << 24)) == N.ONE and R(1 + F(3, 1 << 24)) == N.ONE + 2
    assert R(1 - F(1, 1 << 25)) == N.ONE and R(1 - F(3, 1 << 25)) == N.ONE - 2


def test_round_fraction_equals_the_rounding_of_float64():
    """Every float64 is a rational; struct rounds it to binary32 correctly."""
    rng = np.random.default_rng(5)
    xs = rng.standard_normal(20000) * 10.0 ** rng.uniform(-46, 39, 20000)
    for x in xs:
        assert N.round_fraction(Fraction(float(x))) == N.bits(float(x))


def test_operations_on_small_integers_and_signed_zeros():
    b = N.bits
    assert N.f_add(b(1.5), b(2.25)) == b(3.75) and N.f_mul(b(3.0), b(-0.5)) == b(-1.5)
    assert N.f_div(b(1.0), b(3.0)) == b(1.0 / 3.0) and N.f_sqrt(b(2.0)) == b(2.0 ** 0.5)
    assert N.f_sqrt(b(9.0)) == b(3.0) and N.f_sqrt(N.NZERO) == N.NZERO and N.f_sqrt(b(-1.0)) == N.QNAN
    assert N.f_add(N.PZERO, N.NZERO) == N.PZERO and N.f_add(N.NZERO, N.NZERO) == N.NZERO
    assert N.f_sub(b(1.0), b(1.0)) == N.PZERO and N.f_sub(N.NZERO, N.PZERO) == N.NZERO
    assert N.f_fma(b(-1.0), N.PZERO, N.NZERO) == N.NZERO and N.f_fma(b(1.0), N.PZERO, N.NZERO) == N.PZERO
    assert N.f_mul(N.INF, N.PZERO) == N.QNAN and N.f_sub(N.INF, N.INF) == N.QNAN
    assert N.f_div(b(1.0), N.NZERO) == N.NINF and N.f_div(N.PZERO, N.NZERO) == N.QNAN
    assert N.f_max(N.PZERO, N.NZERO) == N.PZERO == N.f_max(N.NZERO, N.PZERO)
    assert N.f_min(N.PZERO, N.NZERO) == N.NZERO == N.f_min(N.NZERO, N.PZERO)
    assert N.f_max(N.QNAN, b(1.0)) == b(1.0) == N.f_min(b(1.0), N.QNAN)


# ---------------------------------------------------------------------------
# premises of the input sets
# ---------------------------------------------------------------------------
def test_sizes():
    """A few 10^4 to 10^5 rows for the scalar operations (sqrt must hold all
    2^17 + 1 floats around 1), thousands for the vector forms."""
    for op in N.ALL_OPS:
        n = len(N.inputs(op))
        assert 1500 <= n <= 200000, (op, n)
    assert len(N.inputs("sqrt")) >= (1 << 17) + 1


def test_specials_are_all_there():
    s = set(int(x) for x in N.SPECIALS)
    for p in (N.PZERO, N.MIN_DEN, N.MAX_DEN, N.MIN_NORM, N.ONE - 1, N.ONE, N.ONE + 1, N.MAX_FIN, N.INF):
        assert p in s and (p | N.SIGN) in s
    assert N.QNAN in s and all(N.bits(2.0 ** e) in s for e in range(-149, 128))
    assert len(N.binary_inputs()) == len(s) ** 2 and len(N.minmax_zero_rows()) == 2


def test_denormal_products_and_quotients():
    rows = N.denormal_product_rows()
    halfway = 0
    for a, b, s in rows:
        (ma, ea), (mb, eb) = N.dec(a), N.dec(b)
        n, e = ma * mb, ea + eb
        assert e <= -150 and n < (1 << 24) << (-149 - e)                 # below 2^-125: a denormal or the first normals
        halfway += (n << 1) % (1 << (-149 - e)) == 0 and (n % (1 << (-149 - e))) != 0
    assert halfway >= 1500
    d = N.div_inputs()
    both_den = ((d[:, 0] & 0x7F800000) == 0) & ((d[:, 1] & 0x7F800000) == 0) & ((d[:, 0] & 0x7FFFFFFF) != 0) & \
        ((d[:, 1] & 0x7FFFFFFF) != 0)
    assert both_den.sum() >= 6000
    ref = N.reference("div")[:, 0]
    den_result = ((ref & 0x7F800000) == 0) & ((ref & 0x7FFFFFFF) != 0)
    assert den_result.sum() >= 3000
    ref = N.reference("mul")[:, 0]
    assert (((ref & 0x7F800000) == 0) & ((ref & 0x7FFFFFFF) != 0)).sum() >= 3000


def test_fma_killers():
    """At least 1,000 triples on which float64-then-binary32 differs from the
    single rounding, and 1,000 on which the rounded product plus c does."""
    double_rounding = 0
    for a, b, c in N.fma_double_rounding_rows():
        twice = N.bits(N.val(a) * N.val(b) + N.val(c))       # the product is exact in float64; the sum rounds to it
        double_rounding += twice != N.f_fma(a, b, c)
    assert double_rounding >= 1000, double_rounding
    unfused = 0
    for a, b, c in N.fma_double_rounding_rows() + N.fma_cancellation_rows():
        unfused += N.f_add(N.f_mul(a, b), c) != N.f_fma(a, b, c)
    assert unfused >= 1000, unfused
    assert double_rounding == len(N.fma_double_rounding_rows())   # every constructed triple is one


def test_sqrt_inputs():
    s = set(int(x) for x in N.inputs("sqrt")[:, 0])
    assert all(u in s for u in range(N.ONE - (1 << 16), N.ONE + (1 << 16) + 1))
    assert all(N.bits(float(n * n)) in s for n in range(1, 4096))
    assert sum(1 for u in s if 0 < u < N.MIN_NORM) >= 8000
    assert sum(1 for u in s if N.bits(0.25) <= u < N.bits(4.0)) >= 30000


def test_exp_inputs():
    ties = N.exp_rint_ties()
    # about 0.69 binary32 per half-integer map onto it: well over half of the 278 are found
    assert len(ties) >= 150, len(ties)
    for x in ties:
        h = N.val(N.f_mul(x, N.LOG2E))
        assert h - np.floor(h) == 0.5
    x = N.f64(N.inputs("exp")[:, 0])
    assert ((x > 88.7228317) & (x < 88.73)).sum() >= 4 and ((x <= 88.7228317) & (x > 88.72)).sum() >= 4
    assert ((x < -103.972076) & (x > -103.973)).sum() >= 4 and ((x >= -103.972076) & (x < -103.971)).sum() >= 4
    with np.errstate(all="ignore"):
        y = np.exp(x)
    assert ((y > 0) & (y < 2.0 ** -126)).sum() >= 20000          # the two-step ldexp
    assert ((np.abs(x) < 2.0 ** -126) & (x != 0)).sum() >= 2000


def test_log_acos_sincos_pow_inputs():
    u = N.inputs("log")[:, 0]
    assert ((u > 0) & (u < N.MIN_NORM)).sum() >= 10000 and {N.MIN_NORM - 1, N.MIN_NORM, N.MIN_NORM + 1} <= set(u.tolist())
    m = (u & 0x7FFFFF) | 0x3F000000
    switch = N.bits(0.70710678)
    assert ((m >= switch - 6) & (m < switch)).sum() >= 40 and ((m >= switch) & (m <= switch + 6)).sum() >= 40
    assert {N.PZERO, N.NZERO, N.INF, N.ONE - 1, N.ONE + 1, N.bits(-1.0)} <= set(u.tolist())
    a = set(N.inputs("acos")[:, 0].tolist())
    for k in range(65):
        assert N.ONE - k in a and (N.ONE - k) | N.SIGN in a
    assert {N.HALF - 1, N.HALF, N.HALF + 1, N.ONE + 1, (N.ONE + 1) | N.SIGN, N.PZERO, N.NZERO, 1} <= a
    x = N.f64(N.inputs("sin")[:, 0])
    finite = x[~np.isnan(x)]
    assert np.abs(finite).max() < N.SINCOS_DOMAIN and N.SINCOS_DOMAIN * 1.27323954473516 < 2.0 ** 31
    s = set(N.inputs("sin")[:, 0].tolist())
    for k in range(1, int(N.SINCOS_DOMAIN * 4 / np.pi)):
        c = N.bits(k * np.pi / 4)
        assert {c - 2, c - 1, c, c + 1, c + 2} & s >= {c - 1, c}          # the last may cross the domain's end
    assert ((x >= 0) & (x <= 2 * np.pi)).sum() >= 20000
    p = N.inputs("pow")
    assert (p[:, 1] == N.SRGB_EXPONENT).all() and N.f64(p[:, 0]).max() == 1.0
    assert {N.PZERO, N.ONE - 1, N.ONE, 1} <= set(p[:, 0].tolist())


def test_aces_inputs():
    num, den = N.aces_overflow_points()
    a, b, c, d, _ = N.ACES
    assert N.is_inf(N.f_mul(num, N.f_add(N.f_mul(a, num), b))) and not N.is_inf(
        N.f_mul(num - 1, N.f_add(N.f_mul(a, num - 1), b)))
    assert N.is_inf(N.f_mul(den, N.f_add(N.f_mul(c, den), d))) and not N.is_inf(
        N.f_mul(den - 1, N.f_add(N.f_mul(c, den - 1), d)))
    assert num < den
    # what today's definition gives out of range (include/rt2.h, rt2_resolve_tonemap)
    assert N.aces1(num - 1) == N.ONE and N.aces1(num) == N.ONE        # inf / finite = inf clamps to 1
    assert N.aces1(den) == N.PZERO and N.aces1(N.INF) == N.PZERO      # inf / inf = NaN clamps to 0
    assert N.aces1(N.NINF) == N.PZERO and N.aces1(N.QNAN) == N.PZERO
    assert N.aces1(N.bits(1e6)) == N.ONE and N.aces1(N.NZERO) == N.PZERO and N.aces1(N.bits(-1e-3)) == N.PZERO
    assert N.aces1(N.bits(-5.0)) == N.ONE                              # the rational is positive again below -0.012
    s = set(N.inputs("aces1")[:, 0].tolist())
    assert {num - 1, num, den - 1, den, N.INF, N.NINF, N.QNAN, N.NZERO, N.bits(1e6), 1} <= s


def test_vector_inputs():
    v = N.inputs("normalize")
    ref = N.reference("normalize")
    length = N.reference("length")[:, 0]
    assert (length == N.PZERO).sum() >= 500 and (length == N.INF).sum() >= 500      # |v|^2 under- and overflows
    assert (ref == N.INF).any() and (ref == N.PZERO).any() and ((ref & 0x7FFFFFFF) > N.INF).any()
    zero = ((v[:, :3] & 0x7FFFFFFF) == 0)
    assert (zero.sum(1) == 3).sum() >= 10 and (zero.sum(1) == 2).sum() >= 100        # zero and axis-aligned vectors
    r = N.reference("refract")
    assert (r[:, 3] == 0).sum() >= 50 and (r[:, 3] == 1).sum() >= 50
    ks = []
    for row in N.inputs("refract"):
        if row[3] == N.PZERO and row[4] == N.PZERO and row[5] == N.ONE and row[6] == N.bits(1.5):
            d = N.dot((N.PZERO, N.PZERO, N.ONE), tuple(int(x) for x in row[:3]))
            eta = int(row[6])
            ks.append(N.val(N.f_sub(N.ONE, N.f_mul(N.f_mul(eta, eta), N.f_sub(N.ONE, N.f_mul(d, d))))))
    ks = np.array(ks)
    assert ((ks < 0) & (ks > -1e-5)).sum() >= 20 and ((ks >= 0) & (ks < 1e-5)).sum() >= 20
    m = N.inputs("mix")[:, 6]
    assert (m == N.PZERO).sum() >= 100 and (m == N.ONE).sum() >= 100
    s = N.inputs("smoothstep")
    x, e0, e1 = N.f64(s[:, 2]), N.f64(s[:, 0]), N.f64(s[:, 1])
    up = e0 < e1
    assert ((x == e0) & up).sum() >= 3 and ((x == e1) & up).sum() >= 3
    assert ((x < e0) & up).sum() >= 100 and ((x > e1) & up).sum() >= 100


def test_sky_inputs():
    rows = N.inputs("sky")
    sun = N.normalize(N._v(0.6, 0.3, -0.2))
    assert (rows == np.array(sun, np.uint32)).all(1).any()
    dots = np.array([N.val(N.dot(tuple(int(x) for x in r), sun)) for r in rows])
    assert ((dots > 1.0) & (dots < 1.001)).sum() >= 2 and ((dots < 1.0) & (dots > 0.999999)).sum() >= 2
    assert ((dots < -1.0) & (dots > -1.001)).sum() >= 2 and (dots == 1.0).any()
    with np.errstate(all="ignore"):
        ang = np.arccos(np.clip(dots, -1.0, 1.0))
        glow = np.exp(-ang * 600.0)
    assert ((glow > 0) & (glow < 2.0 ** -126)).sum() >= 300                 # the denormal-glow band
    y = set(rows[:, 1].tolist())
    for edge in (-0.1, 0.8, -0.2):
        assert {N.bits(edge) - 1, N.bits(edge), N.bits(edge) + 1} <= y
    assert {N.PZERO, N.NZERO, 1, N.SIGN | 1} <= y
    assert ((rows & 0x7FFFFFFF) > N.INF).any(1).sum() >= 3


def test_rng_states():
    for r in N.DRAW_ZERO:
        assert N.rnd(N.pcg_state_for_draw(r))[0] == N.PZERO
    for r in N.DRAW_ONE:
        assert r >= (1 << 32) - 128 and N.rnd(N.pcg_state_for_draw(r))[0] == N.ONE
    for r in N.DRAW_BELOW_ONE:
        assert N.rnd(N.pcg_state_for_draw(r))[0] == N.ONE - 1
    assert N.rnd(N.pcg_state_for_draw((1 << 32) - 129))[0] == N.ONE - 1    # the last draw below the tie
    have = set(N.inputs("rnd")[:, 0].tolist())
    assert all(N.pcg_state_for_draw(r) in have for r in N.DRAW_ZERO + N.DRAW_ONE + N.DRAW_BELOW_ONE)
    # the acceptance edge: s = 1 - 2^-24 is the last accepted, 1 and 1 + 2^-23 are rejected
    have = set(N.inputs("rnd_dir")[:, 0].tolist())
    for s, states in N.EDGE_STATES.items():
        assert len(states) >= 3
        for st in states:
            assert st in have and N.rnd_dir_s(st) == s
            assert (N.rnd_dir(st)[4] == 1) == (s == N.ONE - 1)
    long = N.long_trip_states()
    assert len(long) >= 100 and all(N.rnd_dir(st)[4] >= 8 for st in long) and set(long) <= have


# ---------------------------------------------------------------------------
# the oracle against the reference
# ---------------------------------------------------------------------------
def _oracle_run(oraclemod, library=None):
    return lambda op, rows: oraclemod.numerics(op, rows, library=library)


@pytest.mark.parametrize("op", N.ALL_OPS)
def test_oracle_against_the_reference(oraclemod, op):
    failure, measured = N.check_op(op, _oracle_run(oraclemod))
    if measured is not None:
        print(f"\n{op}: measured maximum {measured:.4g}")
    assert failure is None, failure


def test_op_tables_agree(rt2mod, oraclemod):
    assert rt2mod.NUMERICS_OPS == oraclemod.NUMERICS_OPS and set(N.ALL_OPS) == set(oraclemod.NUMERICS_OPS)


def test_opposite_zeros_are_pinned(oraclemod):
    """max(+0, -0) = +0 and min = -0 in either order."""
    z = N.binary_inputs()[N.minmax_zero_rows()]
    assert (oraclemod.numerics("fmax", z)[:, 0] == N.PZERO).all()
    assert (oraclemod.numerics("fmin", z)[:, 0] == N.NZERO).all()
    rows = np.array([[N.NZERO, N.PZERO, N.ONE], [N.PZERO, N.NZERO, N.ONE]], np.uint32)
    assert (oraclemod.numerics("clamp", rows)[:, 0] == N.PZERO).all()


def test_tonemap_out_of_range_is_as_documented(oraclemod):
    """include/rt2.h on rt2_resolve_tonemap: NaN, both infinities and every
    value from the denominator's overflow on give 0; 1e6 and everything up to
    that overflow give 1; a negative input follows the rational."""
    def tm(u):
        a = oraclemod.numerics("aces1", np.array([[u]], np.uint32))[:, :1]
        return int(oraclemod.numerics("srgb1", a)[0, 0])
    num, den = N.aces_overflow_points()
    for u in (N.QNAN, N.INF, N.NINF, den, N.MAX_FIN, N.MAX_FIN | N.SIGN, N.NZERO, N.bits(-1e-3)):
        assert tm(u) == N.PZERO, hex(u)
    for u in (N.bits(1e6), num - 1, num, den - 1, N.bits(-5.0), N.bits(-1e6)):
        assert tm(u) == N.ONE, hex(u)


# ---------------------------------------------------------------------------
# sensitivity: mutated builds of the oracle
# ---------------------------------------------------------------------------
DOT = "static inline float dot(v3 a, v3 b) { return fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)); }"
DOT_OTHER_ORDER = "static inline float dot(v3 a, v3 b) { return fmaf(a.x, b.x, fmaf(a.y, b.y, a.z * b.z)); }"
PINNED = ("exp", "log", "acos", "cos", "sin", "pow")


def _build(oraclemod, tmp_path, name, flags, old=None, new=None):
    src = open(ORACLE_SRC).read()
    if old is not None:
        assert old in src
        src = src.replace(old, new)
    c = tmp_path / f"rt_oracle_{name}.c"
    c.write_text(src)
    so = str(tmp_path / f"liboracle_{name}.so")
    subprocess.run(GCC + flags + ["-o", so, str(c), "-lpthread", "-lm"], check=True)
    return oraclemod.load(so)


def _failures(oraclemod, library, ops):
    run = _oracle_run(oraclemod, library)
    return {op for op in ops if N.check_op(op, run)[0] is not None}


def test_an_unchanged_rebuild_passes(oraclemod, tmp_path):
    lib = _build(oraclemod, tmp_path, "same", ["-ffp-contract=off"])
    assert _failures(oraclemod, lib, N.ALL_OPS) == set()
    for op in N.ALL_OPS:
        assert len(N.bit_differences(op, _oracle_run(oraclemod), _oracle_run(oraclemod, lib))) == 0, op


def test_contraction_is_caught(oraclemod, tmp_path):
    """-ffp-contract=fast fuses the sums of products that §Numerics keeps apart."""
    lib = _build(oraclemod, tmp_path, "contract", ["-ffp-contract=fast"])
    failed = _failures(oraclemod, lib, N.EXACT_OPS)
    assert {"reflect", "mix", "aces1", "refract"} <= failed, failed
    # nothing to fuse there; smoothstep's only candidate is 3 - 2 t, and 2 t is exact
    assert not failed & {"div", "sqrt", "fma", "mul", "add", "sub", "dot", "cross", "smoothstep"}, failed


def test_an_unfused_horner_step_is_caught(oraclemod, tmp_path):
    """RT2PM_FMA as a product and a sum: every pinned function changes bits
    (the comparison the device is held to); the library still stays inside the
    accuracy bounds or not, which is printed."""
    lib = _build(oraclemod, tmp_path, "unfused", ["-ffp-contract=off", "-DRT2PM_FMA(a,b,c)=((a)*(b)+(c))"])
    for op in PINNED + ("srgb1", "sky"):
        n = len(N.bit_differences(op, _oracle_run(oraclemod), _oracle_run(oraclemod, lib)))
        print(f"\n{op}: {n} rows differ from the oracle")
        assert n > 0, op
    print("\noutside the accuracy bounds:", sorted(_failures(oraclemod, lib, PINNED + ("sky",))))
    assert _failures(oraclemod, lib, N.EXACT_OPS) == set()      # the explicit fmaf of dot and cross is not the macro


def test_a_reordered_dot_is_caught(oraclemod, tmp_path):
    lib = _build(oraclemod, tmp_path, "dot", ["-ffp-contract=off"], DOT, DOT_OTHER_ORDER)
    failed = _failures(oraclemod, lib, N.EXACT_OPS)
    assert {"dot", "length", "normalize", "reflect", "refract"} <= failed, failed
