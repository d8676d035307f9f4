// Brute-force render kernel whose triangle filter runs on the matrix cores.
// Included by rt2_render.hip only (one translation unit; internal linkage).
//
// The filter quantities of a ray-triangle test are linear in the ray once
// m = d×o is formed per segment (the triple-product form of sweep_plk):
//     U = E1·m − d·P1,  −V = −E0·m + d·P0,  X = V − U + c·dn = (E0−E1)·m + d·(P1−P0+cN),
//     −tn = −o·N + AN,  dn = d·N = −det
// (E0, E1, N = s·e0, s·e1, s·n; P0, P1 = s·(a×e0), s·(a×e1); AN = s·(a·n);
// c = 1 + 2^-10; s = 2^k with s·max(|e0|,|e1|,|n|)∞ in [1,2)).  So for 32
// rays × 32 triangles each quantity is a matrix product over the ray vector
// (d, m, o, 1): v_mfma_f32_32x32x16_f16 with every value split into two f16
// halves (x ≈ hi + lo; hi·hi + hi·lo + lo·hi in 3 k-slots), an approximation
// to ~2^-18 of the terms' magnitude at 16× the f32 VALU rate.
// The distance term Y = s (tnum − bk·det) is the −tn record times a second
// ray fragment (−(o + bk·d), −1), rebuilt when a lane's bound improves (with
// no usable bound: (−Bmax·d, 0), the det > 0 test).
// The VALU then only reduces the terms of a pair to one pass / reject bit.
// Like the division-free filter it only decides which tests to skip: a term
// above the threshold T implies the reference rejects ("The matrix
// filter"), and every (wave, triangle) with a passing pair runs the exact
// phase (mt_pass3 + mt_exact: the reference arithmetic) for all 64 rays in
// index order — the sequential strict `dst < best` scan's result bit for bit.
//
// Three kernels share this header's records and fragments:
//   render_mfma      (here)               the 5-product form, records read from L2 by every wave
//   render_mfma_k5r  (rt2_k5_resident.h)  the threshold in the K-slots, records resident in LDS
//   render_mfma_k5t  (rt2_k5_tiles.h)     the threshold in the K-slots, records streamed through LDS tiles
// The 16x16x32 record layout (prep_mfma) survives for the filter probe alone.
#pragma once

namespace {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef float f4v __attribute__((ext_vector_type(4)));
typedef float f16v __attribute__((ext_vector_type(16)));

constexpr int kMfmaQ = 5;                   // quantities per triangle: U, -V, X, -tn, dn
constexpr float kMfmaC = 1.0009765625f;     // c = 1 + 2^-10 (the w test's slack, as in F)
constexpr float kMfmaTs = 0x1p-12f;         // T = 2^-12 (Omax + A + 1)
constexpr float kMfmaB = 2.0f;              // distance test active while bestK <= 2 (Omax + A + 1)

// What distinguishes two matrix-filter kernels of one template; everything
// else about a kernel's form is a fact of its template.
struct MfmaSpec {
    int block;
    int waves;       // minimum waves per SIMD the register allocation must allow
    int tail_lanes;  // cooperative drain at <= this many live rays (pool dry)
    bool diag = false;      // count groups / groups with survivors / exact tests, phase clocks (experiment variants only)
    int tile_groups = 0;    // render_mfma_k5t: 32-triangle groups per LDS record tile
    bool fair_prio = false;  // render_mfma_k5r: issue priority (s_setprio) by the rays the wave's slowest lane has
                             // left, quartiles of the rays per pixel (fair share among a SIMD's waves)
    int phase_prio = 0;      // render_mfma_k5r: issue priority by phase (1 products high, 2 exact phase high,
                             // 3 shading high, 4 exact phase and shading high; rt2_k5_resident.h phase_prio)
    bool flow_prio = false;  // render_mfma_k5t: issue priority by the wave's finishing rank in the last tile
    bool kt_lane_w = false;  // the B_q slot's ray factor W per ray (its own mw_y + mw_z), not the wave's maximum
    bool lean = false;       // x, y recomputed from the item, segments counted per wave (fewer VGPRs live across
                             // the sweep)
    bool res_l2 = false;     // render_mfma_k5r: groups beyond the resident kResGroups are read from L2 (global loads
                             // per wave) after the resident ones: scenes of up to 256 groups
    int exact_win = 1;       // render_mfma_k5r: groups per window (at most 64): the products of a window's groups run
                             // back to back and one exact episode follows (rt2_k5_resident.h); 1 = per group
    bool y_skip_last = false;  // render_mfma_k5r, exact_win = 1: no Y rebuild after the sweep's last group (windows
                               // of more than one group never rebuild there)
    bool y_first = false;  // render_mfma_k5r, window path: a sweep's first window runs the Y product too (no ray has a
                           // bound there, so Y is the det > 0 test that U, -V, X imply); false: kt_group<false>, and
                           // the Y fragment is first built after that window
    bool exact_lanes = false;  // render_mfma_k5r, window path: the episode tests per ray, not per wave: the window's
                               // hot triangles are compacted into synthetic groups whose transposed products give
                               // every ray its own pass mask (rt2_k5_resident.h exact_window_lanes)
    bool pair_loop = false;  // render_mfma_k5r, window path: two groups per trip of the products' loop (the second
                             // group's records at immediate offsets, one pointer step per pair) and each group's hot
                             // mask put into its lane of maskv by one v_writelane
    bool cam_park = false;   // render_mfma_k5r without the T1 pieces (no_t1): a pixel's camera end point is computed
                             // once per pixel-frame and parked in the lane's 16 bytes of the wave's own unused T1
                             // piece; a new ray reads it back (rt2_path.h advance<.., PARK>)
    bool cluster_rows = false;  // render_mfma_k5r, one window of every group: the scene's cluster table (rt2_cluster.h)
                                // is followed: a compact cluster no live ray needs is skipped, one that at most 32
                                // need is swept in the one-block form with those rays moved into one fragment
                                // (rt2_k5_resident.h sweep_kt_res; DESIGN.md "Compact clusters")
    bool cluster_rows16 = false;  // with cluster_rows: a compact cluster that at most 16 rays need is swept with 16-row
                                  // products (v_mfma_f32_16x16x32_f16: 4 accumulator registers instead of 16), six per
                                  // group for the triangles' two halves (kt_group16; DESIGN.md "16-row products")
    bool cluster_rows8 = false;  // with cluster_rows16: a compact cluster that at most 8 rays need is swept with one
                                 // 16-row fragment that holds each ray twice, [ray | 0] in rows 0..7 and [0 | ray] in
                                 // rows 8..15: three products per group give both triangle halves (kt_group8;
                                 // DESIGN.md "8-row products")
    bool slot_order = false;  // with cluster_rows and exact_lanes: RenderParams::mfma_kt_frag is the scene's slot image
                              // (records, table, triangles and slot_tri of the triangles in slot order); the episode
                              // breaks distance ties by the triangles' indices and the sweep returns an index
                              // (rt2_k5_resident.h slot_image; DESIGN.md "Slot order")
    bool linear = false;  // the linear sink (rt2_render_linear; rt2_path.h end_path_linear)
    bool exact_spread = false;  // with exact_lanes in a kernel without the T1 pieces: after every lane's first pair of
                                // a round, the pairs that are left are dealt out one per lane through a list in LDS
                                // and merged by a 64-bit minimum (rt2_k5_resident.h exact_spread_scan; DESIGN.md
                                // "Leftover pairs on all lanes")
    bool spread_drop = false;   // with exact_spread, one experiment arm (the tests' negative control): a spread round's
                                // last list entry is not tested
};

// per-wave diagnostic counts (wave-uniform; MfmaSpec::diag)
struct MfmaDiag {
    unsigned long long groups = 0, hot = 0, exact = 0;
    // `unused1` is not read, and `xl` only by sweep_kt_res's diagnostic
    // builds.  They keep the struct's 15 words and its members' places:
    // kernels built without diag never touch a MfmaDiag, yet its size changes
    // the registers the compiler assigns in them (the same instructions on
    // other registers), and with this layout their code is the code
    // DESIGN.md's measurements are of.
    // sweep_kt_res, per exact episode: [0] (ray, triangle) pairs that pass the
    // filter's U, -V, X conditions (exact_window: evaluated on the exact
    // quantities; exact_window_lanes: the bits of the rays' masks), summed
    // over the lanes; [1] the largest such count of one lane (exact_window_
    // lanes: the per-lane loop's iterations), summed over the episodes; [2]
    // rounds of 32 hot triangles; [3] the largest [1] of one episode
    unsigned long long xl[4] = {};
    // shader clocks (s_memtime) per wave: waiting for a tile (render_mfma_k5r:
    // the sweep's ray setup), the products (with the records' LDS reads), the
    // exact phase (with the Y rebuilds), the whole sweep
    unsigned long long t_wait = 0, t_filt = 0, t_exact = 0, t_swp = 0;
    unsigned long long unused1 = 0;
    // sweep_kt_flow, of that: issuing the wave's tile shares, waiting for them to land; shares issued.
    // sweep_kt_res, of t_exact: waiting for an episode's first triangle to load, the Y rebuilds; exact episodes
    unsigned long long t_issue = 0, t_pub = 0, claims = 0;
};

// Filter coefficients of padded triangle i (binary64, from the pre-transformed
// f32 triangle) and its record scale tau (a power of two that puts the largest
// coefficient in [2^13, 2^14)).  A triangle outside the validated range (as
// sweep_plk's: |a_i| <= 2^20, e0/e1/n components 0 or in [2^-100, 2^20], max
// >= 2^-30; non-finite) gets all-zero coefficients, which always pass (the
// exact test decides); padding triangles get -tn = +2^13, which never passes
// in the form that evaluates -tn.  The forms without it (the threshold in the
// K-slots) let padding pairs through (U = V = X = 0, Y <= 0); their exact
// phase stops at idx >= n_tris before any triangle is read, so a padding slot
// is never tested (tests/test_gpu_mfma.py test_range_edges: 1, 37 and 302
// triangles, bit-exact on every variant).
// flags[0] += out-of-range triangles, flags[1] = max |a_i| (float bits).
// Shared by every record layout (prep_mfma_k16, prep_mfma_kt, prep_mfma).
struct MfmaCoef {
    double c[kMfmaQ][10];  // quantity x ray slot (d.xyz, m.xyz, o.xyz, 1)
    double tau;
};
__device__ __forceinline__ void mfma_coefs(const float4* tri, int i, int n, MfmaCoef& k, uint32_t* flags) {
    for (int q = 0; q < kMfmaQ; q++)
        for (int c = 0; c < 10; c++) k.c[q][c] = 0.0;
    k.tau = 1.0;
    if (i >= n) {
        k.c[3][9] = 0x1p13;  // padding: -tn' = 2^13 sigma > T
        return;
    }
    const float4 t0 = tri[3 * i], t1 = tri[3 * i + 1], t2 = tri[3 * i + 2];
    const float a[3] = {t0.x, t0.y, t0.z}, e0[3] = {t0.w, t1.x, t1.y}, e1[3] = {t1.z, t1.w, t2.x},
                nn[3] = {t2.y, t2.z, t2.w};
    bool ok = true;
    float A = 0.0f, M = 0.0f;
    for (int j = 0; j < 3; j++) {
        ok = ok && fabsf(a[j]) <= 0x1p20f;
        A = fmaxf(A, fabsf(a[j]));
        for (float x : {e0[j], e1[j], nn[j]}) {
            const float ax = fabsf(x);
            ok = ok && (x == 0.0f || (ax >= 0x1p-100f && ax <= 0x1p20f));
            M = fmaxf(M, ax);
        }
    }
    ok = ok && M >= 0x1p-30f;
    if (!ok) {
        atomicAdd(&flags[0], 1u);
        return;
    }
    int ex;
    (void)frexpf(M, &ex);
    const double s = ldexp(1.0, 1 - ex);
    double E0[3], E1[3], N[3], P0[3], P1[3], A0[3];
    for (int j = 0; j < 3; j++) {
        E0[j] = s * e0[j];
        E1[j] = s * e1[j];
        N[j] = s * nn[j];
        A0[j] = a[j];
    }
    P0[0] = A0[1] * E0[2] - A0[2] * E0[1];
    P0[1] = A0[2] * E0[0] - A0[0] * E0[2];
    P0[2] = A0[0] * E0[1] - A0[1] * E0[0];
    P1[0] = A0[1] * E1[2] - A0[2] * E1[1];
    P1[1] = A0[2] * E1[0] - A0[0] * E1[2];
    P1[2] = A0[0] * E1[1] - A0[1] * E1[0];
    const double AN = A0[0] * N[0] + A0[1] * N[1] + A0[2] * N[2];
    for (int j = 0; j < 3; j++) {
        k.c[0][j] = -P1[j];                                // U: d
        k.c[0][3 + j] = E1[j];                             //    m
        k.c[1][j] = P0[j];                                 // -V: d
        k.c[1][3 + j] = -E0[j];                            //     m
        k.c[2][j] = P1[j] - P0[j] + (double)kMfmaC * N[j];  // X: d
        k.c[2][3 + j] = E0[j] - E1[j];                     //    m
        k.c[3][6 + j] = -N[j];                             // -tn: o
        k.c[4][j] = N[j];                                  // dn: d
    }
    k.c[3][9] = AN;  // -tn: 1
    double mx = 0.0;
    for (int q = 0; q < kMfmaQ; q++)
        for (int c = 0; c < 10; c++) mx = fmax(mx, fabs(k.c[q][c]));
    int e2;
    (void)frexp(mx, &e2);  // mx in [2^(e2-1), 2^e2)
    k.tau = ldexp(1.0, 14 - e2);
    atomicMax(&flags[1], __float_as_uint(A));
}

// The 32 k-slots of one quantity's record: coefficient c < 9 as (hi, hi, lo)
// against the ray's (hi, lo, hi) in slots 3c..3c+2 (hi*hi + hi*lo + lo*hi),
// the constant as (hi, lo) against (sigma, sigma) in slots 27, 28.
__device__ __forceinline__ void mfma_slots(const double* coef, double tau, _Float16 slot[32]) {
    for (int k = 0; k < 32; k++) slot[k] = (_Float16)0.0f;
    for (int c = 0; c < 10; c++) {
        const double v = coef[c] * tau;
        const _Float16 hi = (_Float16)(float)v;
        const _Float16 lo = (_Float16)(float)(v - (double)(float)hi);
        if (c < 9) {
            slot[3 * c] = hi;      // x hi * ray hi
            slot[3 * c + 1] = hi;  // x hi * ray lo
            slot[3 * c + 2] = lo;  // x lo * ray hi
        } else {
            slot[27] = hi;  // * sigma
            slot[28] = lo;  // * sigma
        }
    }
}

__device__ __forceinline__ float wave_max(float x) {
    for (int off = 32; off > 0; off >>= 1) x = fmaxf(x, __shfl_xor(x, off));
    return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x)));
}
// The same maximum through DPP lane moves (no LDS crossbar round trips):
// quad swaps, half-row and row mirrors leave every lane of a 16-lane row with
// the row's maximum; row_bcast:15 / :31 fold rows 0-1 and 2-3 and then the
// halves into row 3, whose lane 63 is read.  Exact (a maximum of the same
// values in another order); x must not be NaN (the callers' values are
// finite, or range-checked before).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_max_step(float x) {
    // rows outside ROW_MASK keep `old` = x: max(x, x) = x
    const int y = __builtin_amdgcn_update_dpp(__float_as_int(x), __float_as_int(x), CTRL, ROW_MASK, 0xf, false);
    return fmaxf(x, __int_as_float(y));
}
__device__ __forceinline__ float wave_max_dpp(float x) {
    x = dpp_max_step<0xB1, 0xf>(x);   // quad_perm [1,0,3,2]
    x = dpp_max_step<0x4E, 0xf>(x);   // quad_perm [2,3,0,1]
    x = dpp_max_step<0x141, 0xf>(x);  // row_half_mirror
    x = dpp_max_step<0x140, 0xf>(x);  // row_mirror
    x = dpp_max_step<0x142, 0xa>(x);  // row_bcast:15 into rows 1, 3
    x = dpp_max_step<0x143, 0xc>(x);  // row_bcast:31 into rows 2, 3
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 63));
}

__device__ __forceinline__ float abs_max3(const f3& v) { return fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fabsf(v.z)); }

// Per-wave, per-segment scales of the matrix filter (shared by every sweep
// and by the filter probe): sigma puts the rays' largest |o|, |m| and
// |o + bk d| for every usable bound in [2^13, 2^14); Tw = sigma * T with
// T = 2^-12 (Omax + A + 1); Bmax = the largest usable distance bound.
// False (wave-uniform) when a ray is outside the filter's range: the caller
// computes the wave's rays with the cooperative drain's code.
// DPP: the wave maxima by wave_max_dpp (the kernels with register fragments);
// render_mfma takes wave_max.
struct MfmaScale {
    float sigma, Tw, Bmax;
};
template <bool DPP>
__device__ __forceinline__ bool mfma_scale(float mfma_A, const f3& o, const f3& d, const f3& m, MfmaScale& sc) {
    if (__ballot(!(abs_max3(o) <= 0x1p20f && abs_max3(d) <= 1.0001f))) return false;  // NaN fails too
    const float Omax = DPP ? wave_max_dpp(abs_max3(o)) : wave_max(abs_max3(o));
    const float R0 = Omax + mfma_A + 1.0f;
    float mx = fmaxf(fmaxf(Omax, DPP ? wave_max_dpp(abs_max3(m)) : wave_max(abs_max3(m))), 1.0f);
    mx = fmaxf(mx, __builtin_fmaf(2.25f, R0, Omax));  // |o + bk d| for every bk <= Bmax
    int ex;
    (void)frexpf(mx, &ex);
    sc.sigma = ldexpf(1.0f, 14 - ex);  // sigma * mx in [2^13, 2^14)
    sc.Tw = sc.sigma * (kMfmaTs * R0);
    sc.Bmax = kMfmaB * R0;
    return true;
}

// This lane's ray vector (sigma-scaled d, m, o, 1) as the 32 f16 k-slots
// (hi, lo, hi per component against the records' hi, hi, lo), stored as four
// 16-byte pieces at `row`.
__device__ __forceinline__ void mfma_main_row(_Float16* row, const f3& d, const f3& m, const f3& o, float sigma) {
    const float comp[9] = {d.x, d.y, d.z, m.x, m.y, m.z, o.x, o.y, o.z};
    _Float16 s[32];
#pragma unroll
    for (int c = 0; c < 9; c++) {
        const float v = comp[c] * sigma;
        const _Float16 hi = (_Float16)v;
        const _Float16 lo = (_Float16)(v - (float)hi);
        s[3 * c] = hi;
        s[3 * c + 1] = lo;
        s[3 * c + 2] = hi;
    }
    s[27] = s[28] = (_Float16)sigma;
    s[29] = s[30] = s[31] = (_Float16)0.0f;
    h8* r = reinterpret_cast<h8*>(row);
#pragma unroll
    for (int k = 0; k < 4; k++)
        r[k] = h8{s[8 * k], s[8 * k + 1], s[8 * k + 2], s[8 * k + 3], s[8 * k + 4], s[8 * k + 5], s[8 * k + 6],
                  s[8 * k + 7]};
}

// The Y fragment's k-slots 16..31 for this lane's distance bound bkv: w = o +
// bkv d (bkv <= Bmax) with the constant slot -sigma, so that the -tn record
// gives Y = w.N - AN = s (tnum - bkv det); or, with no usable bound, w = Bmax d
// and constant 0: Y = -s Bmax det (the det > 0 test).  -w sigma as f16 hi/lo
// in the o slots (18..26, hi lo hi like the main fragment); slots 0..15 are 0.
__device__ __forceinline__ void mfma_y_chunk(_Float16 s[16], const f3& d, const f3& o, float bkv, float sigma,
                                             float Bmax) {
    const bool fin = bkv <= Bmax;
    const float wx = fin ? __builtin_fmaf(bkv, d.x, o.x) : Bmax * d.x;
    const float wy = fin ? __builtin_fmaf(bkv, d.y, o.y) : Bmax * d.y;
    const float wz = fin ? __builtin_fmaf(bkv, d.z, o.z) : Bmax * d.z;
    const float wc[3] = {wx, wy, wz};
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float v = -wc[c] * sigma;
        const _Float16 hi = (_Float16)v;
        const _Float16 lo = (_Float16)(v - (float)hi);
        s[2 + 3 * c] = hi;
        s[3 + 3 * c] = lo;
        s[4 + 3 * c] = hi;
    }
    s[0] = s[1] = (_Float16)0.0f;  // slots 16, 17: m.z (zero here)
    s[11] = s[12] = (_Float16)(fin ? -sigma : 0.0f);
    s[13] = s[14] = s[15] = (_Float16)0.0f;
}

// ---------------------------------------------------------------------------
// The k16 records and render_mfma's 5-product sweep on v_mfma_f32_32x32x16_f16.
// The ray vector's 32 slots are two K-halves: [d (9), m.x m.y m.z-hi (7)] and
// [m.z lo/hi (2), o (9), constant (2), 0 (3)].  U, -V and X use d and m (18
// slots); the 5-product form takes them from the first K-half only and bounds
// the two m.z slots left out per (wave, triangle) in the threshold (DESIGN.md,
// "The 5-product form"); -tn uses o and the constant (second half only) and Y
// the second half of its own fragment: one product each.
// Operand maps (32x32x16, K = 16): lane l holds A[row l&31][k 8(l>>5)+j] and
// B[k 8(l>>5)+j][col l&31]; D: column l&31 in all 16 registers (rows
// 8(i>>2) + 4(l>>5) + (i&3)), so every term a lane holds belongs to triangle
// 32G + (l&31): min over them, one ballot, lanes l and l+32 share a triangle.
// Records: [32-group][op][lane][8 f16], ops U0 U1 V0 V1 X0 X1 T1 (7 KiB per 32
// triangles; the probe's 8-product layout reads all seven); tau per triangle.
constexpr int kK16Ops = 7;

struct MfmaK16Lds {
    // slots 0..31: the main fragment; 32..47: the Y fragment's slots 16..31
    // (112-B rows: 16-B reads of 16 consecutive rows hit distinct banks)
    _Float16 ray[64][56];
};
// ... and the path state a lane does not need during the sweep, field-major
// (one 256-B row per field: conflict-free)
constexpr int kLaneStash = 20;
struct MfmaK16LaneLds : MfmaK16Lds {
    uint32_t lane[kLaneStash][64];
};
__device__ __forceinline__ void lane_stash(const Lane& L, uint32_t (*st)[64], int l) {
    const uint32_t v[kLaneStash] = {(uint32_t)L.st, L.item, (uint32_t)L.x, (uint32_t)L.y, L.frame, L.seed,
                                    (uint32_t)L.ray, (uint32_t)L.bounce, (uint32_t)L.inside,
                                    __float_as_uint(L.rayColor.x), __float_as_uint(L.rayColor.y),
                                    __float_as_uint(L.rayColor.z), __float_as_uint(L.incoming.x),
                                    __float_as_uint(L.incoming.y), __float_as_uint(L.incoming.z),
                                    __float_as_uint(L.colorCum.x), __float_as_uint(L.colorCum.y),
                                    __float_as_uint(L.colorCum.z), L.segs, 0u};
#pragma unroll
    for (int f = 0; f < kLaneStash; f++) st[f][l] = v[f];
}
__device__ __forceinline__ void lane_unstash(Lane& L, const uint32_t (*st)[64], int l) {
    L.st = (int)st[0][l];
    L.item = st[1][l];
    L.x = (int)st[2][l];
    L.y = (int)st[3][l];
    L.frame = st[4][l];
    L.seed = st[5][l];
    L.ray = (int)st[6][l];
    L.bounce = (int)st[7][l];
    L.inside = st[8][l] != 0;
    L.rayColor = mk(__uint_as_float(st[9][l]), __uint_as_float(st[10][l]), __uint_as_float(st[11][l]));
    L.incoming = mk(__uint_as_float(st[12][l]), __uint_as_float(st[13][l]), __uint_as_float(st[14][l]));
    L.colorCum = mk(__uint_as_float(st[15][l]), __uint_as_float(st[16][l]), __uint_as_float(st[17][l]));
    L.segs = st[18][l];
}
// ds_permute of a lane's whole path state to lane to/4 (push; a permutation)
__device__ __forceinline__ int perm_i(int to, int v) { return __builtin_amdgcn_ds_permute(to, v); }
__device__ __forceinline__ float perm_f(int to, float v) { return __int_as_float(__builtin_amdgcn_ds_permute(to, __float_as_int(v))); }
__device__ __forceinline__ f3 perm_f3(int to, const f3& v) { return mk(perm_f(to, v.x), perm_f(to, v.y), perm_f(to, v.z)); }
// XY = false: the caller does not keep x, y (advance<S, false>); SEGS = false:
// nor the per-lane segment count (MfmaSpec::lean)
template <bool XY = true, bool SEGS = true>
__device__ __forceinline__ void lane_permute(Lane& L, int to) {
    L.st = perm_i(to, L.st);
    L.item = (uint32_t)perm_i(to, (int)L.item);
    if constexpr (XY) {
        L.x = perm_i(to, L.x);
        L.y = perm_i(to, L.y);
    }
    L.frame = (uint32_t)perm_i(to, (int)L.frame);
    L.seed = (uint32_t)perm_i(to, (int)L.seed);
    L.ray = perm_i(to, L.ray);
    L.bounce = perm_i(to, L.bounce);
    L.inside = perm_i(to, (int)L.inside) != 0;
    L.o = perm_f3(to, L.o);
    L.d = perm_f3(to, L.d);
    L.rayColor = perm_f3(to, L.rayColor);
    L.incoming = perm_f3(to, L.incoming);
    L.colorCum = perm_f3(to, L.colorCum);
    if constexpr (SEGS) L.segs = (uint32_t)perm_i(to, (int)L.segs);
}

// bnd_out: per triangle, the largest |slot 16| and |slot 17| over U, -V, X —
// the m.z products hi x ray-lo and lo x ray-hi that the 5-product form leaves
// out (sweep_k16 adds their bound to the threshold)
__global__ void prep_mfma_k16(const float4* tri, int n, int n_pad, _Float16* out, float* tau_out, float2* bnd_out,
                              uint32_t* flags) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pad) return;
    MfmaCoef k;
    mfma_coefs(tri, i, n, k, flags);
    const int G = i >> 5, t = i & 31;
    float ch = 0.0f, cl = 0.0f;
    for (int op = 0; op < kK16Ops; op++) {
        const int q = op < 6 ? op >> 1 : 3, h = op < 6 ? (op & 1) : 1;
        _Float16 slot[32];
        mfma_slots(k.c[q], k.tau, slot);
        if (op == 6) {
            // the threshold slots 29..31 of the -tn record (zero in every ray
            // fragment but the probe's mfma_thr_frag): -tau, -CH, -CL, all
            // exact in f16 (tau a power of two in [2^-9, 2^13]; CH, CL f16
            // magnitudes)
            slot[29] = (_Float16)(float)-k.tau;
            slot[30] = (_Float16)-ch;
            slot[31] = (_Float16)-cl;
        }
        for (int j = 0; j < 16; j++)
            out[((size_t)(G * kK16Ops + op) * 64 + t + 32 * (j >> 3)) * 8 + (j & 7)] = slot[16 * h + j];
        if (op < 6) {
            ch = fmaxf(ch, fabsf((float)slot[16]));
            cl = fmaxf(cl, fabsf((float)slot[17]));
        }
    }
    tau_out[i] = (float)k.tau;
    if (bnd_out) bnd_out[i] = make_float2(ch, cl);
}

// f16 of v > 0 rounded up (the threshold may only grow)
__device__ __forceinline__ _Float16 f16_up(float v) {
    _Float16 h = (_Float16)v;
    if ((float)h < v) h = __builtin_bit_cast(_Float16, (uint16_t)(__builtin_bit_cast(uint16_t, h) + 1u));
    return h;
}

// The MFMA A-operand fragments of both 32-ray blocks from each lane's own 16
// k-slots s[0..15] (lane l = ray l): block R's lane l holds ray 32R + (l & 31),
// k-slots 8 (l >> 5) .. +7 — what a fragment row's ds_read_b128 gives.
// v_permlane32_swap(x, y) swaps x's lanes 32..63 with y's lanes 0..31, so with
// x = slots 0..7 and y = slots 8..15: x becomes block 0's fragment (lanes
// 0..31 their own slots 0..7, lanes 32..63 the slots 8..15 of rays 0..31) and
// y block 1's.
__device__ __forceinline__ void frag_pair(const _Float16* s, h8 out[2]) {
    typedef uint32_t u4 __attribute__((ext_vector_type(4)));
    const u4 lo = __builtin_bit_cast(u4, h8{s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7]});
    const u4 hi = __builtin_bit_cast(u4, h8{s[8], s[9], s[10], s[11], s[12], s[13], s[14], s[15]});
    u4 r0, r1;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const auto r = __builtin_amdgcn_permlane32_swap(lo[k], hi[k], false, false);
        r0[k] = r[0];
        r1[k] = r[1];
    }
    out[0] = __builtin_bit_cast(h8, r0);
    out[1] = __builtin_bit_cast(h8, r1);
}

// ---------------------------------------------------------------------------
// The threshold in the K-slots (render_mfma_k5r, render_mfma_k5t; DESIGN.md
// "The threshold in the K-slots").  The threshold is two k-slots of the
// products themselves:
//   - U, -V, X keep d (9 slots), m.x (3) and the hi x hi products of m.y and
//     m.z; the four cross slots of m.y and m.z (coefficient hi x ray lo,
//     coefficient lo x ray hi) are left out and bounded, per component c, by
//     2^-10 CT_c mw_c with CT_c = max(|c_hi|, 2^11 |c_lo|) (triangle) and
//     mw_c = max(|r_hi|, 2^11 |r_lo|) (ray): |c_hi r_lo| <= CT 2^-11 mw and
//     |c_lo r_hi| <= 2^-11 CT mw.  Summed over y and z, <= B_q W with
//     B_q = 2^-10 max(CT_y, CT_z) of the quantity's own coefficients and
//     W = mw_y + mw_z of the ray (MfmaSpec::kt_lane_w) or its maximum over
//     the wave;
//   - slot 14 carries -tau against Tw' = Tw (1 + 2^-8) rounded up to f16, and
//     slot 15 -B_q (rounded up in magnitude) against W' = W (1 + 2^-8) rounded
//     up, so each product comes out as its kept sum minus (tau Tw' + B_q W');
//   - Y's fragment carries Tw' in slot 29 against the -tn record's -tau.
// A pair passes iff all four terms are negative: the sign bit of U & V & X & Y
// (two v_bitop3_b32), ORed over the lane's 16 pairs (all one triangle); the 8
// products per group take a zero accumulator and are independent.
// Records: [32-group][4: U, -V, X (first K-half), T1 (-tn second half)][64][8].
constexpr int kKtOps = 4;
__global__ void prep_mfma_kt(const float4* tri, int n, int n_pad, _Float16* out, uint32_t* flags) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pad) return;
    MfmaCoef k;
    mfma_coefs(tri, i, n, k, flags);
    const int G = i >> 5, t = i & 31;
    for (int op = 0; op < kKtOps; op++) {
        _Float16 slot[32], h[16];
        if (op < 3) {
            mfma_slots(k.c[op], k.tau, slot);
            // slots 12, 13, 14: m.y (hi, hi, lo); 15, 16, 17: m.z (hi, hi, lo)
            const float ct = fmaxf(fmaxf(fabsf((float)slot[12]), 2048.0f * fabsf((float)slot[14])),
                                   fmaxf(fabsf((float)slot[15]), 2048.0f * fabsf((float)slot[17])));
            for (int j = 0; j < 13; j++) h[j] = slot[j];  // d (0..8), m.x (9..11), m.y hi x hi (12)
            h[13] = slot[15];                             // m.z hi x hi
            h[14] = (_Float16)(float)-k.tau;              // a power of two in [2^-9, 2^13]: exact
            h[15] = -f16_up(ct * 0x1p-10f);               // B_q, rounded up in magnitude
        } else {
            mfma_slots(k.c[3], k.tau, slot);
            for (int j = 0; j < 16; j++) h[j] = slot[16 + j];  // o (18..26), the constant (27, 28)
            h[13] = (_Float16)(float)-k.tau;                    // slot 29 against Y's Tw'
            h[14] = h[15] = (_Float16)0.0f;
        }
        for (int j = 0; j < 16; j++) out[((size_t)(G * kKtOps + op) * 64 + t + 32 * (j >> 3)) * 8 + (j & 7)] = h[j];
    }
}

// This lane's first K-half of the main fragment: d and m.x as (hi, lo, hi),
// m.y hi, m.z hi; slots 14, 15 (Tw', W') are filled by the caller.  Returns
// the lane's mw_y + mw_z.
__device__ __forceinline__ float kt_main_slots(_Float16 s[16], const f3& d, const f3& m, float sigma) {
    const float comp[4] = {d.x, d.y, d.z, m.x};
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const float v = comp[c] * sigma;
        const _Float16 hi = (_Float16)v;
        const _Float16 lo = (_Float16)(v - (float)hi);
        s[3 * c] = hi;
        s[3 * c + 1] = lo;
        s[3 * c + 2] = hi;
    }
    float W = 0.0f;
    const float yz[2] = {m.y, m.z};
#pragma unroll
    for (int c = 0; c < 2; c++) {
        const float v = yz[c] * sigma;
        const _Float16 hi = (_Float16)v;
        const _Float16 lo = (_Float16)(v - (float)hi);
        s[12 + c] = hi;
        W += fmaxf(fabsf((float)hi), 2048.0f * fabsf((float)lo));
    }
    return W;
}

// The wave's fragments: a0 (both 32-ray blocks' first K-half with the
// threshold factors) and y1 via frag_pair; tw16 keeps Tw' for the Y rebuilds.
// LANE_W (MfmaSpec::kt_lane_w): each ray's fragment carries its own mw_y +
// mw_z (the bound is per (ray, triangle) product: no wave maximum needed).
template <bool LANE_W>
__device__ __forceinline__ void kt_frags(const f3& d, const f3& m, const MfmaScale& sc, h8 a0[2], _Float16& tw16) {
    constexpr float pad = 1.00390625f;  // 1 + 2^-8 (the f32 sum mw_y + mw_z and the scale product round)
    _Float16 s[16];
    const float Wl = kt_main_slots(s, d, m, sc.sigma);
    const float W = LANE_W ? Wl : wave_max_dpp(Wl);
    tw16 = f16_up(sc.Tw * pad);
    s[14] = tw16;
    s[15] = f16_up(W * pad);
    frag_pair(s, a0);
}
__device__ __forceinline__ void kt_y(const f3& d, const f3& o, float bkv, const MfmaScale& sc, _Float16 tw16,
                                     h8 y1[2]) {
    _Float16 s[16];
    mfma_y_chunk(s, d, o, bkv, sc.sigma, sc.Bmax);
    s[13] = tw16;  // slot 29: Tw' against the record's -tau
    frag_pair(s, y1);
}

// One group's filter for the wave's one or two 32-ray blocks (records bu, bv,
// bx: U, -V, X; bt: the -tn record's second K-half).  Returns the ballot of
// lanes whose triangle has a passing pair.  The two blocks are interleaved so
// that each wave's own products run beside its own reduction VALU, at a
// register peak of 48 product VGPRs: [U0 V0 X0] [AND0] [Y0 U1] [fold0] [V1 X1]
// [AND1] [Y1] [fold1] (scheduling groups; one basic block per form).
// Y = false: the form without the distance term, for a stretch of groups in
// which no ray has a bound yet (y1, bt are not read).  Y is then -s Bmax det
// minus its threshold, the det > 0 test, and U, -V, X < 0 already say 0 <
// u_num + v_num < c det (DESIGN.md "No Y product without a bound"): the
// conjunction without Y passes every pair the one with Y passes.  Three
// products per block, the same 16 ANDs, and an OR chain of 8 three-input steps
// over their results: [U0 V0 X0] [AND0] [U1] [or0] [V1 X1] [AND1] [or1].
template <bool Y = true>
__device__ __forceinline__ unsigned long long kt_group(const h8* a0, const h8* y1, const h8& bu, const h8& bv,
                                                       const h8& bx, const h8& bt, bool upper) {
    const f16v zero = {};
    int acc = 0;
    auto andv = [](const f16v& U, const f16v& V, const f16v& X, int* t3) {
#pragma unroll
        for (int i = 0; i < 16; i++)  // U & V & X (LUT index 4 S0 + 2 S1 + S2)
            t3[i] = __builtin_amdgcn_bitop3_b32(__float_as_int(U[i]), __float_as_int(V[i]), __float_as_int(X[i]), 0x80);
    };
    auto fold = [&](const int* t3, const f16v& Yt, int a) {
#pragma unroll
        for (int i = 0; i < 16; i++)  // (t3 & Y) | a: one chain, no OR tree (which costs 0.5 more per pair)
            a = __builtin_amdgcn_bitop3_b32(t3[i], __float_as_int(Yt[i]), a, 0xEA);
        return a;
    };
    auto orv = [](const int* t3, int a) {
#pragma unroll
        for (int i = 0; i < 8; i++)  // t3[2i] | t3[2i + 1] | a
            a = __builtin_amdgcn_bitop3_b32(t3[2 * i], t3[2 * i + 1], a, 0xFE);
        return a;
    };
    if constexpr (!Y) {
        if (upper) {
            int t0[16], t1[16];
            const f16v U0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0[0], bu, zero, 0, 0, 0);
            const f16v V0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0[0], bv, zero, 0, 0, 0);
            const f16v X0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0[0], bx, zero, 0, 0, 0);
            andv(U0, V0, X0, t0);
            const f16v U1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0[1], bu, zero, 0, 0, 0);
            acc = orv(t0, acc);
            const f16v V1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0[1], bv, zero, 0, 0, 0);
            const f16v X1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0[1], bx, zero, 0, 0, 0);
            andv(U1, V1, X1, t1);
            acc = orv(t1, acc);
            __builtin_amdgcn_sched_group_barrier(0x008, 3, 0);   // MFMA
            __builtin_amdgcn_sched_group_barrier(0x002, 16, 0);  // VALU
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, 8, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, 24, 0);
        } else {
            int t0[16];
            const f16v U0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0[0], bu, zero, 0, 0, 0);
            const f16v V0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0[0], bv, zero, 0, 0, 0);
            const f16v X0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0[0], bx, zero, 0, 0, 0);
            andv(U0, V0, X0, t0);
            acc = orv(t0, acc);
        }
    } else if (upper) {
        int t0[16], t1[16];
        const f16v U0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0[0], bu, zero, 0, 0, 0);
        const f16v V0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0[0], bv, zero, 0, 0, 0);
        const f16v X0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0[0], bx, zero, 0, 0, 0);
        andv(U0, V0, X0, t0);
        const f16v Y0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(y1[0], bt, zero, 0, 0, 0);
        const f16v U1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0[1], bu, zero, 0, 0, 0);
        acc = fold(t0, Y0, acc);
        const f16v V1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0[1], bv, zero, 0, 0, 0);
        const f16v X1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0[1], bx, zero, 0, 0, 0);
        andv(U1, V1, X1, t1);
        const f16v Y1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(y1[1], bt, zero, 0, 0, 0);
        acc = fold(t1, Y1, acc);
        __builtin_amdgcn_sched_group_barrier(0x008, 3, 0);   // MFMA
        __builtin_amdgcn_sched_group_barrier(0x002, 16, 0);  // VALU
        __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 16, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 16, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 16, 0);
    } else {
        int t0[16];
        const f16v U0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0[0], bu, zero, 0, 0, 0);
        const f16v V0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0[0], bv, zero, 0, 0, 0);
        const f16v X0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0[0], bx, zero, 0, 0, 0);
        andv(U0, V0, X0, t0);
        const f16v Y0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(y1[0], bt, zero, 0, 0, 0);
        acc = fold(t0, Y0, acc);
    }
    return __ballot(acc < 0);
}

// MfmaSpec::cluster_rows.  Two groups' filters for ONE 32-ray block `a` (the
// form without Y): the two groups take the places kt_group gives the two
// blocks, so a wave's products still run beside its own fold, at the same
// peak of 48 product registers: [U0 V0 X0] [AND0] [U1] [or0] [V1 X1] [AND1]
// [or1], with an accumulator and a ballot per group.
__device__ __forceinline__ void kt_group_one2(const h8& a, const h8& bu0, const h8& bv0, const h8& bx0, const h8& bu1,
                                              const h8& bv1, const h8& bx1, unsigned long long& M0,
                                              unsigned long long& M1) {
    const f16v zero = {};
    int t0[16], t1[16], acc0 = 0, acc1 = 0;
    const f16v U0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, bu0, zero, 0, 0, 0);
    const f16v V0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, bv0, zero, 0, 0, 0);
    const f16v X0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, bx0, zero, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 16; i++)
        t0[i] = __builtin_amdgcn_bitop3_b32(__float_as_int(U0[i]), __float_as_int(V0[i]), __float_as_int(X0[i]), 0x80);
    const f16v U1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, bu1, zero, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 8; i++) acc0 = __builtin_amdgcn_bitop3_b32(t0[2 * i], t0[2 * i + 1], acc0, 0xFE);
    const f16v V1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, bv1, zero, 0, 0, 0);
    const f16v X1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, bx1, zero, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 16; i++)
        t1[i] = __builtin_amdgcn_bitop3_b32(__float_as_int(U1[i]), __float_as_int(V1[i]), __float_as_int(X1[i]), 0x80);
#pragma unroll
    for (int i = 0; i < 8; i++) acc1 = __builtin_amdgcn_bitop3_b32(t1[2 * i], t1[2 * i + 1], acc1, 0xFE);
    __builtin_amdgcn_sched_group_barrier(0x008, 3, 0);   // MFMA
    __builtin_amdgcn_sched_group_barrier(0x002, 16, 0);  // VALU
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
    __builtin_amdgcn_sched_group_barrier(0x002, 8, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
    __builtin_amdgcn_sched_group_barrier(0x002, 24, 0);
    M0 = __ballot(acc0 < 0);
    M1 = __ballot(acc1 < 0);
}

// MfmaSpec::cluster_rows16.  The filter of 16 rays (the form without Y) by
// v_mfma_f32_16x16x32_f16: A holds row l & 15, B column l & 15, k-slots
// 8 (l >> 4) .. +7 of 32; D is column l & 15, rows 4 (l >> 4) + reg, in 4
// registers.  A record register read through kt16_record_lane holds triangle
// j's 16 slots in the lower K-half of column j and triangle j + 16's in the
// upper one, so two A fragments give the two halves' exact 16-slot sums from
// the one B register: alo = [rays | 0] triangles 0..15, ahi = [0 | rays]
// triangles 16..31 (the other 16 slots add 0 x finite: every f16 of a record is
// finite, rt2_scene_create asserts it).  Per half 4 ANDs and 2 ORs instead of
// 16 and 8; a half's ballot has triangle j in bits j, j + 16, j + 32, j + 48.
__device__ __forceinline__ int kt16_record_lane(int l) { return (l & 15) + 16 * (l >> 5) + 32 * ((l >> 4) & 1); }
__device__ __forceinline__ int kt16_fold(const f4v& U, const f4v& V, const f4v& X) {
    int t[4];
#pragma unroll
    for (int i = 0; i < 4; i++)
        t[i] = __builtin_amdgcn_bitop3_b32(__float_as_int(U[i]), __float_as_int(V[i]), __float_as_int(X[i]), 0x80);
    return __builtin_amdgcn_bitop3_b32(t[0], t[1], t[2], 0xFE) | t[3];
}
__device__ __forceinline__ uint32_t kt16_hot(unsigned long long Mlo, unsigned long long Mhi) {
    const uint32_t lo = (uint32_t)(Mlo | Mlo >> 32), hi = (uint32_t)(Mhi | Mhi >> 32);
    return ((lo | lo >> 16) & 0xffffu) | (hi | hi >> 16) << 16;
}
// one group: its hot mask
__device__ __forceinline__ uint32_t kt_group16(const h8& alo, const h8& ahi, const h8& bu, const h8& bv,
                                               const h8& bx) {
    const f4v zero = {};
    const f4v Ul = __builtin_amdgcn_mfma_f32_16x16x32_f16(alo, bu, zero, 0, 0, 0);
    const f4v Vl = __builtin_amdgcn_mfma_f32_16x16x32_f16(alo, bv, zero, 0, 0, 0);
    const f4v Xl = __builtin_amdgcn_mfma_f32_16x16x32_f16(alo, bx, zero, 0, 0, 0);
    const f4v Uh = __builtin_amdgcn_mfma_f32_16x16x32_f16(ahi, bu, zero, 0, 0, 0);
    const f4v Vh = __builtin_amdgcn_mfma_f32_16x16x32_f16(ahi, bv, zero, 0, 0, 0);
    const f4v Xh = __builtin_amdgcn_mfma_f32_16x16x32_f16(ahi, bx, zero, 0, 0, 0);
    const int al = kt16_fold(Ul, Vl, Xl);
    const int ah = kt16_fold(Uh, Vh, Xh);
    __builtin_amdgcn_sched_group_barrier(0x008, 6, 0);   // MFMA
    __builtin_amdgcn_sched_group_barrier(0x002, 12, 0);  // VALU
    return kt16_hot(__ballot(al < 0), __ballot(ah < 0));
}
// two groups per trip, a half's products beside the fold of the half before:
// [lo0 hi0] [fold lo0] [lo1] [fold hi0] [hi1] [fold lo1] [fold hi1]; at most 36
// product registers live
__device__ __forceinline__ void kt_group16_2(const h8& alo, const h8& ahi, const h8& bu0, const h8& bv0,
                                             const h8& bx0, const h8& bu1, const h8& bv1, const h8& bx1, uint32_t& m0,
                                             uint32_t& m1) {
    const f4v zero = {};
    const f4v Ul0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(alo, bu0, zero, 0, 0, 0);
    const f4v Vl0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(alo, bv0, zero, 0, 0, 0);
    const f4v Xl0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(alo, bx0, zero, 0, 0, 0);
    const f4v Uh0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(ahi, bu0, zero, 0, 0, 0);
    const f4v Vh0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(ahi, bv0, zero, 0, 0, 0);
    const f4v Xh0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(ahi, bx0, zero, 0, 0, 0);
    const int al0 = kt16_fold(Ul0, Vl0, Xl0);
    const f4v Ul1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(alo, bu1, zero, 0, 0, 0);
    const f4v Vl1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(alo, bv1, zero, 0, 0, 0);
    const f4v Xl1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(alo, bx1, zero, 0, 0, 0);
    const int ah0 = kt16_fold(Uh0, Vh0, Xh0);
    const f4v Uh1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(ahi, bu1, zero, 0, 0, 0);
    const f4v Vh1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(ahi, bv1, zero, 0, 0, 0);
    const f4v Xh1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(ahi, bx1, zero, 0, 0, 0);
    const int al1 = kt16_fold(Ul1, Vl1, Xl1);
    const int ah1 = kt16_fold(Uh1, Vh1, Xh1);
    __builtin_amdgcn_sched_group_barrier(0x008, 6, 0);  // MFMA
    __builtin_amdgcn_sched_group_barrier(0x002, 6, 0);  // VALU
    __builtin_amdgcn_sched_group_barrier(0x008, 3, 0);
    __builtin_amdgcn_sched_group_barrier(0x002, 6, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, 3, 0);
    __builtin_amdgcn_sched_group_barrier(0x002, 12, 0);
    m0 = kt16_hot(__ballot(al0 < 0), __ballot(ah0 < 0));
    m1 = kt16_hot(__ballot(al1 < 0), __ballot(ah1 < 0));
}

// MfmaSpec::cluster_rows8.  The filter of 8 rays by one 16-row product per
// quantity: fragment a8 holds ray r < 8 twice, [ray | 0] in row r (lanes r,
// r + 16) and [0 | ray] in row r + 8 (lanes r + 40, r + 56), every other lane
// zero.  Against the record register of kt_group16, D row r is (ray r,
// triangle j) and D row r + 8 is (ray r, triangle j + 16): each term the sum of
// the same 16 f16 products as alo's and ahi's, the other 16 slots adding
// 0 x finite.  Lanes 0..31 of D hold rows 0..7 and lanes 32..63 rows 8..15, so
// one ballot has triangle j in bits j and j + 16 and triangle j + 16 in bits
// j + 32 and j + 48.  3 products, 4 ANDs, 2 ORs and one compare per group.
__device__ __forceinline__ uint32_t kt8_hot(unsigned long long M) {
    const uint32_t lo = (uint32_t)M, hi = (uint32_t)(M >> 32);
    return ((lo | lo >> 16) & 0xffffu) | (hi | hi >> 16) << 16;
}
// one group: its hot mask
__device__ __forceinline__ uint32_t kt_group8(const h8& a8, const h8& bu, const h8& bv, const h8& bx) {
    const f4v zero = {};
    const f4v U = __builtin_amdgcn_mfma_f32_16x16x32_f16(a8, bu, zero, 0, 0, 0);
    const f4v V = __builtin_amdgcn_mfma_f32_16x16x32_f16(a8, bv, zero, 0, 0, 0);
    const f4v X = __builtin_amdgcn_mfma_f32_16x16x32_f16(a8, bx, zero, 0, 0, 0);
    const int a = kt16_fold(U, V, X);
    __builtin_amdgcn_sched_group_barrier(0x008, 3, 0);  // MFMA
    __builtin_amdgcn_sched_group_barrier(0x002, 6, 0);  // VALU
    return kt8_hot(__ballot(a < 0));
}
// two groups per trip, the second group's products beside the first one's
// fold: [g0] [g1] [fold g0] [fold g1]; 24 product registers live
__device__ __forceinline__ void kt_group8_2(const h8& a8, const h8& bu0, const h8& bv0, const h8& bx0, const h8& bu1,
                                            const h8& bv1, const h8& bx1, uint32_t& m0, uint32_t& m1) {
    const f4v zero = {};
    const f4v U0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a8, bu0, zero, 0, 0, 0);
    const f4v V0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a8, bv0, zero, 0, 0, 0);
    const f4v X0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a8, bx0, zero, 0, 0, 0);
    const f4v U1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a8, bu1, zero, 0, 0, 0);
    const f4v V1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a8, bv1, zero, 0, 0, 0);
    const f4v X1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a8, bx1, zero, 0, 0, 0);
    const int a0 = kt16_fold(U0, V0, X0);
    const int a1 = kt16_fold(U1, V1, X1);
    __builtin_amdgcn_sched_group_barrier(0x008, 6, 0);   // MFMA
    __builtin_amdgcn_sched_group_barrier(0x002, 12, 0);  // VALU
    m0 = kt8_hot(__ballot(a0 < 0));
    m1 = kt8_hot(__ballot(a1 < 0));
}

// Closest hit of every lane's ray (o, d) over all triangles, records read
// from L2; the whole wave calls it (lanes without a ray of their own carry a
// copy of a live one).  Five products per 32-ray block: U, -V, X from the
// first K-half, -tn and Y from the second; each block's products, then their
// reduction, with scheduling fences between the phases.  upper = false: lanes
// 32..63 carry no ray of their own (the caller moved the live rays to the
// low half), so the second 32-ray block's products and reduction are skipped.
// Returns false (nothing done) when a ray is outside the bound's range.
__device__ __forceinline__ bool sweep_k16(const RenderParams& p, MfmaK16LaneLds& sh, const f3& o, const f3& d,
                                          float& best, int& bi, float& bestK, bool upper) {
    const int lane = (int)lane_id();
    const int r32 = lane & 31, hl = lane >> 5;
    const f3 m = cross(d, o);
    MfmaScale sc;
    if (!mfma_scale<false>(p.mfma_A, o, d, m, sc)) return false;
    mfma_main_row(&sh.ray[lane][0], d, m, o, sc.sigma);
    // the wave's largest |ray lo| and |ray hi| of m.z (slots 16 and 17 of the
    // main fragment, the same arithmetic as mfma_main_row): with the records'
    // per-triangle |hi|, |lo| of the m.z coefficients they bound the two
    // products the 5-product form leaves out of U, -V and X
    const float vz = m.z * sc.sigma;
    const _Float16 hz = (_Float16)vz;
    const _Float16 lz = (_Float16)(vz - (float)hz);
    const float zhi = wave_max(fabsf((float)hz));
    const float zlo = wave_max(fabsf((float)lz));
    auto write_y = [&](float bkv) {
        _Float16 s[16];
        mfma_y_chunk(s, d, o, bkv, sc.sigma, sc.Bmax);
        h8* row = reinterpret_cast<h8*>(&sh.ray[lane][32]);
        row[0] = h8{s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7]};
        row[1] = h8{s[8], s[9], s[10], s[11], s[12], s[13], s[14], s[15]};
    };
    write_y(bestK);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    h8 a0[2], a1[2], y1[2];
#pragma unroll
    for (int R = 0; R < 2; R++) {
        a0[R] = *reinterpret_cast<const h8*>(&sh.ray[32 * R + r32][8 * hl]);
        a1[R] = *reinterpret_cast<const h8*>(&sh.ray[32 * R + r32][16 + 8 * hl]);
    }
    auto read_y = [&]() {
#pragma unroll
        for (int R = 0; R < 2; R++) y1[R] = *reinterpret_cast<const h8*>(&sh.ray[32 * R + r32][32 + 8 * hl]);
    };
    read_y();

    const int ng = (p.n_tris + 31) >> 5;
    // per-lane record pointers advanced in VGPRs (no per-group reload of the
    // spilled base addresses)
    const h8* fg = reinterpret_cast<const h8*>(p.mfma_k16_frag) + lane;
    const float* tg = p.mfma_k16_tau + r32;
    const float2* bg = p.mfma_k16_bnd + r32;
    for (int G = 0; G < ng; G++) {
        // U0, V0, X0, T1 (the second K-halves of U, V, X are not read)
        const h8 bu = fg[0], bv = fg[64 * 2], bx = fg[64 * 4], bt = fg[64 * 6];
        const float tau = *tg;
        const float2 bnd = *bg;
        bg += 32;
        fg += kK16Ops * 64;
        tg += 32;
        // + |c_hi| max|ray lo| + |c_lo| max|ray hi| of the left-out m.z slots,
        // padded by 2^-10 for its own rounding ("The 5-product form")
        const float Tl = tau * sc.Tw + (bnd.x * zlo + bnd.y * zhi) * 1.0009765625f;
        int tmin = 0x7fffffff;
#pragma unroll
        for (int R = 0; R < 2; R++) {
            if (R == 1 && !upper) break;
            const f16v zero = {};
            const f16v U = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0[R], bu, zero, 0, 0, 0);
            const f16v V = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0[R], bv, zero, 0, 0, 0);
            const f16v X = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0[R], bx, zero, 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            // The max of the terms on their bit patterns as signed integers:
            // negative floats are negative integers, positive floats order
            // like their patterns, so max_int(terms) <= int(Tl) (Tl > 0) iff
            // every term <= Tl; then the min over the lane's 16 pairs (all one
            // triangle) and one compare per group.
            int t3[16];
#pragma unroll
            for (int i = 0; i < 16; i++)
                t3[i] = max(max(__float_as_int(U[i]), __float_as_int(V[i])), __float_as_int(X[i]));
            __builtin_amdgcn_sched_barrier(0);
            const f16v T = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1[R], bt, zero, 0, 0, 0);
            const f16v Y = __builtin_amdgcn_mfma_f32_32x32x16_f16(y1[R], bt, zero, 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 16; i++)
                tmin = min(tmin, max(max(t3[i], __float_as_int(T[i])), __float_as_int(Y[i])));
        }
        const unsigned long long M = __ballot(tmin <= __float_as_int(Tl));
        if (M) {
            // triangles of the group with a passing pair: the exact phase, in index order
            uint32_t m32 = (uint32_t)(M | M >> 32);
            const float bk0 = bestK;
            while (m32) {
                const int t = __builtin_ctz(m32);
                m32 &= m32 - 1;
                const int idx = 32 * G + t;
                if (idx >= p.n_tris) break;
                cfloat* tp = (cfloat*)p.tri + 12 * idx;
                const MtQ qq = mt_quantities(o, d, ldc4(tp), ldc4(tp + 4), ldc4(tp + 8));
                if (mt_pass3(qq, bestK)) mt_exact(qq, idx, best, bi, bestK);
            }
            if (__ballot(bestK != bk0)) {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();  // every lane has read the rows' previous Y slots
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                write_y(bestK);
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                read_y();
            }
        }
    }
    return true;
}

// Closest hit of every ray of `act` (lane j's o, d), one ray at a time by the
// whole wave (coop_closest: the sequential strict-< scan's result); lane j
// receives its own ray's (best, bi), lanes outside `act` keep theirs.
// `bound` (nullable): lane j's starting bound (coop_closest's `bound`).
__device__ __forceinline__ void coop_each(unsigned long long act, const f3& o, const f3& d, const RenderParams& p,
                                          float& best, int& bi, const float* bound = nullptr) {
    while (act) {
        const int j = __builtin_ctzll(act);
        act &= act - 1;
        const f3 oj = mk(__shfl(o.x, j), __shfl(o.y, j), __shfl(o.z, j));
        const f3 dj = mk(__shfl(d.x, j), __shfl(d.y, j), __shfl(d.z, j));
        float b;
        int bidx;
        coop_closest(oj, dj, p.tri, p.n_tris, b, bidx, bound ? __shfl(*bound, j) : 1e38f);
        if ((int)lane_id() == j) {
            best = b;
            bi = bidx;
        }
    }
}

// render_smem's lockstep segment loop (the workgroup's waves start every
// segment together: one barrier per segment) and cooperative drain with
// sweep_k16 as the closest-hit sweep; the lane's path state (all but o, d)
// waits in LDS during the sweep.  A wave whose rays leave the filter's range
// computes them with the cooperative drain's code instead (coop_each).
template <MfmaSpec S>
__global__ __launch_bounds__(S.block) __attribute__((amdgpu_waves_per_eu(S.waves))) void render_mfma(RenderParams p_arg) {
    __shared__ MfmaK16LaneLds wl[S.block / 64];
    MfmaK16LaneLds& sh = wl[threadIdx.x >> 6];
    __shared__ BlockVote<S.block / 64> vote;
    uint32_t vote_parity = 0;
    Lane L;
    lane_init(L);
    for (;;) {
        // the kernel arguments are re-read from the kernarg segment (scalar
        // loads) in every segment instead of being held in SGPRs across the
        // sweep (whose register pressure then spills them to VGPR lanes)
        const RenderParams& p = kargs<RenderParams>();
        advance<1, true, false, false, S.linear>(L, p);
        unsigned long long act = __ballot(L.st == ST_TRACE);
        if (!block_any<S.block / 64>(act != 0, vote, vote_parity)) break;
        if (!act) continue;
        if (__popcll(act) <= (unsigned)S.tail_lanes && __any(L.st == ST_DONE)) {
            float mybest = 1e38f;
            int mybi = -1;
            coop_each(act, L.o, L.d, p, mybest, mybi);
            if (L.st == ST_TRACE) {
                L.bounce += 1;
                L.segs += 1;
                shade<1, false, S.linear>(L, p, mybest, mybi);
            }
            continue;
        }
        // at most 32 live rays: move them to lanes 0..31 (every lane's path
        // state travels with it; lanes are interchangeable), so that the
        // sweep runs the first 32-ray block only
        bool upper = true;
        if (__popcll(act) <= 32) {
            if (act >> 32) {
                const uint32_t l = lane_id(), nl = (uint32_t)__popcll(act);
                const bool live = (act >> l) & 1ull;
                const int to = 4 * (int)(live ? lanes_below(act) : nl + lanes_below(~act));
                lane_permute(L, to);
                act = __ballot(L.st == ST_TRACE);
            }
            upper = false;
        }
        // lanes without a ray carry the first live lane's (their passes add no
        // triangle; such a lane is ST_DONE and never reads its o, d again)
        const int j0 = __builtin_ctzll(act);
        const bool mine = L.st == ST_TRACE;
        {
            const f3 o = mk(__shfl(L.o.x, j0), __shfl(L.o.y, j0), __shfl(L.o.z, j0));
            const f3 dd = mk(__shfl(L.d.x, j0), __shfl(L.d.y, j0), __shfl(L.d.z, j0));
            if (!mine) {
                L.o = o;
                L.d = dd;
            }
        }
        const f3 ro = L.o, rd = L.d;
        float best = 1e38f, bestK = 1e38f * 1.0009765625f;
        int bi = -1;
        // the path state waits in LDS (its registers are free during the sweep)
        lane_stash(L, sh.lane, (int)lane_id());
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        const bool swept = sweep_k16(p, sh, ro, rd, best, bi, bestK, upper);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const f3 lo = L.o, ld = L.d;
        lane_unstash(L, sh.lane, (int)lane_id());
        L.o = lo;
        L.d = ld;
        // a ray outside the filter's range (wave-uniform): the wave computes each
        // live ray's closest hit together (the drain's code, vector loads: no
        // SGPR block of records competing with the sweep's registers)
        if (!swept) coop_each(act, ro, rd, p, best, bi);
        if (mine) {
            L.bounce += 1;
            L.segs += 1;
            shade<1, false, S.linear>(L, p, best, bi);
        }
    }
    flush_counters(L, p_arg);
}

// ---------------------------------------------------------------------------
// Filter probe (test hook rt2_mfma_probe, not part of the render): the five
// filter terms of every (ray, triangle) pair exactly as a product sweep
// computes them — the same scales (mfma_scale), fragments (mfma_main_row,
// mfma_y_chunk, kt_frags), records and MFMA instructions — written out
// instead of reduced, with the operand fragments and the reference's own
// accept decision (mt_quantities + mt_exact against the ray's bound), so the
// host can measure the products' error against a binary64 evaluation of the
// same operands and check the filter's conservativeness on the hardware.
// Besides the forms the render kernels use (layouts 2, 5, 6) it keeps the
// forms the filter grew through (layouts 0, 1, 3, 4), whose error
// budgets the tests still pin; what only they need is defined here.
// One wave per 64 rays (n_rays a multiple of 64).
//   rays:   per ray {o.x, o.y, o.z, best} {d.x, d.y, d.z, 0}
//   terms:  [ray][tri][5] (U, -V, X, -tn, Y; tri < n_pad)
//   frags:  [ray][48] f16: main slots 0..31, Y slots 16..31
//   rinfo:  [ray][8]: in range, sigma, Tw, Bmax, m.x, m.y, m.z, bestK
//   accept: [ray][tri] (tri < n_tris): the reference accepts the pair

// Layout 0's records in the v_mfma_f32_16x16x32_f16 B-operand order (one
// thread per padded triangle): [16-group][quantity][lane][8 f16] (5 KiB per
// 16 triangles) plus a per-triangle scale tau.  Operand maps: A = rays, lane
// l holds ray 16R + (l&15), k-slots 8(l>>4)..+7; B = triangles, lane l holds
// triangle 16G + (l&15), the same k-slots; D: lane l holds rays 16R + 4(l>>4)
// + i (i = 0..3) x triangle l&15.
__global__ void prep_mfma(const float4* tri, int n, int n_pad, _Float16* out, float* tau_out, uint32_t* flags) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pad) return;
    MfmaCoef k;
    mfma_coefs(tri, i, n, k, flags);
    const int G = i >> 4, t = i & 15;
    for (int q = 0; q < kMfmaQ; q++) {
        _Float16 slot[32];
        mfma_slots(k.c[q], k.tau, slot);
        for (int s = 0; s < 32; s++) out[((size_t)(G * kMfmaQ + q) * 64 + 16 * (s >> 3) + t) * 8 + (s & 7)] = slot[s];
    }
    tau_out[i] = (float)k.tau;
}

// Layout 4: mfma_main_row's first K-half only (slots 0..15: d, m.x, m.y, m.z hi)
__device__ __forceinline__ void mfma_main_half_slots(_Float16 s[18], const f3& d, const f3& m, float sigma) {
    const float comp[6] = {d.x, d.y, d.z, m.x, m.y, m.z};
#pragma unroll
    for (int c = 0; c < 6; c++) {
        const float v = comp[c] * sigma;
        const _Float16 hi = (_Float16)v;
        const _Float16 lo = (_Float16)(v - (float)hi);
        s[3 * c] = hi;
        s[3 * c + 1] = lo;
        s[3 * c + 2] = hi;
    }
}

// Layouts 3, 4 (the threshold in the accumulator): the A fragment
// whose product with the -tn record's second K-half is -Tl'' in every row,
// Tl'' = tau Tw + CH ML + CL MH with the wave's factors padded by 2^-8 and
// rounded up to f16 (slots 29..31 against the record's -tau, -CH, -CL; every
// other slot 0).  The three products are exact in f32 and of one sign, so the
// sum's rounding (2^-23) is inside the pad: Tl'' > Tl' = tau Tw + (CH ML + CL
// MH)(1 + 2^-10), sweep_k16's threshold.  Added as the accumulator operand, it
// turns "term <= Tl'" into "term' < 0".  The factors are wave-uniform and kept
// as two scalar words (elements 4, 5 = 0, Tw; 6, 7 = ML, MH of the upper
// lanes' 8 slots).
struct ThrBits {
    uint32_t w2, w3;
};
__device__ __forceinline__ ThrBits mfma_thr_bits(float Tw, float zlo, float zhi) {
    constexpr float pad = 1.00390625f;  // 1 + 2^-8
    const uint32_t t = __builtin_bit_cast(uint16_t, f16_up(Tw * pad));
    const uint32_t a = __builtin_bit_cast(uint16_t, f16_up(zlo * pad));
    const uint32_t b = __builtin_bit_cast(uint16_t, f16_up(zhi * pad));
    return ThrBits{(uint32_t)__builtin_amdgcn_readfirstlane(t << 16), (uint32_t)__builtin_amdgcn_readfirstlane(a | b << 16)};
}
__device__ __forceinline__ h8 mfma_thr_frag(ThrBits tb) {
    typedef uint32_t u4 __attribute__((ext_vector_type(4)));
    const bool up = lane_id() >= 32;  // slots 8..15 of the K-half: 29, 30, 31 are elements 5, 6, 7
    // opaque() outside the selects: an asm value inside a ?: compiled to two
    // exec-masked branches per group instead of two v_cndmask
    const uint32_t w2 = opaque(tb.w2), w3 = opaque(tb.w3);
    const u4 v = {0u, 0u, up ? w2 : 0u, up ? w3 : 0u};
    return __builtin_bit_cast(h8, v);
}

// Layouts 1..3: the five terms of 32 rays (fragments a0/a1 = the main
// fragment's two K-halves, y1 = the Y fragment's second half) x 32 triangles
// (records b[7]), U, -V, X as two chained products each: 8 products per block.
struct K16Terms {
    f16v U, V, X, T, Y;
};
__device__ __forceinline__ K16Terms k16_terms(const h8& a0, const h8& a1, const h8& y1, const h8* b) {
    const f16v zero = {};
    K16Terms r;
    r.U = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b[0], zero, 0, 0, 0);
    r.V = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b[2], zero, 0, 0, 0);
    r.X = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b[4], zero, 0, 0, 0);
    r.U = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b[1], r.U, 0, 0, 0);
    r.V = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b[3], r.V, 0, 0, 0);
    r.X = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b[5], r.X, 0, 0, 0);
    r.T = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b[6], zero, 0, 0, 0);
    r.Y = __builtin_amdgcn_mfma_f32_32x32x16_f16(y1, b[6], zero, 0, 0, 0);
    return r;
}

// LAYOUT: rt2_mfma_probe's (rt2_render.hip) — 0 = the 16x16x32 form, 1 = the
// 8-product k16 form, 2 = the 5-product form, 3 = the 5-product form with the
// threshold in the accumulator, 4 = layout 3 on frag_pair fragments, 5 = the
// threshold in the K-slots, 6 = layout 5 with each ray's own W, 7 = layout 6's
// U, -V, X by the 16-row products (MfmaSpec::cluster_rows16), 8 = the same by
// the 8-row products (MfmaSpec::cluster_rows8).
template <int LAYOUT>
__global__ __launch_bounds__(64) void mfma_probe_kernel(RenderParams p, const float4* rays, int n_pad, float* terms,
                                                        _Float16* frags, float* rinfo, uint8_t* accept) {
    constexpr bool kPerm = LAYOUT >= 4;  // fragments built in registers (frag_pair), wave maxima by DPP
    constexpr bool kKthr = LAYOUT >= 5, kK16 = LAYOUT >= 1 && LAYOUT <= 3, kK5 = LAYOUT == 2 || LAYOUT == 3,
                   kCthr = LAYOUT == 3;
    __shared__ MfmaK16Lds sh;
    const int lane = (int)threadIdx.x;
    const size_t ray = (size_t)blockIdx.x * 64 + lane;
    const float4 r0 = rays[2 * ray], r1 = rays[2 * ray + 1];
    const f3 o = mk(r0.x, r0.y, r0.z), d = mk(r1.x, r1.y, r1.z);
    const float best = r0.w, bestK = best * 1.0009765625f;
    for (int t = 0; t < p.n_tris; t++) {
        cfloat* tp = (cfloat*)p.tri + 12 * t;
        float b = best, bk = bestK;
        int bi = -1;
        mt_exact(mt_quantities(o, d, ldc4(tp), ldc4(tp + 4), ldc4(tp + 8)), t, b, bi, bk);
        accept[ray * p.n_tris + t] = bi == t;
    }
    const f3 m = cross(d, o);
    MfmaScale sc{0.0f, 0.0f, 0.0f};
    const bool ok = mfma_scale<kPerm>(p.mfma_A, o, d, m, sc);
    float* ri = rinfo + ray * 8;
    ri[0] = ok ? 1.0f : 0.0f;
    ri[1] = sc.sigma;
    ri[2] = sc.Tw;
    ri[3] = sc.Bmax;
    ri[4] = m.x;
    ri[5] = m.y;
    ri[6] = m.z;
    ri[7] = bestK;
    if (!ok) return;  // wave-uniform
    mfma_main_row(&sh.ray[lane][0], d, m, o, sc.sigma);
    {
        _Float16 s[16];
        mfma_y_chunk(s, d, o, bestK, sc.sigma, sc.Bmax);
        for (int j = 0; j < 16; j++) sh.ray[lane][32 + j] = s[j];
    }
    __syncthreads();
    for (int j = 0; j < 48; j++) frags[ray * 80 + j] = sh.ray[lane][j];
    const size_t ray0 = (size_t)blockIdx.x * 64;
    if constexpr (kPerm) {
        // the operand path of render_mfma_k5r / render_mfma_k5t: fragments
        // built in registers by frag_pair, not read from LDS rows.
        // frags[ray][48..63] receives the main fragment and [64..79] the Y
        // fragment as the MFMA A operand holds them (block R, lane l: ray 32R
        // + (l & 31), k-slots 8 (l >> 5) .. +7), so the host can check the
        // permutation against the rows above.
        const int r32 = lane & 31, hl = lane >> 5;
        h8 a0[2], y1[2];
        [[maybe_unused]] ThrBits tb = {};
        [[maybe_unused]] _Float16 tw16 = (_Float16)0.0f;
        if constexpr (kKthr) {
            kt_frags<LAYOUT >= 6>(d, m, sc, a0, tw16);
            kt_y(d, o, bestK, sc, tw16, y1);
        } else {
            _Float16 s[18];
            mfma_main_half_slots(s, d, m, sc.sigma);
            frag_pair(s, a0);
            _Float16 t[16];
            mfma_y_chunk(t, d, o, bestK, sc.sigma, sc.Bmax);
            frag_pair(t, y1);
            const float vz = m.z * sc.sigma;
            const _Float16 hz = (_Float16)vz;
            const _Float16 lz = (_Float16)(vz - (float)hz);
            tb = mfma_thr_bits(sc.Tw, wave_max(fabsf((float)lz)), wave_max(fabsf((float)hz)));
        }
        for (int R = 0; R < 2; R++)
            for (int j = 0; j < 8; j++) {
                frags[(ray0 + 32 * R + r32) * 80 + 48 + 8 * hl + j] = a0[R][j];
                frags[(ray0 + 32 * R + r32) * 80 + 64 + 8 * hl + j] = y1[R][j];
            }
        const h8* fg = reinterpret_cast<const h8*>(kKthr ? p.mfma_kt_frag : p.mfma_k16_frag) + lane;
        const int nops = kKthr ? kKtOps : kK16Ops;
        const f16v zero = {};
        if constexpr (LAYOUT == 7) {
            // MfmaSpec::cluster_rows16: U, -V, X of layout 6 by kt_group16's
            // products.  Each 16 rays of the wave in turn are the 16 rows:
            // alo = [rows | 0], ahi = [0 | rows]; the records through
            // kt16_record_lane.  T and Y stay 0 (the form has no Y).
            typedef uint32_t u4 __attribute__((ext_vector_type(4)));
            const h8* fg16 = reinterpret_cast<const h8*>(p.mfma_kt_frag) + kt16_record_lane(lane);
            const f4v zero4 = {};
            for (int R16 = 0; R16 < 4; R16++) {
                const u4 src = __builtin_bit_cast(u4, a0[R16 >> 1]);
                u4 lo, hi;
                for (int k = 0; k < 4; k++) {
                    const uint32_t v = (uint32_t)__shfl((int)src[k], 16 * (R16 & 1) + (lane & 15) + 32 * ((lane >> 4) & 1));
                    lo[k] = lane < 32 ? v : 0u;
                    hi[k] = lane < 32 ? 0u : v;
                }
                const h8 alo = __builtin_bit_cast(h8, lo), ahi = __builtin_bit_cast(h8, hi);
                for (int G = 0; G < n_pad / 32; G++) {
                    const h8* t = fg16 + (size_t)G * kKtOps * 64;
                    f4v q[2][3];
                    for (int op = 0; op < 3; op++) {
                        q[0][op] = __builtin_amdgcn_mfma_f32_16x16x32_f16(alo, t[64 * op], zero4, 0, 0, 0);
                        q[1][op] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ahi, t[64 * op], zero4, 0, 0, 0);
                    }
                    for (int h = 0; h < 2; h++)
                        for (int i = 0; i < 4; i++) {
                            const size_t rr = ray0 + 16 * R16 + 4 * (lane >> 4) + i;
                            float* tt = terms + (rr * n_pad + 32 * G + 16 * h + (lane & 15)) * 5;
                            tt[0] = q[h][0][i];
                            tt[1] = q[h][1][i];
                            tt[2] = q[h][2][i];
                        }
                }
            }
            return;
        }
        if constexpr (LAYOUT == 8) {
            // MfmaSpec::cluster_rows8: U, -V, X of layout 6 by kt_group8's
            // products.  Each 8 rays of the wave in turn are rows 0..7 as
            // [ray | 0] and rows 8..15 as [0 | the same ray], every other lane
            // of the fragment zero; the records through kt16_record_lane.
            typedef uint32_t u4 __attribute__((ext_vector_type(4)));
            const h8* fg16 = reinterpret_cast<const h8*>(p.mfma_kt_frag) + kt16_record_lane(lane);
            const f4v zero4 = {};
            const bool holds = lane < 32 ? (lane & 15) < 8 : (lane & 15) >= 8;
            for (int R8 = 0; R8 < 8; R8++) {
                const u4 src = __builtin_bit_cast(u4, a0[R8 >> 2]);
                u4 f;
                for (int k = 0; k < 4; k++) {
                    const uint32_t v = (uint32_t)__shfl((int)src[k], 8 * (R8 & 3) + (lane & 7) + 32 * ((lane >> 4) & 1));
                    f[k] = holds ? v : 0u;
                }
                const h8 a8 = __builtin_bit_cast(h8, f);
                for (int G = 0; G < n_pad / 32; G++) {
                    const h8* t = fg16 + (size_t)G * kKtOps * 64;
                    f4v q[3];
                    for (int op = 0; op < 3; op++)
                        q[op] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a8, t[64 * op], zero4, 0, 0, 0);
                    // D rows 4 (lane >> 4) + i: rows 0..7 are the rays against triangles 0..15, rows 8..15 the
                    // same rays against triangles 16..31
                    for (int i = 0; i < 4; i++) {
                        const int row = 4 * (lane >> 4) + i;
                        const size_t rr = ray0 + 8 * R8 + (row & 7);
                        float* tt = terms + (rr * n_pad + 32 * G + 16 * (row >> 3) + (lane & 15)) * 5;
                        tt[0] = q[0][i];
                        tt[1] = q[1][i];
                        tt[2] = q[2][i];
                    }
                }
            }
            return;
        }
        for (int G = 0; G < n_pad / 32; G++) {
            h8 b[kK16Ops];
            for (int op = 0; op < nops; op++) b[op] = fg[(size_t)G * nops * 64 + 64 * op];
            for (int R = 0; R < 2; R++) {
                K16Terms q;
                if constexpr (kKthr) {
                    q.U = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0[R], b[0], zero, 0, 0, 0);
                    q.V = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0[R], b[1], zero, 0, 0, 0);
                    q.X = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0[R], b[2], zero, 0, 0, 0);
                    q.T = zero;
                    q.Y = __builtin_amdgcn_mfma_f32_32x32x16_f16(y1[R], b[3], zero, 0, 0, 0);
                } else {
                    const f16v c = __builtin_amdgcn_mfma_f32_32x32x16_f16(mfma_thr_frag(tb), b[6], zero, 0, 0, 0);
                    q.U = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0[R], b[0], c, 0, 0, 0);
                    q.V = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0[R], b[2], c, 0, 0, 0);
                    q.X = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0[R], b[4], c, 0, 0, 0);
                    q.T = c;
                    q.Y = __builtin_amdgcn_mfma_f32_32x32x16_f16(y1[R], b[6], c, 0, 0, 0);
                }
                for (int i = 0; i < 16; i++) {
                    const size_t rr = ray0 + 32 * R + 8 * (i >> 2) + 4 * hl + (i & 3);
                    float* tt = terms + (rr * n_pad + 32 * G + r32) * 5;
                    tt[0] = q.U[i];
                    tt[1] = q.V[i];
                    tt[2] = q.X[i];
                    tt[3] = q.T[i];
                    tt[4] = q.Y[i];
                }
            }
        }
    } else if constexpr (kK16) {
        const int r32 = lane & 31, hl = lane >> 5;
        // layout 3: the threshold factors (the wave's m.z halves)
        [[maybe_unused]] ThrBits tb = {};
        if constexpr (kCthr) {
            const float vz = m.z * sc.sigma;
            const _Float16 hz = (_Float16)vz;
            const _Float16 lz = (_Float16)(vz - (float)hz);
            tb = mfma_thr_bits(sc.Tw, wave_max(fabsf((float)lz)), wave_max(fabsf((float)hz)));
        }
        const h8* fg = reinterpret_cast<const h8*>(p.mfma_k16_frag) + lane;
        for (int G = 0; G < n_pad / 32; G++) {
            h8 b[kK16Ops];
            for (int op = 0; op < kK16Ops; op++) b[op] = fg[(size_t)G * kK16Ops * 64 + 64 * op];
            for (int R = 0; R < 2; R++) {
                const h8 a0 = *reinterpret_cast<const h8*>(&sh.ray[32 * R + r32][8 * hl]);
                const h8 a1 = *reinterpret_cast<const h8*>(&sh.ray[32 * R + r32][16 + 8 * hl]);
                const h8 y1 = *reinterpret_cast<const h8*>(&sh.ray[32 * R + r32][32 + 8 * hl]);
                K16Terms q = k16_terms(a0, a1, y1, b);
                if constexpr (kK5) {
                    // the 5-product form: U, -V, X from the first K-half only;
                    // layout 3: all four with the threshold product TT as the
                    // accumulator, TT itself in the -tn slot
                    const f16v zero = {};
                    f16v c = zero;
                    if constexpr (kCthr) c = __builtin_amdgcn_mfma_f32_32x32x16_f16(mfma_thr_frag(tb), b[6], zero, 0, 0, 0);
                    q.U = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b[0], c, 0, 0, 0);
                    q.V = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b[2], c, 0, 0, 0);
                    q.X = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b[4], c, 0, 0, 0);
                    if constexpr (kCthr) {
                        q.T = c;
                        q.Y = __builtin_amdgcn_mfma_f32_32x32x16_f16(y1, b[6], c, 0, 0, 0);
                    }
                }
                for (int i = 0; i < 16; i++) {
                    const size_t rr = ray0 + 32 * R + 8 * (i >> 2) + 4 * hl + (i & 3);
                    float* tt = terms + (rr * n_pad + 32 * G + r32) * 5;
                    tt[0] = q.U[i];
                    tt[1] = q.V[i];
                    tt[2] = q.X[i];
                    tt[3] = q.T[i];
                    tt[4] = q.Y[i];
                }
            }
        }
    } else {
        // the 16x16x32 form: A rows in the main/Y LDS rows, the Y fragment
        // with slots 0..15 zero
        const h8* fg = reinterpret_cast<const h8*>(p.mfma_frag) + lane;
        const f4v zero = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int G = 0; G < n_pad / 16; G++) {
            const h8 c0 = fg[(size_t)G * kMfmaQ * 64], c1 = fg[(size_t)G * kMfmaQ * 64 + 64],
                     c2 = fg[(size_t)G * kMfmaQ * 64 + 128], c3 = fg[(size_t)G * kMfmaQ * 64 + 192];
            for (int R = 0; R < 4; R++) {
                const int row = 16 * R + (lane & 15), k0 = 8 * (lane >> 4);
                const h8 ra = *reinterpret_cast<const h8*>(&sh.ray[row][k0]);
                h8 ya = h8{};
                if (k0 >= 16) ya = *reinterpret_cast<const h8*>(&sh.ray[row][32 + k0 - 16]);
                const f4v qU = __builtin_amdgcn_mfma_f32_16x16x32_f16(ra, c0, zero, 0, 0, 0);
                const f4v qV = __builtin_amdgcn_mfma_f32_16x16x32_f16(ra, c1, zero, 0, 0, 0);
                const f4v qX = __builtin_amdgcn_mfma_f32_16x16x32_f16(ra, c2, zero, 0, 0, 0);
                const f4v qT = __builtin_amdgcn_mfma_f32_16x16x32_f16(ra, c3, zero, 0, 0, 0);
                const f4v qY = __builtin_amdgcn_mfma_f32_16x16x32_f16(ya, c3, zero, 0, 0, 0);
                for (int i = 0; i < 4; i++) {
                    const size_t rr = ray0 + 16 * R + 4 * (lane >> 4) + i;
                    float* tt = terms + (rr * n_pad + 16 * G + (lane & 15)) * 5;
                    tt[0] = qU[i];
                    tt[1] = qV[i];
                    tt[2] = qX[i];
                    tt[3] = qT[i];
                    tt[4] = qY[i];
                }
            }
        }
    }
}

}  // namespace
