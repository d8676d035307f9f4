// Preview shading queries (rt2_shade_rays): the reference's traceBasic
// (compute.glsl:565-645) for a caller's rays.  Record i holds what trace_basic
// (rt2_misc_kernels.h) returns for Ray(o_i, d_i) with insideGlass = false, bit
// for bit, and the closest-hit searches the ray cost (bounces plus the shadow
// ray).  rt2_ray.tmax is not used: every segment of traceBasic is unbounded.
// Included by rt2_render.hip only (one translation unit; internal linkage).
//
//   shade_rays_k5r<O>        brute force on the matrix filter: trace_rays_k5r's
//                            frame (rt2_query.h) with a bounce loop per 64-ray
//                            chunk around sweep_kt_res, one step of traceBasic
//                            per live lane after each search (shade_step), and
//                            one sweep_kt_occ at the end for the lanes whose
//                            path ended on a surface that casts a shadow ray
//   shade_rays_scalar<B,BVH> one thread per ray: trace_basic itself, then one
//                            16-byte store; BVH traversal, RT2_TRACE_SCALAR,
//                            scenes outside the filter's range
//
// The chunk's bounce loop.  A lane is tracing, done, or waiting for its shadow
// ray.  Lanes that do not trace carry the first tracing lane's ray through the
// sweep, as render_mfma_k5r's do; what they hold (a finished colour, or a
// shadow ray with its colour and bounce count) is not touched.  When at most 32
// lanes trace they are moved to lanes 0..31 and only the first 32-ray block is
// swept; the whole lane state moves, the ray's slot in the chunk included, so
// every record is stored at its own index.  The shadow ray is deferred: a lane
// that ends on a diffuse, checker or texture hit keeps (o, toLight) and leaves
// the loop, and one any-hit sweep at bound 1e38f serves all of the chunk's
// waiting lanes.  rt2_occluded's contract makes its answer closest_any's
// bi >= 0, which is what trace_basic tests.
#pragma once

namespace {

struct ShadeParams {
    const rt2_ray* rays;
    rt2_shaded* out;
    long long n;
};

enum : int { SH_TRACE = 0, SH_DONE = 1, SH_SHADOW = 2 };

// One ray's state between the segments of traceBasic.  SH_DONE: cum is the
// returned colour.  SH_SHADOW: (o, d) is the shadow ray, cum the sum before
// the two divisions.  bc counts the bounces; slot is the ray's place in its
// chunk (-1: the padding of a ragged chunk, nothing is stored).
struct ShadeLane {
    f3 o, d, cum;
    int bc, st, slot;
    bool inside;
};

// One step of traceBasic's loop after the search of segment (L.o, L.d) ended
// at (best, bi): trace_basic's body (rt2_misc_kernels.h), the same operations
// in the same order, with its returns turned into states.
__device__ __forceinline__ void shade_step(const RenderParams& p, ShadeLane& L, float best, int bi) {
    L.bc++;
    if (bi < 0) {
        L.cum = divs(add(L.cum, sky(L.d)), (float)L.bc);
        L.st = SH_DONE;
        return;
    }
    const float4 t2 = p.tri[3 * bi + 2];
    const f3 normal = normalize(mk(t2.y, t2.z, t2.w));
    const f3 hitPoint = add(L.o, muls(L.d, best));
    const rt2_material m = p.mats[p.tri_mtl[bi]];
    const f3 tex = m.materialType == RT2_TEXTURE ? texture_color(p, m.textureIndex, bi, L.o, L.d)
                                                  : mk(0.0f, 0.0f, 0.0f);
    L.o = sub(hitPoint, muls(normal, 1e-4f));  // :579
    switch (m.materialType) {
    case RT2_SPECULAR:
        L.cum = add(L.cum, xyz4(m.color));
        L.d = reflect(L.d, normal);
        break;
    case RT2_DIFFUSE:
    case RT2_TEXTURE:
    case RT2_CHECKER: {
        f3 color;
        if (m.materialType == RT2_TEXTURE) {
            color = tex;
        } else if (m.materialType == RT2_DIFFUSE) {
            color = xyz4(m.color);
        } else {
            const float s = m.checkerScale;
            bool black = false;
            if (s > 0.0f) {
                const float sum = floorf(L.o.x * s) + floorf(L.o.y * s) + floorf(L.o.z * s);
                black = sum - 2.0f * floorf(sum / 2.0f) == 0.0f;
            }
            color = black ? mk(0.0f, 0.0f, 0.0f) : mk(1.0f, 1.0f, 1.0f);
        }
        L.cum = add(L.cum, color);
        if (p.basicShadow) {  // :614-621: the shadow ray waits for the chunk's any-hit sweep
            L.d = normalize(sub(ld3(p.light), hitPoint));
            L.st = SH_SHADOW;
        } else {
            L.cum = divs(L.cum, (float)L.bc);
            L.st = SH_DONE;
        }
        return;
    }
    case RT2_LIGHT: {  // normalizeColor, :462-470
        const f3 e = xyz4(m.emissionColor);
        const float mx = rt2pm_fmaxf(rt2pm_fmaxf(e.x, e.y), e.z);
        L.cum = mx > 1.0f ? divs(e, mx) : e;
        L.st = SH_DONE;
        return;
    }
    case RT2_GLASS: {
        const float eta = L.inside ? m.refractiveIndex : 1.0f / m.refractiveIndex;
        bool refr;
        L.d = refract_(L.d, normal, eta, refr);
        L.inside = refr != L.inside;
        L.cum = xyz4(m.color);
        break;
    }
    case RT2_GLASS_HIGHLIGHT:  // `if (bounceCount == 0)` never holds after bounceCount++
        break;
    default:
        L.cum = mk(1.0f, 0.0f, 1.0f);
        L.st = SH_DONE;
        return;
    }
    if (L.bc >= p.maxBounce) {  // the loop's own end
        L.cum = divs(L.cum, (float)L.bc);
        L.st = SH_DONE;
    }
}

// Moves every lane's state to lane `to / 4` (ds_permute's byte address).
__device__ __forceinline__ void shade_permute(ShadeLane& L, int to) {
    L.o = perm_f3(to, L.o);
    L.d = perm_f3(to, L.d);
    L.cum = perm_f3(to, L.cum);
    L.bc = perm_i(to, L.bc);
    L.st = perm_i(to, L.st);
    L.slot = perm_i(to, L.slot);
    L.inside = perm_i(to, (int)L.inside) != 0;
}

template <OccSpec O>
__global__ __launch_bounds__(O.m.block) __attribute__((amdgpu_waves_per_eu(O.m.waves))) void shade_rays_k5r(RenderParams p_arg,
                                                                                                           ShadeParams q) {
    constexpr MfmaSpec S = O.m;  // the closest-hit sweeps and the any-hit sweep share the frame and its records
    query_chunks<S>(q.n, [&](const RenderParams& p, const h8* rec, long long base, int live, MfmaDiag& dg,
                             unsigned long long& segs_w) {
        const int lane = (int)lane_id();
        ShadeLane L;
        {
            // lanes of a ragged last chunk hold the chunk's first ray and never trace it; tmax is not used
            float unused;
            query_load(q.rays, base + (lane < live ? lane : 0), L.o, L.d, unused);
        }
        L.cum = mk(0.0f, 0.0f, 0.0f);
        L.bc = 0;
        L.inside = false;  // `Ray ray;` leaves insideGlass undefined (:674); false as in trace_basic
        L.st = lane < live ? SH_TRACE : SH_DONE;
        L.slot = lane < live ? lane : -1;
        for (;;) {
            unsigned long long act = __ballot(L.st == SH_TRACE);
            if (!act) break;
            segs_w += (unsigned long long)__popcll(act);
            // at most 32 tracing lanes: move them to lanes 0..31 and sweep the first 32-ray block only
            bool upper = true;
            if (__popcll(act) <= 32) {
                if (act >> 32) {
                    const uint32_t nl = (uint32_t)__popcll(act);
                    const bool tr = (act >> lane) & 1ull;
                    shade_permute(L, 4 * (int)(tr ? lanes_below(act) : nl + lanes_below(~act)));
                    act = __ballot(L.st == SH_TRACE);
                }
                upper = false;
            }
            // lanes that do not trace carry the first tracing lane's ray through the sweep
            const int j0 = __builtin_ctzll(act);
            const bool mine = L.st == SH_TRACE;
            f3 ro = mk(__shfl(L.o.x, j0), __shfl(L.o.y, j0), __shfl(L.o.z, j0));
            f3 rd = mk(__shfl(L.d.x, j0), __shfl(L.d.y, j0), __shfl(L.d.z, j0));
            if (mine) {
                ro = L.o;
                rd = L.d;
            }
            float best = 1e38f, bestK = 1e38f * 1.0009765625f;
            int bi = -1;
            bool swept = false;
            if (!__ballot(!query_finite(ro, rd))) swept = sweep_kt_res<S>(p, rec, ro, rd, best, bi, bestK, dg, upper);
            // a ray outside the filter's range or not finite (wave-uniform): the drain's exact code
            if (!swept) coop_each(act, ro, rd, p, best, bi);
            if (mine) shade_step(p, L, best, bi);
        }
        // the deferred shadow rays: one any-hit sweep for all of the chunk's waiting lanes
        const unsigned long long pend = __ballot(L.st == SH_SHADOW);
        if (pend) {
            segs_w += (unsigned long long)__popcll(pend);
            const int j0 = __builtin_ctzll(pend);
            const bool mine = L.st == SH_SHADOW;
            f3 so = mk(__shfl(L.o.x, j0), __shfl(L.o.y, j0), __shfl(L.o.z, j0));
            f3 sd = mk(__shfl(L.d.x, j0), __shfl(L.d.y, j0), __shfl(L.d.z, j0));
            if (mine) {
                so = L.o;
                sd = L.d;
            }
            bool occ = false, swept = false;
            if (!__ballot(!query_finite(so, sd)))
                swept = sweep_kt_occ<O>(p, rec, so, sd, 1e38f, 1e38f * 1.0009765625f, (pend >> 32) != 0, mine, occ);
            if (!swept) {
                float best = 1e38f;
                int bi = -1;
                coop_each(pend, so, sd, p, best, bi);
                occ = bi >= 0;
            }
            if (mine) {
                L.cum = divs(occ ? divs(L.cum, 5.0f) : L.cum, (float)L.bc);
                L.bc += 1;  // the shadow ray's search
            }
        }
        if (L.slot >= 0)  // one 16-byte store per ray, at the ray's own index
            *reinterpret_cast<float4*>(q.out + base + L.slot) =
                make_float4(L.cum.x, L.cum.y, L.cum.z, __int_as_float(L.bc));
    });
}

// One thread per ray: trace_basic as render_basic calls it, then the record.
// BVH: dynamic LDS = stack_slots * BLOCK ints (closest_bvh's stack).
template <int BLOCK, bool BVH>
__global__ __launch_bounds__(BLOCK) void shade_rays_scalar(RenderParams p, ShadeParams q) {
    extern __shared__ int shade_stack[];
    const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    uint32_t segs = 0, tests = 0, visits = 0;
    if (i < q.n) {
        f3 o, d;
        float unused;  // tmax
        query_load(q.rays, i, o, d, unused);
        const f3 c = trace_basic<BLOCK, BVH>(p, o, d, shade_stack, segs, tests, &visits);
        *reinterpret_cast<float4*>(q.out + i) = make_float4(c.x, c.y, c.z, __int_as_float((int)segs));
    }
    unsigned long long s = segs, t = tests, v = visits;
    for (int off = 32; off > 0; off >>= 1) {
        s += __shfl_xor(s, off);
        t += __shfl_xor(t, off);
        v += __shfl_xor(v, off);
    }
    if (lane_id() == 0) {
        atomicAdd(p.seg_counter, s);
        if (BVH) {
            atomicAdd(p.seg_counter + 1, t);  // leaf triangle tests
            atomicAdd(p.seg_counter + 2, v);  // interior node visits
        }
    }
}

}  // namespace
