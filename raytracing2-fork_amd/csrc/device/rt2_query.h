// Ray queries (rt2_trace_rays): the closest hit of a caller's rays, read from
// memory instead of being made by the path tracer.  hits[i] is the sequential
// strict `dst < best` scan of calculateRayCollision (compute.glsl:429-434, or
// the BVH walk :410-460) over the triangles as uploaded, started at best =
// bound_i, bit for bit.
// Included by rt2_render.hip only (one translation unit; internal linkage).
//
//   trace_rays_k5r<S>     brute force on the matrix filter: the resident
//                         kernel's frame (rt2_k5_resident.h: 1,024 threads,
//                         the records in LDS once per launch, one barrier)
//                         around sweep_kt_res; each wave takes chunks of 64
//                         consecutive rays, a grid stride apart
//   trace_rays_scalar<B>  one thread per ray: sweep_masked (triangles through
//                         the scalar cache) or closest_bvh; scenes outside
//                         the filter's range, BVH traversal, RT2_TRACE_SCALAR
//
// Rays outside the filter's range.  sweep_kt_res returns false, wave-uniform
// and with nothing computed, when some lane has |o|inf > 2^20 or |d|inf >
// 1.0001 (mfma_scale); the chunk then takes the cooperative drain's exact code
// (coop_each, started at each ray's bound).  mfma_scale's test sends infinite
// components there but not every NaN: its maxima are v_max_f32, which returns
// the other operand of a NaN, so (NaN, 1, 1) passes as 1.  An explicit lane
// test (query_finite) therefore routes a chunk with any non-finite component
// to the exact code before sweep_kt_res is called: no NaN reaches the wave
// maxima or the fragments that other lanes' rays share.  The exact code is the
// reference arithmetic, in which a non-finite component ends as a NaN or
// infinite dst that fails `dst < best`: a miss.
#pragma once

namespace {

// The query's own kernel arguments (RenderParams stays the first argument:
// kargs<RenderParams>() reads it from the start of the kernarg segment).
struct QueryParams {
    const rt2_ray* rays;
    rt2_hit* hits;
    long long n;
};

// bound_i of rt2.h: tmax when 0 < tmax < 1e38f, else 1e38f (zero, negative, NaN, infinite: unbounded)
__device__ __forceinline__ float query_bound(float tmax) { return (tmax > 0.0f && tmax < 1e38f) ? tmax : 1e38f; }

__device__ __forceinline__ bool query_finite(const f3& o, const f3& d) {
    const float big = 3.4028234664e38f;  // FLT_MAX; false for NaN
    return fabsf(o.x) <= big && fabsf(o.y) <= big && fabsf(o.z) <= big && fabsf(d.x) <= big && fabsf(d.y) <= big &&
           fabsf(d.z) <= big;
}

__device__ __forceinline__ void query_load(const rt2_ray* rays, long long i, f3& o, f3& d, float& bound) {
    const float4* r = reinterpret_cast<const float4*>(rays + i);  // two 16-B loads
    const float4 a = r[0], b = r[1];
    o = mk(a.x, a.y, a.z);
    d = mk(b.x, b.y, b.z);
    bound = query_bound(a.w);
}

__device__ __forceinline__ void query_store(rt2_hit* hits, long long i, float best, int bi) {
    *reinterpret_cast<float2*>(hits + i) = make_float2(best, __int_as_float(bi));  // one 8-B store
}

// The resident chunk frame of the five *_k5r kernels: the resident records into LDS (one barrier), then each wave
// takes chunks of 64 consecutive rays, a grid stride of waves apart, and lane 0 adds the wave's segments to the
// launch's counter at the end.  body(p, rec, base, live, dg, segs_w) handles the chunk of `live` rays from ray `base`
// on and adds its segments to segs_w (the wave's count, by reference and not returned: a returned count is summed
// in another order, and shade_rays_k5r and radiance_rays_k5r then compile to other code than before the frame was
// shared).  Returns the sweeps' diagnostic counters (S.diag).
// (A device-wide chunk counter, one atomic per chunk, held the whole launch to 14 ns per chunk: 2^22 rays took
// 0.91 ms whatever their sweeps cost.)
template <MfmaSpec S, class Body>
__device__ __forceinline__ MfmaDiag query_chunks(long long n, Body body) {
    __shared__ K5Resident rs;
    res_load_records<S>(rs);
    MfmaDiag dg;
    const int lane = (int)lane_id();
    const unsigned long long n_chunks = ((unsigned long long)n + 63) >> 6;
    unsigned long long segs_w = 0;
    const unsigned long long n_waves = (unsigned long long)gridDim.x * (S.block / 64);
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // wave-uniform to the compiler
    for (unsigned long long c = (unsigned long long)blockIdx.x * (S.block / 64) + wave; c < n_chunks; c += n_waves) {
        const RenderParams& p = kargs<RenderParams>();
        const long long base = (long long)(c << 6);
        const int live = (int)min(64ll, n - base);
        body(p, rs.rec, base, live, dg, segs_w);
    }
    const RenderParams& p = kargs<RenderParams>();
    if (lane == 0) atomicAdd(p.seg_counter, segs_w);
    return dg;
}

template <MfmaSpec S>
__global__ __launch_bounds__(S.block) __attribute__((amdgpu_waves_per_eu(S.waves))) void trace_rays_k5r(RenderParams p_arg,
                                                                                                         QueryParams q) {
    const MfmaDiag sum = query_chunks<S>(q.n, [&](const RenderParams& p, const h8* rec, long long base, int live,
                                                  MfmaDiag& dg, unsigned long long& segs_w) {
        const int lane = (int)lane_id();
        const bool mine = lane < live;
        const unsigned long long act = live == 64 ? ~0ull : (1ull << live) - 1ull;
        // lanes of a ragged last chunk carry the chunk's first ray (and its bound)
        f3 o, d;
        float bound;
        query_load(q.rays, base + (mine ? lane : 0), o, d, bound);
        float best = bound, bestK = bound * 1.0009765625f;
        int bi = -1;
        bool swept = false;
        if (!__ballot(!query_finite(o, d))) swept = sweep_kt_res<S>(p, rec, o, d, best, bi, bestK, dg, live > 32);
        // a ray outside the filter's range or not finite (wave-uniform): the drain's exact code
        if (!swept) coop_each(act, o, d, p, best, bi, &bound);
        if (mine) query_store(q.hits, base + lane, best, bi);
        segs_w += (unsigned long long)live;
    });
    if constexpr (S.diag) {  // render_mfma_k5r's counter slots (rt2_scene_diag_ex)
        const RenderParams& p = kargs<RenderParams>();
        if (lane_id() == 0) {
            atomicAdd(p.seg_counter + 1, sum.groups);    // (wave, triangle group) sweeps
            atomicAdd(p.seg_counter + 2, sum.hot);       // ... with a passing pair
            atomicAdd(p.seg_counter + 3, sum.exact);     // (wave, triangle) exact tests
            atomicAdd(p.seg_counter + 12, sum.t_wait);   // shader clocks: the sweep's ray setup
            atomicAdd(p.seg_counter + 13, sum.t_filt);   // ... products + record reads
            atomicAdd(p.seg_counter + 14, sum.t_exact);  // ... exact phase
            atomicAdd(p.seg_counter + 15, sum.t_swp);    // ... whole sweeps
        }
    }
}

// One thread per ray: closest_any's two arms started at the ray's bound.
// BVH: dynamic LDS = stack_slots * BLOCK ints (closest_bvh's stack).
template <int BLOCK, bool BVH>
__global__ __launch_bounds__(BLOCK) void trace_rays_scalar(RenderParams p, QueryParams q) {
    extern __shared__ int query_stack[];
    const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    uint32_t tests = 0, visits = 0;
    if (i < q.n) {
        f3 o, d;
        float best;
        query_load(q.rays, i, o, d, best);
        int bi = -1;
        if constexpr (BVH) {
            closest_bvh<BLOCK>(o, d, p.nodes, p.tri, query_stack, p.stack_slots, best, bi, tests, visits);
        } else {
            float bestK = best * 1.0009765625f;
            sweep_masked<8, true>(o, d, nullptr, (const float*)p.tri, p.n_tris, 0, best, bi, bestK);
        }
        query_store(q.hits, i, best, bi);
    }
    unsigned long long s = i < q.n, t = tests, v = visits;
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
