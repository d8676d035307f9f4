// Surface queries (rt2_surface_rays): what is at the closest hit of a caller's
// rays.  Record i holds rt2_trace_rays' (dst, tri) for ray i, bit for bit, and
// the reference's HitInfo (compute.glsl:97-106) plus the surface's base colour:
// material index and type, the unit normal, rayTriangleIntersect's
// barycentrics and what traceBasic (compute.glsl:565-645) returns for the ray
// with maxBounceCount = 1 and basicShadingShadow = 0.
// Included by rt2_render.hip only (one translation unit; internal linkage).
//
//   surface_k5r<S>         brute force on the matrix filter: trace_rays_k5r's
//                          frame (rt2_query.h) with surface_record and three
//                          16-byte stores per lane where query_store was; a
//                          64-ray chunk writes 3 KiB contiguous
//   surface_scalar<B,BVH>  one thread per ray, trace_rays_scalar's search and
//                          the same epilogue: BVH traversal, RT2_TRACE_SCALAR,
//                          scenes outside the filter's range
//   camera_rays_kernel     the deterministic primary ray of every pixel of a
//                          shard's slab (main's basicShading branch,
//                          compute.glsl:665-676, as render_basic evaluates it)
//
// The epilogue runs once per ray after the search, on the ray's own o and d:
// nothing of it is live during the sweep.
#pragma once

namespace {

struct SurfaceParams {
    const rt2_ray* rays;
    rt2_surface* out;
    long long n;
};

struct SurfaceRec {
    float4 a, b, c;  // {dst, tri, mtl, mtl_type} {normal, u} {albedo, v}
};

// The record of ray (o, d) whose search ended at (best, bi).  The arithmetic is
// trace_basic's first bounce (rt2_misc_kernels.h) and texture_color's
// barycentrics (rt2_path.h), the same operations in the same order.
__device__ __forceinline__ SurfaceRec surface_record(const RenderParams& p, const f3& o, const f3& d, float best,
                                                     int bi) {
    SurfaceRec r;
    if (bi < 0) {  // a miss: dst = bound_i, three indices of -1, eight floats of +0.0
        r.a = make_float4(best, __int_as_float(-1), __int_as_float(-1), __int_as_float(-1));
        r.b = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        r.c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return r;
    }
    const int mi = p.tri_mtl[bi];
    const rt2_material m = p.mats[mi];
    const float4 un = p.unit_n[bi];
    const f3 normal = mk(un.x, un.y, un.z);  // normalize(cross01), compute.glsl:331 (prep_unit_normals)
    // rayTriangleIntersect's u, v (compute.glsl:322-337) as texture_color recomputes them
    const MtQ q = mt_quantities(o, d, p.tri[3 * bi], p.tri[3 * bi + 1], p.tri[3 * bi + 2]);
    const float inv = 1.0f / q.det;
    const float u = -q.U * inv;
    const float v = q.V * inv;
    f3 cum = mk(0.0f, 0.0f, 0.0f);
    switch (m.materialType) {
    case RT2_SPECULAR:
    case RT2_DIFFUSE:
        cum = add(cum, xyz4(m.color));
        break;
    case RT2_TEXTURE:
        cum = add(cum, texture_color(p, m.textureIndex, bi, o, d));
        break;
    case RT2_CHECKER: {
        const f3 hitPoint = add(o, muls(d, best));
        const f3 c = sub(hitPoint, muls(normal, 1e-4f));  // :579
        const float s = m.checkerScale;
        bool black = false;
        if (s > 0.0f) {
            const float sum = floorf(c.x * s) + floorf(c.y * s) + floorf(c.z * s);
            black = sum - 2.0f * floorf(sum / 2.0f) == 0.0f;
        }
        cum = add(cum, black ? mk(0.0f, 0.0f, 0.0f) : mk(1.0f, 1.0f, 1.0f));
        break;
    }
    case RT2_LIGHT: {  // normalizeColor, :462-470; returned as it is
        const f3 e = xyz4(m.emissionColor);
        const float mx = rt2pm_fmaxf(rt2pm_fmaxf(e.x, e.y), e.z);
        cum = mx > 1.0f ? divs(e, mx) : e;
        break;
    }
    case RT2_GLASS:
        cum = xyz4(m.color);
        break;
    case RT2_GLASS_HIGHLIGHT:  // `if (bounceCount == 0)` never holds after bounceCount++
        break;
    default:
        cum = mk(1.0f, 0.0f, 1.0f);
    }
    r.a = make_float4(best, __int_as_float(bi), __int_as_float(mi), __int_as_float(m.materialType));
    r.b = make_float4(normal.x, normal.y, normal.z, u);
    r.c = make_float4(cum.x, cum.y, cum.z, v);
    return r;
}

__device__ __forceinline__ void surface_store(rt2_surface* out, long long i, const SurfaceRec& r) {
    float4* w = reinterpret_cast<float4*>(out + i);  // three 16-B stores
    w[0] = r.a;
    w[1] = r.b;
    w[2] = r.c;
}

template <MfmaSpec S>
__global__ __launch_bounds__(S.block) __attribute__((amdgpu_waves_per_eu(S.waves))) void surface_k5r(RenderParams p_arg,
                                                                                                      SurfaceParams q) {
    query_chunks<S>(q.n, [&](const RenderParams& p, const h8* rec, long long base, int live, MfmaDiag& dg,
                             unsigned long long& segs_w) {
        const int lane = (int)lane_id();
        const bool mine = lane < live;
        const unsigned long long act = live == 64 ? ~0ull : (1ull << live) - 1ull;
        // lanes of a ragged last chunk carry the chunk's first ray (and its bound) and store nothing
        f3 o, d;
        float bound;
        query_load(q.rays, base + (mine ? lane : 0), o, d, bound);
        float best = bound, bestK = bound * 1.0009765625f;
        int bi = -1;
        bool swept = false;
        if (!__ballot(!query_finite(o, d))) swept = sweep_kt_res<S>(p, rec, o, d, best, bi, bestK, dg, live > 32);
        // a ray outside the filter's range or not finite (wave-uniform): the drain's exact code
        if (!swept) coop_each(act, o, d, p, best, bi, &bound);
        if (mine) surface_store(q.out, base + lane, surface_record(p, o, d, best, bi));
        segs_w += (unsigned long long)live;
    });
}

// One thread per ray: trace_rays_scalar's search, then the record.
// BVH: dynamic LDS = stack_slots * BLOCK ints (closest_bvh's stack).
template <int BLOCK, bool BVH>
__global__ __launch_bounds__(BLOCK) void surface_scalar(RenderParams p, SurfaceParams q) {
    extern __shared__ int surface_stack[];
    const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    uint32_t tests = 0, visits = 0;
    if (i < q.n) {
        f3 o, d;
        float best;
        query_load(q.rays, i, o, d, best);
        int bi = -1;
        if constexpr (BVH) {
            closest_bvh<BLOCK>(o, d, p.nodes, p.tri, surface_stack, p.stack_slots, best, bi, tests, visits);
        } else {
            float bestK = best * 1.0009765625f;
            sweep_masked<8, true>(o, d, nullptr, (const float*)p.tri, p.n_tris, 0, best, bi, bestK);
        }
        surface_store(q.out, i, surface_record(p, o, d, best, bi));
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

struct CameraParams {
    float cam[3], vpRight[3], vpUp[3], vpFront[3];
    int W, H;
    int tile_rows, rank, nranks;
    long long n;  // slab pixels
    rt2_ray* out;
};

// One thread per slab pixel: render_basic's ray, two 16-B stores.
__global__ __launch_bounds__(256) void camera_rays_kernel(CameraParams p) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= p.n) return;
    const int lr = (int)(i / p.W);
    const int x = (int)(i - (long long)lr * p.W);
    const int y = shard_row(lr, p.tile_rows, p.rank, p.nranks);
    const float px = (float)(x * 2 - p.W) / (float)p.W;
    const float py = (float)(y * 2 - p.H) / (float)p.H;
    const f3 dir = normalize(add(add(ld3(p.vpFront), muls(ld3(p.vpRight), px)), muls(ld3(p.vpUp), py)));
    float4* w = reinterpret_cast<float4*>(p.out + i);
    w[0] = make_float4(p.cam[0], p.cam[1], p.cam[2], 0.0f);  // tmax = 0: unbounded
    w[1] = make_float4(dir.x, dir.y, dir.z, 0.0f);
}

}  // namespace
