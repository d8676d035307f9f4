// Radiance queries (rt2_radiance_rays, rt2_path_rays): the reference's
// Monte-Carlo path tracer trace() (compute.glsl:472-563) for a caller's rays
// and random streams.  Record i holds what trace returns for Ray(o_i, d_i,
// insideGlass = false) with rngState = rng[i]: the value end_path (rt2_path.h)
// adds to colorCumulative, bit for bit, and the closest-hit searches the path
// cost; rng[i] is left at the state after the path's last draw.  rt2_ray.tmax
// is not used: every segment of trace is unbounded.
// Included by rt2_render.hip only (one translation unit; internal linkage).
//
//   radiance_rays_k5r<O>        brute force on the matrix filter: shade_rays_k5r's
//                               frame (rt2_shade.h) with one step of trace's loop
//                               per live lane after each search (radiance_step)
//                               and a random stream per lane; no deferred sweep,
//                               trace has no shadow ray
//   radiance_rays_scalar<B,BVH> one thread per ray around closest_any with the
//                               same step; BVH traversal, RT2_TRACE_SCALAR, scenes
//                               outside the filter's range
//   path_rays_kernel            the path tracer's camera: advance's ST_NEW_RAY
//                               block (rt2_path.h) for every pixel of a slab
//
// The chunk's bounce loop is shade_rays_k5r's: a lane is tracing or done, lanes
// that do not trace carry the first tracing lane's ray through the sweep, and
// when at most 32 lanes trace they are moved to lanes 0..31 with their whole
// state, the random stream and the ray's slot in the chunk included, so every
// record and every stream state is stored at its own index.  The small fields
// (bounce count, insideGlass, done, slot) share one register.
#pragma once

namespace {

struct RadianceParams {
    const rt2_ray* rays;
    uint32_t* rng;
    rt2_radiance* out;
    long long n;
};

// RadLane::pk: bits 0..8 the bounces traced (0 .. 256), bit 9 insideGlass, bit
// 10 the path has ended, bits 11..17 the ray's place in its chunk plus one (0:
// the padding of a ragged chunk, nothing is stored).
enum : uint32_t { RD_BOUNCE = 0x1ffu, RD_INSIDE = 1u << 9, RD_DONE = 1u << 10, RD_SLOT_SHIFT = 11u };

// One ray's state between the segments of trace.  When the path has ended,
// incoming is the returned colour and seed the stream's state after its last draw.
struct RadLane {
    f3 o, d, rayColor, incoming;
    uint32_t seed, pk;
};

// One step of trace's loop after the search of segment (L.o, L.d) ended at
// (best, bi): shade's body (rt2_path.h), the same operations in the same
// order, with every end_path turned into RD_DONE.
__device__ __forceinline__ void radiance_step(const RenderParams& p, RadLane& L, float best, int bi) {
    L.pk += 1u;  // bounceCount++
    const int bounce = (int)(L.pk & RD_BOUNCE);
    if (bi >= 0) {
        const int mi = p.tri_mtl[bi];
        f3 tex = mk(0.0f, 0.0f, 0.0f);
        if (p.mats[mi].materialType == RT2_TEXTURE) tex = texture_color(p, p.mats[mi].textureIndex, bi, L.o, L.d);
        const float4 un = p.unit_n[bi];
        const f3 normal = mk(un.x, un.y, un.z);
        const f3 hitPoint = add(L.o, muls(L.d, best));
        const rt2_material m = p.mats[mi];
        if (m.materialType != RT2_GLASS)
            L.o = sub(hitPoint, muls(muls(L.d, best), -1e-3f));
        else
            L.o = add(hitPoint, muls(muls(L.d, best), -1e-3f));
        f3 atten = mk(0.0f, 0.0f, 0.0f);
        const f3 prevDir = L.d;
        switch (m.materialType) {
        case RT2_DIFFUSE:
        case RT2_TEXTURE:
            L.d = normalize(add(normal, rnd_dir(L.seed)));
            atten = m.materialType == RT2_DIFFUSE ? xyz4(m.color) : tex;
            break;
        case RT2_SPECULAR: {
            f3 diffuseDir = normalize(add(normal, rnd_dir(L.seed)));
            f3 specDir = reflect(L.d, normal);
            bool isSpec = m.specularProbability > rnd(L.seed);
            L.d = mixs(diffuseDir, specDir, isSpec ? m.smoothness : 0.0f);
            atten = isSpec ? mk(1.0f, 1.0f, 1.0f) : xyz4(m.color);
            break;
        }
        case RT2_LIGHT: {
            f3 emitted = muls(xyz4(m.emissionColor), m.emissionStrength);
            L.incoming = add(L.incoming, mul(emitted, L.rayColor));
            L.pk |= RD_DONE;
            return;
        }
        case RT2_CHECKER: {
            L.d = normalize(add(normal, rnd_dir(L.seed)));
            float s = m.checkerScale;
            bool black = false;
            if (s > 0.0f) {
                float sum = floorf(L.o.x * s) + floorf(L.o.y * s) + floorf(L.o.z * s);
                float md = sum - 2.0f * floorf(sum / 2.0f);
                black = md == 0.0f;
            }
            atten = black ? mk(0.0f, 0.0f, 0.0f) : mk(1.0f, 1.0f, 1.0f);
            break;
        }
        case RT2_GLASS: {
            const bool inside = (L.pk & RD_INSIDE) != 0;
            float eta = inside ? m.refractiveIndex : 1.0f / m.refractiveIndex;
            bool refr;
            L.d = refract_(L.d, normal, eta, refr);
            if (refr) L.pk ^= RD_INSIDE;  // insideGlass = refr != insideGlass
            atten = xyz4(m.color);
            break;
        }
        default:  // GLASS_HIGHLIGHT and unknown types: trace() returns magenta
            L.incoming = mk(1.0f, 0.0f, 1.0f);
            L.pk |= RD_DONE;
            return;
        }
        if (m.isEdgeHighlight && bounce > 1)
            L.d = prevDir;
        else
            L.rayColor = mul(L.rayColor, atten);
        float pr = rt2pm_fmaxf(L.rayColor.x, rt2pm_fmaxf(L.rayColor.y, L.rayColor.z));
        if (rnd(L.seed) > pr) {
            L.pk |= RD_DONE;
            return;
        }
        L.rayColor = muls(L.rayColor, 1.0f / pr);
        if (bounce >= p.maxBounce) L.pk |= RD_DONE;
    } else {
        if (p.envLight) L.incoming = add(L.incoming, mul(sky(L.d), L.rayColor));
        L.pk |= RD_DONE;
    }
}

// Moves every lane's state to lane `to / 4` (ds_permute's byte address).
__device__ __forceinline__ void radiance_permute(RadLane& L, int to) {
    L.o = perm_f3(to, L.o);
    L.d = perm_f3(to, L.d);
    L.rayColor = perm_f3(to, L.rayColor);
    L.incoming = perm_f3(to, L.incoming);
    L.seed = (uint32_t)perm_i(to, (int)L.seed);
    L.pk = (uint32_t)perm_i(to, (int)L.pk);
}

template <OccSpec O>
__global__ __launch_bounds__(O.m.block) __attribute__((amdgpu_waves_per_eu(O.m.waves))) void radiance_rays_k5r(
    RenderParams p_arg, RadianceParams q) {
    constexpr MfmaSpec S = O.m;  // shade_rays_k5r's frame and records
    query_chunks<S>(q.n, [&](const RenderParams& p, const h8* rec, long long base, int live, MfmaDiag& dg,
                             unsigned long long& segs_w) {
        const int lane = (int)lane_id();
        RadLane L;
        {
            // lanes of a ragged last chunk hold the chunk's first ray and stream and never trace; tmax is not used
            float unused;
            query_load(q.rays, base + (lane < live ? lane : 0), L.o, L.d, unused);
            L.seed = q.rng[base + (lane < live ? lane : 0)];
        }
        L.rayColor = mk(1.0f, 1.0f, 1.0f);
        L.incoming = mk(0.0f, 0.0f, 0.0f);
        L.pk = lane < live ? (uint32_t)(lane + 1) << RD_SLOT_SHIFT : RD_DONE;  // bounce 0, insideGlass = false
        for (;;) {
            unsigned long long act = __ballot(!(L.pk & RD_DONE));
            if (!act) break;
            segs_w += (unsigned long long)__popcll(act);
            // at most 32 tracing lanes: move them to lanes 0..31 and sweep the first 32-ray block only
            bool upper = true;
            if (__popcll(act) <= 32) {
                if (act >> 32) {
                    const uint32_t nl = (uint32_t)__popcll(act);
                    const bool tr = (act >> lane) & 1ull;
                    radiance_permute(L, 4 * (int)(tr ? lanes_below(act) : nl + lanes_below(~act)));
                    act = __ballot(!(L.pk & RD_DONE));
                }
                upper = false;
            }
            // lanes that do not trace carry the first tracing lane's ray through the sweep
            const int j0 = __builtin_ctzll(act);
            const bool mine = !(L.pk & RD_DONE);
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
            if (mine) radiance_step(p, L, best, bi);
        }
        const int slot = (int)(L.pk >> RD_SLOT_SHIFT) - 1;
        if (slot >= 0) {  // one 16-byte store per ray and the stream's state, at the ray's own index
            *reinterpret_cast<float4*>(q.out + base + slot) =
                make_float4(L.incoming.x, L.incoming.y, L.incoming.z, __int_as_float((int)(L.pk & RD_BOUNCE)));
            q.rng[base + slot] = L.seed;
        }
    });
}

// One thread per ray: trace's loop around closest_any, then the record and the
// stream's state.  BVH: dynamic LDS = stack_slots * BLOCK ints (closest_bvh's stack).
template <int BLOCK, bool BVH>
__global__ __launch_bounds__(BLOCK) void radiance_rays_scalar(RenderParams p, RadianceParams q) {
    extern __shared__ int radiance_stack[];
    const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    uint32_t segs = 0, tests = 0, visits = 0;
    if (i < q.n) {
        RadLane L;
        float unused;  // tmax
        query_load(q.rays, i, L.o, L.d, unused);
        L.seed = q.rng[i];
        L.rayColor = mk(1.0f, 1.0f, 1.0f);
        L.incoming = mk(0.0f, 0.0f, 0.0f);
        L.pk = 0u;
        while (!(L.pk & RD_DONE)) {
            segs++;
            float best;
            int bi;
            closest_any<BLOCK, BVH>(p, L.o, L.d, radiance_stack, best, bi, tests, &visits);
            radiance_step(p, L, best, bi);
        }
        *reinterpret_cast<float4*>(q.out + i) =
            make_float4(L.incoming.x, L.incoming.y, L.incoming.z, __int_as_float((int)segs));
        q.rng[i] = L.seed;
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

struct PathRaysParams {
    float cam[3], vpRight[3], vpUp[3], vpFront[3], pixR[3], pixU[3], defR[3], defU[3];
    int W, H;
    int tile_rows, rank, nranks;
    uint32_t frame;
    int reseed;
    long long n;  // slab pixels
    uint32_t* rng;
    rt2_ray* out;
};

// One thread per slab pixel: the seed of compute.glsl:668 (with reseed), then
// advance's ST_NEW_RAY block (rt2_path.h), the same operations in the same
// order; two 16-B stores and the stream's state.
__global__ __launch_bounds__(256) void path_rays_kernel(PathRaysParams p) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= p.n) return;
    const int lr = (int)(i / p.W);
    const int x = (int)(i - (long long)lr * p.W);
    const int y = shard_row(lr, p.tile_rows, p.rank, p.nranks);
    uint32_t seed = p.reseed ? (uint32_t)x + (uint32_t)y * (uint32_t)p.W + p.frame * 968824447u : p.rng[i];
    const float px = (float)(x * 2 - p.W) / (float)p.W;
    const float py = (float)(y * 2 - p.H) / (float)p.H;
    const f3 endPoint = add(add(add(ld3(p.cam), ld3(p.vpFront)), muls(ld3(p.vpRight), px)), muls(ld3(p.vpUp), py));
    float ang = rnd(seed);
    float cs = rt2pm_cosf(ang), sn = rt2pm_sinf(ang);
    const f3 o = add(add(ld3(p.cam), muls(ld3(p.defR), cs)), muls(ld3(p.defU), sn));
    float jr = -0.5f + (0.5f - -0.5f) * rnd(seed);
    float ju = -0.5f + (0.5f - -0.5f) * rnd(seed);
    f3 endJ = add(add(endPoint, muls(ld3(p.pixR), jr)), muls(ld3(p.pixU), ju));
    const f3 d = normalize(sub(endJ, o));
    float4* w = reinterpret_cast<float4*>(p.out + i);
    w[0] = make_float4(o.x, o.y, o.z, 0.0f);  // tmax = 0: not used
    w[1] = make_float4(d.x, d.y, d.z, 0.0f);
    p.rng[i] = seed;
}

}  // namespace
