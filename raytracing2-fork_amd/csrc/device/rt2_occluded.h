// Occlusion queries (rt2_occluded): is anything in front of a caller's ray
// before its bound?  occluded[i] = (rt2_trace_rays' tri >= 0) for the same
// scene, traversal and ray, without the closest hit being found.
// Included by rt2_render.hip only (one translation unit; internal linkage).
//
// An occlusion query's bound never moves: it is the caller's bound_i from
// start to finish.  In the closest-hit scan best == bound_i until the first
// accept, and bi never returns to -1 after it, so stopping at the first accept
// gives that scan's `tri >= 0` in either traversal.  The matrix filter is
// conservative per (ray, triangle) pair against bestK = bound_i (1 + 2^-10),
// with or without the Y product, so the result is the OR of mt_pass3 && accept
// over the surviving pairs, in any order.
//
//   occluded_k5r<O>        brute force on the matrix filter, trace_rays_k5r's
//                          frame (rt2_query.h) around sweep_kt_occ: windows of
//                          O.win groups, an exact phase per ray (a lane stops
//                          at its first accept: any_window_lanes) or per wave
//                          (any_window_wave), and a wave that leaves the sweep
//                          after a window when none of its own rays is
//                          undecided
//   occluded_scalar<B,BVH> one thread per ray: the array scan in batches of 8
//                          that ends with the wave's last undecided ray, or
//                          any_bvh (closest_bvh's walk against the fixed
//                          bound, returning at the first accept)
//
// Chunks with a ray outside the filter's range or a non-finite component take
// the cooperative drain's exact code as in trace_rays_k5r (query_finite,
// coop_each) and convert bi >= 0: the path is rare.
#pragma once

namespace {

struct OccParams {
    const rt2_ray* rays;
    uint8_t* out;
    long long n;
};

// What distinguishes two occluded_k5r kernels.
struct OccSpec {
    MfmaSpec m;    // the frame: block, waves, res_l2, kt_lane_w; m.exact_win and m.y_first only decide whether
                   // res_load_records brings the T1 records (read by the Y product alone) into LDS
    int win;       // groups per window: products back to back, one exact episode, then the wave's exit test
    bool y_later;  // the Y product from the second window on (its fragment built once, after the first window, at the
                   // fixed bound); false: no Y product at all (6 products per group)
    bool per_wave = false;  // the episode tests every hot triangle on the whole wave, the triangle through the scalar
                            // cache (any_window_wave: trace_rays_k5r's exact_window without its updates), instead of
                            // per ray (any_window_lanes)
};

// mt_exact's acceptance (compute.glsl:312-327 on the phase-1 intermediates, the same operations in the same order)
// against a fixed bound: nothing is updated.
__device__ __forceinline__ bool mt_accept(const MtQ& q, float bound) {
    if ((q.det < 1e-10f && q.det > -1e-10f) || q.det < 0.0f) return false;
    const float inv = 1.0f / q.det;
    const float dst = q.tnum * inv;
    const float u = -q.U * inv;
    const float v = q.V * inv;
    return !(dst <= 1e-6f) && !(u < 0.0f || v < 0.0f || 1.0f - u - v < 0.0f) && dst < bound;
}

// The any-hit episode of one window: exact_window_lanes' compaction, gather,
// transposed products and pack (rt2_k5_resident.h; the same list, operands and
// bit order), then every lane walks its own bits until its first accept.
// `live`: the lane holds a ray of its own and is undecided; other lanes (the
// padding of a ragged chunk, lanes 32..63 when upper = false, decided rays)
// drop their pairs.  The rounds end early when no live lane is left.
template <MfmaSpec S, bool YP, bool LDS>
__device__ __forceinline__ void any_window_lanes(int maskv, int Gw, int n_tris, const float4* tri4, const h8* a0,
                                                 const h8* y1, const h8* recs, bool upper, bool mine, const f3& o,
                                                 const f3& d, float bound, float bestK, bool& occ) {
    const int lane = (int)lane_id();
    // padding slots of the scene's last group never enter the list
    if (n_tris & 31) maskv = lane == (n_tris >> 5) - Gw ? maskv & (int)((1u << (n_tris & 31)) - 1u) : maskv;
    unsigned long long hotg = __ballot(maskv != 0);
    const int src = 4 * xl_bit_of_row(lane & 31);  // ds_bpermute address of the list entry this lane gathers
    const f16v zero = {};
    uint32_t m = 0;  // the current group's triangles still to be listed
    int gj = 0;      // ... its lane of maskv
#pragma nounroll
    for (;;) {
        int lst = 0, c = 0;
#pragma nounroll
        while (c < 32) {
            if (!m) {
                if (!hotg) break;
                gj = __builtin_ctzll(hotg);
                hotg &= hotg - 1;
                m = (uint32_t)__builtin_amdgcn_readlane(maskv, gj);
            }
            const int idx = 32 * (Gw + gj) + __builtin_ctz(m);
            m &= m - 1;
            lst = lane == c ? idx : lst;
            c++;
        }
        if (!c) break;
        const int T = __builtin_amdgcn_ds_bpermute(src, lst);
        const h8* rp = recs + ((T >> 5) * (kKtOps * 64) + (T & 31) + (lane & 32));
        auto block = [&](int R) {
            int t3[16];
            {
                const f16v U = __builtin_amdgcn_mfma_f32_32x32x16_f16(rp[0], a0[R], zero, 0, 0, 0);
                const f16v V = __builtin_amdgcn_mfma_f32_32x32x16_f16(rp[64], a0[R], zero, 0, 0, 0);
                const f16v X = __builtin_amdgcn_mfma_f32_32x32x16_f16(rp[128], a0[R], zero, 0, 0, 0);
#pragma unroll
                for (int i = 0; i < 16; i++)  // U & V & X, as kt_group
                    t3[i] = __builtin_amdgcn_bitop3_b32(__float_as_int(U[i]), __float_as_int(V[i]),
                                                        __float_as_int(X[i]), 0x80);
            }
            if constexpr (YP) {
                asm volatile("" : "+v"(t3[0]), "+v"(t3[1]), "+v"(t3[2]), "+v"(t3[3]), "+v"(t3[4]), "+v"(t3[5]),
                             "+v"(t3[6]), "+v"(t3[7]), "+v"(t3[8]), "+v"(t3[9]), "+v"(t3[10]), "+v"(t3[11]),
                             "+v"(t3[12]), "+v"(t3[13]), "+v"(t3[14]), "+v"(t3[15]));
                const f16v Yt = __builtin_amdgcn_mfma_f32_32x32x16_f16(rp[192], y1[R], zero, 0, 0, 0);
#pragma unroll
                for (int i = 0; i < 16; i++) t3[i] &= __float_as_int(Yt[i]);
            }
            int mk = 0;
#pragma unroll
            for (int i = 15; i >= 0; i--)  // mk << 1 | sign: register i ends in bit i
                mk = (int)__builtin_amdgcn_alignbit((uint32_t)mk, (uint32_t)t3[i], 31);
            asm volatile("" : "+v"(mk));
            return mk;
        };
        const int mk0 = block(0);
        int mk1 = 0;
        if (upper) mk1 = block(1);
        // lanes 0..31: block 0's two halves of ray l; lanes 32..63: block 1's
        const auto sw = __builtin_amdgcn_permlane32_swap((uint32_t)mk0, (uint32_t)mk1, false, false);
        uint32_t pm = (sw[0] | sw[1] << 16) & (c == 32 ? ~0u : (1u << c) - 1u);
        if (!mine || occ) pm = 0;
        // The lane's pairs, lowest bit first, the next pair's triangle requested before the current test runs (a lane
        // without a further bit reads entry 31 of the list, a valid index or 0, and never uses it).
        auto entry = [&](uint32_t m) { return __builtin_amdgcn_ds_bpermute(4 * __builtin_ctz(m | 0x80000000u), lst); };
        struct Tri {
            int idx;
            float4 t0, t1, t2;
        };
        auto fetch = [&](Tri& t) {
            t.idx = entry(pm);
            t.t0 = tri4[3 * t.idx], t.t1 = tri4[3 * t.idx + 1], t.t2 = tri4[3 * t.idx + 2];
        };
        auto step = [&](const Tri& cur, Tri& nxt) {
            const bool has = pm != 0;
            pm &= pm - 1;
            fetch(nxt);
            if (has) {
                const MtQ qq = mt_quantities(o, d, cur.t0, cur.t1, cur.t2);
                if (mt_pass3(qq, bestK) && mt_accept(qq, bound)) {
                    occ = true;
                    pm = 0;  // the first accept decides the ray: its other pairs are dropped
                }
            }
        };
        Tri ta, tb2;
        fetch(ta);
#pragma nounroll
        while (__ballot(pm != 0)) {
            step(ta, tb2);
            if (!__ballot(pm != 0)) break;
            step(tb2, ta);
        }
        if (c < 32 || !__ballot(mine && !occ)) break;
    }
}

// The any-hit episode of one window per wave (OccSpec::per_wave): exact_window's
// walk (rt2_k5_resident.h: group Gw + j's hot mask is lane j of maskv, the
// groups ascending, each triangle read once through the scalar cache and tested
// by all 64 lanes) with a fixed bound and no updates.  A lane's flag is set at
// its first accept; the walk ends after a group when no lane that holds a ray
// of its own is undecided.  Costs nothing where no group is hot, and per hot
// triangle what one test costs, whatever the number of rays that asked for it.
__device__ __forceinline__ void any_window_wave(int maskv, int Gw, int cnt, int n_tris, cfloat* tri, bool mine,
                                                const f3& o, const f3& d, float bound, float bestK, bool& occ) {
    for (int j = 0; j < cnt; j++) {
        uint32_t m32 = (uint32_t)__builtin_amdgcn_readlane(maskv, j);
        if (!m32) continue;
        while (m32) {
            const int tt = __builtin_ctz(m32);
            m32 &= m32 - 1;
            const int idx = 32 * (Gw + j) + tt;
            if (idx >= n_tris) break;  // the padding slots of the scene's last group
            cfloat* tp = tri + 12 * idx;
            const MtQ qq = mt_quantities(o, d, ldc4(tp), ldc4(tp + 4), ldc4(tp + 8));
            if (mt_pass3(qq, bestK) && mt_accept(qq, bound)) occ = true;
        }
        if (!__ballot(mine && !occ)) return;
    }
}

// Whether each lane's ray is occluded before `bound`, records from LDS (and,
// res_l2, the groups beyond kResGroups from L2): sweep_kt_res's ray setup and
// products (kt_group, unchanged) in windows of O.win groups with a constant
// bestK.  After each window the wave leaves when no lane that holds a ray of
// its own (`mine`) is undecided; the loops are bounded by the group count.
// Returns false (wave-uniform, nothing computed) when a ray is outside the
// filter's range.
template <OccSpec O>
__device__ __forceinline__ bool sweep_kt_occ(const RenderParams& p, const h8* rec, const f3& o, const f3& d,
                                             float bound, float bestK, bool upper, bool mine, bool& occ) {
    constexpr MfmaSpec S = O.m;
    constexpr int W = O.win;
    static_assert(W >= 2 && W <= 64, "a window's masks are the lanes of one VGPR");
    const int lane = (int)lane_id();
    const f3 m = cross(d, o);
    MfmaScale sc;
    if (!mfma_scale<true>(p.mfma_A, o, d, m, sc)) return false;
    h8 a0[2], y1[2];
    _Float16 tw16;
    kt_frags<S.kt_lane_w>(d, m, sc, a0, tw16);
    const int ng = (p.n_tris + 31) >> 5, n_tris = p.n_tris;
    const int nres = S.res_l2 ? min(ng, kResGroups) : ng;
    const float4* tri4 = reinterpret_cast<const float4*>(p.tri);
    const h8* const l2 = reinterpret_cast<const h8*>(p.mfma_kt_frag);
    // one window of cnt groups from Gw on, records at tb (advanced)
    auto window = [&](auto yp, auto lds, const h8*& tb, int Gw, int cnt) {
        constexpr bool YP = decltype(yp)::value;
        constexpr bool LDS = decltype(lds)::value;
        int maskv = 0;
        uint32_t any = 0;
        for (int j = 0; j < cnt; j++) {
            const h8 b0 = tb[0], b1 = tb[64], b2 = tb[128];
            h8 b3 = {};
            if constexpr (YP) b3 = tb[192];
            tb += kKtOps * 64;
            const unsigned long long M = kt_group<YP>(a0, y1, b0, b1, b2, b3, upper);
            const uint32_t m32 = (uint32_t)(M | M >> 32);
            maskv = lane == j ? (int)m32 : maskv;
            any |= m32;
        }
        if (any) {
            phase_prio<S>(1);
            if constexpr (O.per_wave) {
                any_window_wave(maskv, Gw, cnt, n_tris, (cfloat*)p.tri, mine, o, d, bound, bestK, occ);
            } else {
                const h8* recs = l2;  // the episode gathers from the window's own records
                if constexpr (LDS) recs = rec;
                any_window_lanes<S, YP, LDS>(maskv, Gw, n_tris, tri4, a0, y1, recs, upper, mine, o, d, bound, bestK,
                                             occ);
            }
            phase_prio<S>(0);
        }
    };
    // The windows over the groups [Gw, G1), none of them straddling G1; false: the wave is done.
    auto windows = [&](auto yp, auto lds, const h8* tb, int& Gw, int G1) {
        while (Gw < G1) {
            const int cnt = min(W, G1 - Gw);
            window(yp, lds, tb, Gw, cnt);
            Gw += cnt;
            if (!__ballot(mine && !occ)) return false;
        }
        return true;
    };
    int Gw = 0;
    if constexpr (!O.y_later) {
        if (!windows(std::false_type{}, std::true_type{}, rec + lane, Gw, nres)) return true;
        if constexpr (S.res_l2)
            windows(std::false_type{}, std::false_type{}, l2 + (size_t)nres * (kKtOps * 64) + lane, Gw, ng);
    } else {
        // the first window without Y; its fragment is built once, when groups follow and a ray is undecided
        const h8* tb = rec + lane;
        const int cnt = min(W, nres);
        window(std::false_type{}, std::true_type{}, tb, 0, cnt);
        Gw = cnt;
        if (Gw >= ng || !__ballot(mine && !occ)) return true;
        kt_y(d, o, bestK, sc, tw16, y1);
        if (!windows(std::true_type{}, std::true_type{}, tb, Gw, nres)) return true;
        if constexpr (S.res_l2)
            windows(std::true_type{}, std::false_type{}, l2 + (size_t)nres * (kKtOps * 64) + lane, Gw, ng);
    }
    return true;
}

template <OccSpec O>
__global__ __launch_bounds__(O.m.block) __attribute__((amdgpu_waves_per_eu(O.m.waves))) void occluded_k5r(RenderParams p_arg,
                                                                                                         OccParams q) {
    constexpr MfmaSpec S = O.m;
    query_chunks<S>(q.n, [&](const RenderParams& p, const h8* rec, long long base, int live, MfmaDiag&,
                               unsigned long long& segs_w) {
        const int lane = (int)lane_id();
        const bool mine = lane < live;
        const unsigned long long act = live == 64 ? ~0ull : (1ull << live) - 1ull;
        // lanes of a ragged last chunk carry the chunk's first ray (and its bound)
        f3 o, d;
        float bound;
        query_load(q.rays, base + (mine ? lane : 0), o, d, bound);
        bool occ = false, swept = false;
        if (!__ballot(!query_finite(o, d)))
            swept = sweep_kt_occ<O>(p, rec, o, d, bound, bound * 1.0009765625f, live > 32, mine, occ);
        if (!swept) {
            // a ray outside the filter's range or not finite (wave-uniform): the drain's exact code
            float best = bound;
            int bi = -1;
            coop_each(act, o, d, p, best, bi, &bound);
            occ = bi >= 0;
        }
        if (mine) q.out[base + lane] = occ ? (uint8_t)1 : (uint8_t)0;  // one byte per live lane
        segs_w += (unsigned long long)live;
    });
}

// calculateRayCollisionBVH (closest_bvh: the same visiting order, the same
// pruning) against the fixed bound `best`, returning at the first accept.
// tests: the leaf triangles tested up to the exit; visits: interior nodes.
template <int BLOCK>
__device__ __forceinline__ bool any_bvh(const f3& o, const f3& d, const rt2_node* __restrict__ nodes,
                                        const float4* __restrict__ tri, int* stack, int stack_slots, float best,
                                        uint32_t& tests, uint32_t& visits) {
    const bool sx = d.x < 1e-6f && d.x > -1e-6f;
    const bool sy = d.y < 1e-6f && d.y > -1e-6f;
    const bool sz = d.z < 1e-6f && d.z > -1e-6f;
    const float bestK = best * 1.0009765625f;
    int* st = stack + threadIdx.x;
    int sp = 0;
    st[0] = 0;
    sp = 1;
    while (sp > 0) {
        sp -= 1;
        const int ni = st[sp * BLOCK];
        const int4 meta = *reinterpret_cast<const int4*>(&nodes[ni].triangleIndex);
        if (meta.z == -1) {  // leaf: compute.glsl:429-435
            for (int i = meta.x; i < meta.x + meta.y; i++) {
                const float4* t = tri + 3 * i;
                const MtQ q = mt_quantities(o, d, t[0], t[1], t[2]);
                tests++;
                if (mt_pass(q, bestK) && mt_accept(q, best)) return true;
            }
        } else {  // compute.glsl:441-456
            visits++;
            const int ia = meta.z, ib = meta.z + 1;
            const float dA = ray_bounds(o, d, sx, sy, sz, nodes[ia].bmin, nodes[ia].bmax);
            const float dB = ray_bounds(o, d, sx, sy, sz, nodes[ib].bmin, nodes[ib].bmax);
            const bool nearA = dA < dB;
            const float dNear = nearA ? dA : dB;
            const float dFar = nearA ? dB : dA;
            const int iNear = nearA ? ia : ib;
            const int iFar = nearA ? ib : ia;
            if (dFar < best && sp < stack_slots) st[(sp++) * BLOCK] = iFar;
            if (dNear < best && sp < stack_slots) st[(sp++) * BLOCK] = iNear;
        }
    }
    return false;
}

// One thread per ray.  BVH: dynamic LDS = stack_slots * BLOCK ints (any_bvh's stack).
template <int BLOCK, bool BVH>
__global__ __launch_bounds__(BLOCK) void occluded_scalar(RenderParams p, OccParams q) {
    extern __shared__ int occ_stack[];
    const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    const bool live = i < q.n;
    uint32_t tests = 0, visits = 0;
    f3 o = mk(0.0f, 0.0f, 0.0f), d = o;
    float bound = 1e38f;
    if (live) query_load(q.rays, i, o, d, bound);
    bool occ = false;
    if constexpr (BVH) {
        if (live) occ = any_bvh<BLOCK>(o, d, p.nodes, p.tri, occ_stack, p.stack_slots, bound, tests, visits);
    } else {
        // the array scan through the scalar cache, 8 triangles per batch (wave-uniform trip count: every lane stays
        // until the wave's last undecided ray is decided or the array ends)
        const float bestK = bound * 1.0009765625f;
        cfloat* const tri = (cfloat*)p.tri;
        for (int t0 = 0; t0 < p.n_tris; t0 += 8) {
#pragma unroll
            for (int k = 0; k < 8; k++) {
                if (t0 + k < p.n_tris) {
                    cfloat* tp = tri + 12 * (t0 + k);
                    const MtQ qq = mt_quantities(o, d, ldc4(tp), ldc4(tp + 4), ldc4(tp + 8));
                    if (mt_pass3(qq, bestK) && mt_accept(qq, bound)) occ = true;
                }
            }
            if (!__ballot(live && !occ)) break;
        }
    }
    if (live) q.out[i] = occ ? (uint8_t)1 : (uint8_t)0;
    unsigned long long s = live, t = tests, v = visits;
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
