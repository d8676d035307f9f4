// The matrix filter with the threshold in the K-slots (rt2_mfma.h) and its
// record operands streamed through workgroup-shared LDS tiles: the north
// star's "triangle arrays streamed from HBM in coalesced tiles and staged in
// LDS".  Included by rt2_render.hip only (one translation unit; internal
// linkage).
//
// What it replaces: in render_mfma every wave loads its own copy of each
// 32-triangle group's records from L2/MALL — for a 100k-triangle scene 12.8 MB
// per wave-segment, about 2 B per (ray, triangle) pair, half of it missing the
// L2 (DESIGN.md, config C PMC).  The reference reads `triangles[i]` from SSBO
// 1 in every leaf test (compute.glsl:429-431, block :75-78).
//
// Here the NW waves of a workgroup (one workgroup per CU) sweep the same
// records in the same order, so each tile of K groups is brought into LDS
// once per workgroup and segment, by LDS-DMA (global_load_lds_dwordx4: 1-KiB
// coalesced pieces, no VGPRs), split across the waves and double-buffered:
// tile t+1 is in flight while tile t is swept.  The record traffic from L2
// falls NW-fold.  The ray fragments are built in registers (frag_pair) and
// the path state stays in registers too.  The arithmetic of every product,
// threshold and exact test is render_mfma_k5r's term for term, so the result
// is the sequential strict `dst < best` scan's bit for bit.
#pragma once

namespace {

// LDS of one workgroup's record tiles: kTileBufs buffers x K groups x the 4
// kt operands (U, -V, X, T1) as 64 lanes x 16 B
constexpr int kTileBufs = 2;
template <int K>
struct K5Tiles {
    h8 rec[kTileBufs][K * 4 * 64];
};

__device__ __forceinline__ void wait_vm0() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// The record tiles as a stream with LDS counters instead of a workgroup
// barrier per tile (DESIGN.md "LDS record tiles").  With one barrier per tile
// the 12 waves meet 165 times per config C segment and wait for the slowest
// of them every time.  Here a wave waits only for
// the tile it is about to read: the waves drift apart by up to a tile and a
// wave that is behind is not waited for until it holds the stream up.
//
// Every wave walks the same stream of tiles (stream index s: tile s % nt of
// the segment, buffer s % NB; a segment is nt consecutive indices, so the
// index runs on across segments) and, per tile: waits until all NW shares of
// tile s have landed in buffer b (landed[b] == NW * (s / NB + 1)), sweeps it
// (when it has rays), and releases it (rel[b] += 1).  Each wave issues its own
// share of each tile's LDS-DMA pieces (pc = wave, wave + NW, ...) once every
// wave has released the buffer's previous tile (rel[b] == NW * (s / NB)), and
// publishes the share (landed[b] += 1) after its own `s_waitcnt vmcnt(0)`, two
// groups later or at once when it is waiting anyway.  No wave reads a buffer
// before every share of its tile has landed, and no DMA overwrites a buffer
// before all NW waves released it.  MfmaSpec::flow_prio: a wave's issue
// priority for the next tile follows its finishing rank in this one (the
// last to finish take the SIMD's issue slots first).
struct TileFlow {
    uint32_t landed[kTileBufs];  // per buffer: shares landed so far (NW per tile)
    uint32_t rel[kTileBufs];     // per buffer: releases so far (NW per tile)
};
// the wave's place in the stream (wave-uniform; kept across segments)
struct FlowWave {
    uint32_t next = 0;        // stream index of the next tile this wave reads
    uint32_t next_issue = 0;  // ... of the next tile this wave issues its share of
    int pend = -1;            // a share issued whose landing is not published yet
    int age = 0;              // groups swept since that share was issued
};

__device__ __forceinline__ uint32_t lds_acquire(uint32_t* a) {
    return __builtin_amdgcn_readfirstlane(__hip_atomic_load(a, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP));
}

template <MfmaSpec S, class TL, class FL>
__device__ __forceinline__ bool sweep_kt_flow(const RenderParams& p, TL& tl, FL& fl, FlowWave& fw, const f3& o,
                                              const f3& d, float& best, int& bi, float& bestK, MfmaDiag& dg,
                                              bool sweeping, bool upper) {
    static_assert(S.tile_groups > 0, "groups per tile");
    constexpr int K = S.tile_groups, NW = S.block / 64, NB = kTileBufs;
    static_assert((NB & (NB - 1)) == 0 && NW % 2 == 0, "stream counters: NB a power of two, NW even (wrap-safe)");
    const int lane = (int)lane_id(), wave = (int)(threadIdx.x >> 6);
    // MfmaSpec::diag: shader clocks per phase (MfmaDiag t_wait / t_filt / t_exact / t_swp)
    [[maybe_unused]] unsigned long long tc = 0, tsw = 0;
    if constexpr (S.diag) tsw = tc = __builtin_amdgcn_s_memtime();
    auto stamp = [&](unsigned long long& acc) {
        if constexpr (S.diag) {
            const unsigned long long t = __builtin_amdgcn_s_memtime();
            acc += t - tc;
            tc = t;
        }
    };
    MfmaScale sc{0.0f, 0.0f, 0.0f};
    h8 a0[2], y1[2];
    _Float16 tw16 = (_Float16)0.0f;
    bool compute = false, in_range = true;
    if (sweeping) {
        const f3 m = cross(d, o);
        in_range = mfma_scale<true>(p.mfma_A, o, d, m, sc);
        if (in_range) {
            kt_frags<S.kt_lane_w>(d, m, sc, a0, tw16);
            kt_y(d, o, bestK, sc, tw16, y1);
            compute = true;
        }
    }
    const int ng = (p.n_tris + 31) >> 5, nt = (ng + K - 1) / K;
    const h8* gsrc = reinterpret_cast<const h8*>(p.mfma_kt_frag) + lane;
    // this wave's share of stream index s: pieces pc = wave, wave + NW, ...
    // (4 per group, 1 KiB each: a lane's 16 B land at base + 16 lane); the kt
    // records of a tile are contiguous
    auto issue_share = [&](uint32_t s) {
        const int g0 = (int)(s % (uint32_t)nt) * K, gn = min(K, ng - g0), b = (int)(s % NB);
        const h8* src = gsrc + (size_t)g0 * (kKtOps * 64);
        for (int pc = wave; pc < kKtOps * gn; pc += NW)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + pc * 64),
                                             (__attribute__((address_space(3))) void*)&tl.rec[b][pc * 64], 16, 0, 0);
    };
    // the wave's part of the stream's upkeep: publish a share that has had
    // time to land (`force`: now), then issue the next share once every wave
    // has released that tile's buffer
    auto upkeep = [&](bool force, bool try_issue) {
        if (fw.pend >= 0 && (force || fw.age >= 2)) {
            [[maybe_unused]] unsigned long long t0 = 0;
            if constexpr (S.diag) t0 = __builtin_amdgcn_s_memtime();
            wait_vm0();  // this wave's pieces (its only vector-memory operations in flight) have landed
            if constexpr (S.diag) dg.t_pub += __builtin_amdgcn_s_memtime() - t0;
            if (lane == 0)
                __hip_atomic_fetch_add(&fl.landed[fw.pend % NB], 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
            fw.pend = -1;
        }
        if (fw.pend < 0 && try_issue) {
            const uint32_t s = fw.next_issue;
            if (lds_acquire(&fl.rel[s % NB]) == (uint32_t)NW * (s / NB)) {
                [[maybe_unused]] unsigned long long t0 = 0;
                if constexpr (S.diag) t0 = __builtin_amdgcn_s_memtime();
                issue_share(s);
                if constexpr (S.diag) {
                    dg.t_issue += __builtin_amdgcn_s_memtime() - t0;
                    dg.claims += 1;
                }
                fw.pend = (int)s;
                fw.age = 0;
                fw.next_issue = s + 1u;
            }
        }
    };
    for (int t = 0; t < nt; t++) {
        const uint32_t s = fw.next++;
        const int b = (int)(s % NB), gn = min(K, ng - t * K);
        stamp(dg.t_exact);
        upkeep(true, true);
        // (wrap-safe: the counters and stream index are 32-bit and may wrap in
        // a launch of hours; NB and NW even keep NW * (s / NB) consistent mod 2^32)
        // (bounded: a wait of 2^24 sleeps, ~1 s, cannot be a slow wave — a
        // tile takes ~20-40 k clocks — so the kernel traps instead of hanging)
        uint32_t spins = 0;
        while ((int32_t)(lds_acquire(&fl.landed[b]) - (uint32_t)NW * (s / NB + 1u)) < 0) {
            upkeep(true, true);
            __builtin_amdgcn_s_sleep(1);
            if (++spins == (1u << 24)) __builtin_trap();
        }
        stamp(dg.t_wait);
        if (compute) {
            const h8* tb = &tl.rec[b][lane];
            for (int gi = 0; gi < gn; gi++) {
                const int G = t * K + gi;
                const h8 b0 = tb[0], b1 = tb[64], b2 = tb[128], b3 = tb[192];
                tb += kKtOps * 64;
                fw.age++;
                upkeep(false, gi == K / 2);
                const unsigned long long M = kt_group(a0, y1, b0, b1, b2, b3, upper);
                if constexpr (S.diag) dg.groups += 1;
                stamp(dg.t_filt);
                if (M) {
                    if constexpr (S.diag) dg.hot += 1;
                    // the exact phase, in index order (compute.glsl:302-340, strict `dst < best`)
                    uint32_t m32 = (uint32_t)(M | M >> 32);
                    const float bk0 = bestK;
                    while (m32) {
                        const int idx = 32 * G + __builtin_ctz(m32);
                        m32 &= m32 - 1;
                        if (idx >= p.n_tris) break;
                        if constexpr (S.diag) dg.exact += 1;
                        cfloat* tp = (cfloat*)p.tri + 12 * idx;
                        const MtQ qq = mt_quantities(o, d, ldc4(tp), ldc4(tp + 4), ldc4(tp + 8));
                        if (mt_pass3(qq, bestK)) mt_exact(qq, idx, best, bi, bestK);
                    }
                    if (__ballot(bestK != bk0)) kt_y(d, o, bestK, sc, tw16, y1);
                    stamp(dg.t_exact);
                }
            }
        }
        // done with buffer b (the LDS executes this wave's reads before the add)
        uint32_t r_old = 0;
        if (lane == 0) r_old = __hip_atomic_fetch_add(&fl.rel[b], 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        if constexpr (S.flow_prio) {
            const int rank = (int)(__builtin_amdgcn_readfirstlane(r_old) - (uint32_t)NW * (s / NB));
            const int q = rank * 4 / NW;
            if (q >= 3)
                __builtin_amdgcn_s_setprio(3);
            else if (q == 2)
                __builtin_amdgcn_s_setprio(2);
            else if (q == 1)
                __builtin_amdgcn_s_setprio(1);
            else
                __builtin_amdgcn_s_setprio(0);
        }
    }
    if constexpr (S.flow_prio) __builtin_amdgcn_s_setprio(0);
    stamp(dg.t_exact);
    if constexpr (S.diag) dg.t_swp += __builtin_amdgcn_s_memtime() - tsw;
    return in_range;
}

// render_mfma's lockstep segment loop around sweep_kt_flow: every wave of the
// workgroup walks the tile stream of every segment the workgroup runs
// (block_any decides, workgroup-uniformly, whether it runs one), sweeping
// only when it has rays and is not in the cooperative drain.  The path state
// stays in registers.
template <MfmaSpec S>
__global__ __launch_bounds__(S.block) __attribute__((amdgpu_waves_per_eu(S.waves))) void render_mfma_k5t(RenderParams p_arg) {
    constexpr int NW = S.block / 64;
    __shared__ K5Tiles<S.tile_groups> tl;
    __shared__ BlockVote<NW> vote;
    __shared__ TileFlow flow;  // the tile stream's counters (sweep_kt_flow)
    FlowWave fw;
    if (threadIdx.x == 0) {
        for (int b = 0; b < kTileBufs; b++) flow.landed[b] = flow.rel[b] = 0;
    }
    __syncthreads();
    uint32_t vote_parity = 0;
    Lane L;
    lane_init(L);
    MfmaDiag dg;
    [[maybe_unused]] unsigned long long t_start = 0;
    if constexpr (S.diag) t_start = __builtin_amdgcn_s_memtime();
    // MfmaSpec::lean (as in render_mfma_k5r): x, y recomputed from the item,
    // the wave counts its lanes' segments
    [[maybe_unused]] unsigned long long segs_w = 0;
    for (;;) {
        const RenderParams& p = kargs<RenderParams>();
        advance<1, !S.lean, false, false, S.linear>(L, p);
        unsigned long long act = __ballot(L.st == ST_TRACE);
        if (!block_any<NW>(act != 0, vote, vote_parity)) break;
        if constexpr (S.lean) segs_w += (unsigned long long)__popcll(act);
        const bool coop = act != 0 && __popcll(act) <= (unsigned)S.tail_lanes && __any(L.st == ST_DONE);
        const bool sweeping = act != 0 && !coop;
        bool upper = true;
        if (sweeping && __popcll(act) <= 32) {
            if (act >> 32) {
                const uint32_t l = lane_id(), nl = (uint32_t)__popcll(act);
                const bool live = (act >> l) & 1ull;
                const int to = 4 * (int)(live ? lanes_below(act) : nl + lanes_below(~act));
                lane_permute<!S.lean, !S.lean>(L, to);
                act = __ballot(L.st == ST_TRACE);
            }
            upper = false;
        }
        const bool mine = L.st == ST_TRACE;
        if (sweeping) {
            // lanes without a ray carry the first live lane's (ST_DONE lanes
            // never read their o, d again)
            const int j0 = __builtin_ctzll(act);
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
        const bool swept = sweep_kt_flow<S>(p, tl, flow, fw, ro, rd, best, bi, bestK, dg, sweeping, upper);
        L.o = ro;
        L.d = rd;
        if (coop) {
            float mybest = 1e38f;
            int mybi = -1;
            coop_each(act, L.o, L.d, p, mybest, mybi);
            if (mine) {
                L.bounce += 1;
                if constexpr (!S.lean) L.segs += 1;
                shade<1, false, S.linear>(L, p, mybest, mybi);
            }
            continue;
        }
        if (!act) continue;
        if (!swept) coop_each(act, ro, rd, p, best, bi);
        if (mine) {
            L.bounce += 1;
            if constexpr (!S.lean) L.segs += 1;
            shade<1, false, S.linear>(L, p, best, bi);
        }
    }
    // a share of the next segment's first tiles may still be in flight; it
    // must land before the workgroup's LDS is given back
    wait_vm0();
    const RenderParams& p = kargs<RenderParams>();
    if constexpr (S.lean) {
        if (lane_id() == 0) atomicAdd(p.seg_counter, segs_w);
    } else {
        flush_counters(L, p);
    }
    if constexpr (S.diag)
        if (lane_id() == 0) {
            atomicAdd(p.seg_counter + 1, dg.groups);  // (wave, triangle group) sweeps
            atomicAdd(p.seg_counter + 2, dg.hot);     // ... with a passing pair
            atomicAdd(p.seg_counter + 3, dg.exact);   // (wave, triangle) exact tests
            atomicAdd(p.seg_counter + 12, dg.t_wait);  // shader clocks: waiting for tiles
            atomicAdd(p.seg_counter + 13, dg.t_filt);  // ... products + record reads
            atomicAdd(p.seg_counter + 14, dg.t_exact); // ... exact phase + Y rebuilds (+ loop)
            atomicAdd(p.seg_counter + 15, dg.t_swp);   // ... whole sweeps
            atomicAdd(p.seg_counter + 16, __builtin_amdgcn_s_memtime() - t_start);  // ... the wave's life
            atomicAdd(p.seg_counter + 17, dg.t_issue);  // ... issuing claimed tiles (inside wait / filter)
            atomicAdd(p.seg_counter + 18, dg.t_pub);    // ... a claimer's wait for its pieces (inside wait)
            atomicAdd(p.seg_counter + 19, dg.claims);   // tiles claimed
        }
}

}  // namespace
