// The matrix filter for scenes whose records fit the LDS: every 32-triangle
// group's four record operands (4 KiB; the kt records of rt2_mfma.h, the
// threshold in the K-slots) are brought into the workgroup's LDS ONCE per
// launch and every wave sweeps them from there for the rest of the launch.
// Included by rt2_render.hip only (one translation unit; internal linkage).
//
// Why: a kernel whose waves read the records from L2 (render_mfma) re-reads
// the whole scene's records in every wave-segment — config B's 38 groups are
// 152 KiB per wave and segment, 16 waves per CU — and 38 % of its wave cycles
// wait on those loads or the segment barrier; the LDS-tiled
// kernel (render_mfma_k5t) shares them per segment but pays for the tile
// stream.  Here the 152 KiB stay in LDS: no record traffic to L2 after the
// launch's first microseconds, no barrier after the initial one (waves run
// free: each leaves when its own lanes are done and the item pool is dry),
// and a group's operands are 4 conflict-free ds_read_b128 per lane (~100
// cycles) instead of L2 loads.  MfmaSpec::res_l2: a scene of more than
// kResGroups groups keeps its first kResGroups resident and reads the rest
// per wave from L2 after them (up to 256 groups).
//
// The LDS then has no room for fragment rows, so the ray fragments are built
// in registers: each lane forms its own ray's 16 k-slots (the rows' exact
// f16 values) and one v_permlane32_swap per dword exchanges halves between
// lanes l and l + 32, which yields the MFMA A-operand layout of both 32-ray
// blocks at once (frag_pair).  The Y fragment is rebuilt the same way when a
// lane's bound improves: no LDS, no wave barrier.
//
// The filter only decides which (wave, triangle) pairs skip the exact test;
// the exact phase is the reference arithmetic in index order, so the image is
// the sequential strict `dst < best` scan's bit for bit.  Reference:
// compute.glsl:429-434 (the `triangles[i]` loop this sweep replaces).
//
// The exact phase runs once per window of MfmaSpec::exact_win groups, not
// once per hot group: the window's products run back to back (no branch, no
// priority flip, no Y rebuild between its groups), each group's 32-bit hot
// mask is parked in a lane of one VGPR, and one episode then tests the
// window's survivors, groups ascending and indices ascending within a group,
// and rebuilds Y once if a bound improved and groups remain (never after the
// sweep's last group).  The shipped kernels take a window of kResGroups: the
// resident sweep is one stretch of products and one episode; the L2 loop's
// windows start again at group kResGroups.
// Why this is exact: inside a window the Y fragment carries the bound the
// window started with, which is >= the bound the per-group form would use at
// each of its groups.  The filter's guarantee is that it never rejects a pair
// the reference would accept under the bound it was given, and a looser bound
// only passes more pairs; those are decided by mt_pass3 / mt_exact against the
// current bound, in index order, like every other survivor.  The price is
// more tests (config B: 0.686 per (wave, group) against 0.634).
//
// A sweep's first window runs without the Y product (kt_group<false>): every
// sweep starts with no distance bound, nothing rebuilds Y inside a window, so
// Y there is the det > 0 test, which U, -V, X < 0 imply up to the thresholds
// (rt2_mfma.h kt_group).  Leaving a term out of the conjunction only passes
// more pairs.  The Y fragment is first built after that window, when groups
// follow it; in a kernel whose first window is the whole scene (353, 354) it
// never exists and the T1 records are not brought into LDS.
// MfmaSpec::y_first keeps the Y product there (the A/B arms).
//
// MfmaSpec::exact_lanes (353, 354): the episode tests per ray, not per wave.
// A hot triangle is hot for about 3 of the wave's 64 rays, so the window's hot
// triangles are compacted into synthetic groups of 32 whose products, with the
// operands exchanged, give every ray its own pass mask, and each lane tests
// only its own pairs (exact_window_lanes below; DESIGN.md "Exact tests per
// ray").  The filter's guarantee is per (ray, triangle) pair, so this skips
// only tests the reference would reject.
//
// MfmaSpec::pair_loop (353, 354): the products' loop takes two groups per
// trip and writes each hot mask into its lane of the mask register with one
// v_writelane (sweep_kt_res).  MfmaSpec::cam_park (353, 354): the kernels that
// never load the T1 pieces keep every lane's camera end point in the wave's
// own T1 piece, written once per pixel-frame and read once per ray
// (render_mfma_k5r; rt2_path.h advance<.., PARK>).  Neither changes a value
// that reaches the image.
//
// MfmaSpec::cluster_rows (353, 354): the scene's groups come in clusters
// (rt2_cluster.h; the table lies behind the kt records), and a compact
// cluster's groups are swept only for the rays whose half line can meet its
// padded box: skipped when no live ray does, and in the one-block form, at
// half the products and half the fold, with those rays moved into one 32-row
// fragment when at most 32 do (sweep_kt_res, cluster_rows_frag).  The hot
// masks can only lose triangles no ray of the wave can hit; the episode builds
// every ray's pass mask from the unpermuted fragments as before (DESIGN.md
// "Compact clusters").
//
// MfmaSpec::cluster_rows16 (353, 354): a compact cluster that at most 16 live
// rays need is swept with 16-row products (v_mfma_f32_16x16x32_f16, 4
// accumulator registers): the rays in one fragment's lower K-half for the
// group's triangles 0..15 and in another's upper K-half for 16..31, the
// records read from the same LDS image through the lane's own pointer
// (cluster_rows_frag16; rt2_mfma.h kt_group16; DESIGN.md "16-row products").
// Every term is the sum of the same 16 f16 products as in the 32-row form (the
// other 16 k-slots add zeros), so the filter's guarantee is unchanged.
//
// MfmaSpec::cluster_rows8 (353, 354): a compact cluster that at most 8 live
// rays need is swept with one 16-row fragment that holds each ray twice, as
// [ray | 0] in rows 0..7 and as [0 | ray] in rows 8..15, so three products per
// group give both triangle halves (cluster_rows_frag8; rt2_mfma.h kt_group8;
// DESIGN.md "8-row products").  The terms are those of the 16-row form.
//
// MfmaSpec::slot_order (353, 354): the scene's triangles are regrouped by
// place at upload (rt2_cluster_order_build) and the sweep reads that slot
// image: records, table and the episode's triangles in slot order.  A ray's
// survivors are then tested in ascending slot, not index; mt_exact_slot takes
// the lower index on equal distances, which leaves the index-order scan's
// result, and the hit's slot is mapped to its index after the sweep (DESIGN.md
// "Slot order").
//
// MfmaSpec::exact_spread (353, 354): per round of the episode every lane tests
// its first pair itself, and the pairs that are left are dealt out one per
// lane through a list in the wave's second unused T1 piece and merged by a
// 64-bit minimum (exact_spread_scan, exact_window_lanes; DESIGN.md "Leftover
// pairs on all lanes").  The result is the minimum by (distance, index) over
// the same accepted pairs.
#pragma once

// v_writelane_b32 (value and lane wave-uniform).  clang has a builtin for
// readlane but none for writelane; a declaration under the intrinsic's own name
// reaches it, and the compiler places the lane select (m0 on gfx9) itself.
extern "C" __device__ int rt2_writelane(int value, int lane, int old) __asm("llvm.amdgcn.writelane.i32");

namespace {

constexpr int kResGroups = 38;  // 152 KiB of records (4 KiB per group) of the CU's 160 KiB

// LDS of the resident records: kResGroups groups x the 4 operands x 64 lanes x 16 B
struct K5Resident {
    h8 rec[kResGroups * 4 * 64];
};

// The exact phase of one group (exact_win = 1, the A/B arms' per-group form):
// the triangles with a passing pair (ballot M) in index order, mt_pass3 + mt_exact (compute.glsl:302-340, strict `dst <
// best`).  Returns whether some lane's bound improved.
template <MfmaSpec S>
__device__ __forceinline__ bool exact_group(unsigned long long M, int G, int n_tris, cfloat* tri, const f3& o,
                                            const f3& d, float& best, int& bi, float& bestK, MfmaDiag& dg) {
    if constexpr (S.diag) dg.hot += 1;
    uint32_t m32 = (uint32_t)(M | M >> 32);
    const float bk0 = bestK;
    while (m32) {
        const int tt = __builtin_ctz(m32);
        m32 &= m32 - 1;
        const int idx = 32 * G + tt;
        if (idx >= n_tris) break;
        if constexpr (S.diag) dg.exact += 1;
        cfloat* tp = tri + 12 * idx;
        const MtQ qq = mt_quantities(o, d, ldc4(tp), ldc4(tp + 4), ldc4(tp + 8));
        if (mt_pass3(qq, bestK)) mt_exact(qq, idx, best, bi, bestK);
    }
    return __ballot(bestK != bk0) != 0;
}

// diag: one episode's MfmaDiag::xl counts from each lane's pairs and its `k`
// (the wave's largest k is what a per-lane test loop would run)
__device__ __forceinline__ void xl_counts(MfmaDiag& dg, int pairs, int k, int rounds) {
    for (int off = 32; off > 0; off >>= 1) {
        pairs += __shfl_xor(pairs, off);
        k = max(k, __shfl_xor(k, off));
    }
    const unsigned long long kw = (unsigned long long)__builtin_amdgcn_readfirstlane(k);
    dg.xl[0] += (unsigned long long)__builtin_amdgcn_readfirstlane(pairs);
    dg.xl[1] += kw;
    dg.xl[2] += (unsigned long long)rounds;
    dg.xl[3] = kw > dg.xl[3] ? kw : dg.xl[3];
}

// MfmaSpec::exact_lanes.  A ray's 32-bit mask of a round: bit b is the b-th
// hot triangle of the round in ascending index, and it comes out of the
// transposed product's row xl_row_of_bit(b): lane l of the product's result
// holds ray l & 31 in all 16 registers, register r being row 8 (r >> 2) +
// 4 (l >> 5) + (r & 3); the two lanes of a ray pack their registers into bits
// 0..15 (l < 32) and 16..31.
__host__ __device__ constexpr int xl_row_of_bit(int b) { return 8 * ((b & 15) >> 2) + 4 * (b >> 4) + (b & 3); }
__host__ __device__ constexpr int xl_bit_of_row(int r) { return 16 * ((r >> 2) & 1) + 4 * (r >> 3) + (r & 3); }

// MfmaSpec::exact_spread (353, 354): a round's leftover pairs on all lanes.
// exact_window_lanes' per-lane loop runs until the wave's busiest ray is done,
// and after every lane's first pair the pairs that are left sit on a few
// lanes.  So per round: every lane tests its first pair itself; the r pairs a
// lane has left get the places at .. at + r - 1 (exclusive prefix sum over the
// wave, total Rw) of a list in LDS, an entry being (lane, bit of its mask);
// lane w < Rw tests entry w on a copy of the source ray's o, d and (best, bi)
// as they are after the first pair, the unchanged mt_quantities / mt_pass3 /
// mt_exact_slot; a worker whose copy improved publishes distance bits << 32 |
// triangle index << 16 | slot by an unsigned 64-bit minimum into the source
// lane's slot, and the source takes its slot's key.  The image cannot change
// (DESIGN.md "Leftover pairs on all lanes"): a ray's result is the minimum by
// (distance, index) over its accepted pairs; a worker's bound is looser than
// the scan's and passes every pair the scan passes; accepted distances are
// above 1e-6, so their bits order as unsigned integers; the minimum does not
// depend on the order.  A round with no lane holding two leftovers (the loop
// would end after one more trip) or with Rw > 64 takes the per-lane loop.
// Inclusive DPP scan (row_shr 1, 2, 4, 8 inside a row of 16, then row_bcast
// 15 / 31 across the rows); returns Rw, the count on the lanes below in `at`.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_add_step(int x) {
    // lanes without a source, and rows outside ROW_MASK, add `old` = 0
    return x + __builtin_amdgcn_update_dpp(0, x, CTRL, ROW_MASK, 0xf, false);
}
__device__ __forceinline__ int exact_spread_scan(int r, int& at) {
    int x = r;
    x = dpp_add_step<0x111, 0xf>(x);  // row_shr:1
    x = dpp_add_step<0x112, 0xf>(x);  // row_shr:2
    x = dpp_add_step<0x114, 0xf>(x);  // row_shr:4
    x = dpp_add_step<0x118, 0xf>(x);  // row_shr:8
    x = dpp_add_step<0x142, 0xa>(x);  // row_bcast:15 into rows 1, 3
    x = dpp_add_step<0x143, 0xc>(x);  // row_bcast:31 into rows 2, 3
    at = x - r;
    return __builtin_amdgcn_readlane(x, 63);
}

// The exact episode of one window with the tests per ray (MfmaSpec::
// exact_lanes) instead of per wave.  exact_window runs every hot triangle's
// test on all 64 lanes, though only a few rays asked for it.  Here:
//   - compaction: the window's hot triangles (maskv, the scene's last group
//     cut to n_tris) in ascending index, 32 per round, are listed in `lst`
//     (lane s = the index of the round's s-th) by a scalar walk of the masks:
//     per hot triangle a compare and a v_cndmask beside its SALU, no LDS and
//     no per-lane loop;
//   - gather: a kt record is per triangle column (lane t + 32 h of a group's
//     operand holds triangle t's k-slots 8 h .. 8 h + 7: prep_mfma_kt), so a
//     16-byte read at per-lane addresses makes a valid operand out of any 32
//     triangles.  Lane l reads the triangle of bit xl_bit_of_row(l & 31);
//     slots past the round's count read triangle 0's record and their bits
//     are cleared;
//   - transposed products: mfma(records, a0[R]) instead of mfma(a0[R],
//     records).  The A and B layouts of the 32x32x16 product are the same, so
//     the operands are the ones kt_group takes; the result's lanes are rays;
//   - pack: the same 16 ANDs as kt_group (with Y when the window has it),
//     then 16 v_alignbit (mask << 1 | sign) per block and one
//     v_permlane32_swap, after which lane l holds its own ray's 32 bits;
//   - every lane walks its own bits, lowest first: the triangle by vector
//     loads, then the unchanged mt_quantities / mt_pass3 / mt_exact.
// Rounds ascend and a lane's bits ascend, so every ray sees its surviving
// pairs in index order against its current bound: the sequential strict `dst <
// best` scan.  MfmaSpec::slot_order: maskv, recs, tri4 and the list are in
// slot order, and mt_exact_slot's tie rule keeps the scan's result.  The
// filter's guarantee is per (ray, triangle) pair (DESIGN.md "Exact tests per
// ray"), so a ray may skip what other rays of its wave test.
// upper = false: lanes 32..63 hold no ray of their own and get a zero mask.
// LDS: the records of every group of the window are resident (recs = the
// LDS copy); else recs = the scene's kt records in global memory.
template <MfmaSpec S, bool YP, bool LDS, class Rebuild>
__device__ __forceinline__ void exact_window_lanes(int maskv, int Gw, bool more, int n_tris, const float4* tri4,
                                                   const h8* a0, const h8* y1, const h8* recs, bool upper, const f3& o,
                                                   const f3& d, float& best, int& bi, float& bestK, MfmaDiag& dg,
                                                   Rebuild rebuild, [[maybe_unused]] const int* slot_tri = nullptr,
                                                   [[maybe_unused]] unsigned long long* xs_diag = nullptr,
                                                   [[maybe_unused]] int xs_wave = 0) {
    const int lane = (int)lane_id();
    // MfmaSpec::exact_spread: the wave's list (64 x 4 B) and merge slots (64 x 8 B at byte 512) in the T1 piece of
    // group 16 + wave, which nothing else reads or writes (render_mfma_k5r's static_assert)
    [[maybe_unused]] uint32_t* xs_list = nullptr;
    [[maybe_unused]] unsigned long long* xs_slot = nullptr;
    // (the kernel's one resident window, which has no Y; the other forms are never run in such a kernel)
    constexpr bool XS = S.exact_spread && LDS && !YP;
    if constexpr (XS) {
        xs_list = reinterpret_cast<uint32_t*>(const_cast<h8*>(recs) + (4 * (16 + xs_wave) + 3) * 64);
        xs_slot = reinterpret_cast<unsigned long long*>(xs_list + 128);
    }
    [[maybe_unused]] unsigned long long tc = 0;
    if constexpr (S.diag) {
        dg.claims += 1;
        tc = __builtin_amdgcn_s_memtime();
    }
    // padding slots of the scene's last group never enter the list
    if (n_tris & 31) maskv = lane == (n_tris >> 5) - Gw ? maskv & (int)((1u << (n_tris & 31)) - 1u) : maskv;
    unsigned long long hotg = __ballot(maskv != 0);
    if constexpr (S.diag) dg.hot += (unsigned long long)__popcll(hotg);
    const float bk0 = bestK;
    const int src = 4 * xl_bit_of_row(lane & 31);  // ds_bpermute address of the list entry this lane gathers
    const f16v zero = {};
    uint32_t m = 0;  // the current group's triangles still to be listed
    int gj = 0;      // ... its lane of maskv
    [[maybe_unused]] int pairs = 0, iters = 0, rounds = 0;
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
        if constexpr (S.diag) {
            dg.exact += (unsigned long long)c;
            rounds += 1;
        }
        // this lane's row of the synthetic group
        const int T = __builtin_amdgcn_ds_bpermute(src, lst);
        const h8* rp = recs + ((T >> 5) * (kKtOps * 64) + (T & 31) + (lane & 32));
        // One block's products and its 16-bit mask: kt_group's three products
        // and 16 ANDs at its peak of 48 product registers (the episode has
        // those and no more), then Y on its own where the window has it.  The
        // empty asm statements pin a stage's results in registers before the
        // next one starts: without them the compiler runs both blocks'
        // products side by side (96 registers) and spills the path state.
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
        if constexpr (S.diag) pairs += __popc(pm);
        // The lane's pairs, lowest bit first.  The mask is known up front, so
        // the next pair's triangle is requested before the current test runs
        // (a lane without a further bit reads entry 31 of the list, a valid
        // index or 0, and never uses it).
        auto entry = [&](uint32_t m) { return __builtin_amdgcn_ds_bpermute(4 * __builtin_ctz(m | 0x80000000u), lst); };
        struct Tri {
            int idx;
            float4 t0, t1, t2;
        };
        auto fetch = [&](Tri& t) {
            t.idx = entry(pm);
            t.t0 = tri4[3 * t.idx], t.t1 = tri4[3 * t.idx + 1], t.t2 = tri4[3 * t.idx + 2];
        };
        // one pair: request the next triangle into `nxt`, test `cur`
        auto step = [&](const Tri& cur, Tri& nxt) {
            if constexpr (S.diag) iters += 1;
            const bool has = pm != 0;
            pm &= pm - 1;
            fetch(nxt);
            if (has) {
                const MtQ qq = mt_quantities(o, d, cur.t0, cur.t1, cur.t2);
                if (mt_pass3(qq, bestK)) {
                    if constexpr (S.slot_order)
                        mt_exact_slot(qq, cur.idx, slot_tri, best, bi, bestK);
                    else
                        mt_exact(qq, cur.idx, best, bi, bestK);
                }
            }
        };
        Tri ta, tb2;
        fetch(ta);
        if constexpr (XS) {
            // MfmaSpec::exact_spread (the comment above exact_spread_scan): every lane's first pair on its own
            // lane, against its current bound
            {
                if constexpr (S.diag) iters += 1;
                const bool has = pm != 0;
                pm &= pm - 1;
                if (has) {
                    const MtQ qq = mt_quantities(o, d, ta.t0, ta.t1, ta.t2);
                    if (mt_pass3(qq, bestK)) {
                        if constexpr (S.slot_order)
                            mt_exact_slot(qq, ta.idx, slot_tri, best, bi, bestK);
                        else
                            mt_exact(qq, ta.idx, best, bi, bestK);
                    }
                }
            }
            // the leftovers: r per lane, `at` of them on the lanes below, Rw in the wave
            const int r = __popc(pm);
            int at;
            const int Rw = exact_spread_scan(r, at);
            if (Rw) {
                const bool spread = Rw <= 64 && __ballot(r >= 2) != 0;
                if constexpr (S.diag) {
                    xs_diag[0] += (unsigned long long)Rw;
                    xs_diag[1] += spread ? 1ull : Rw > 64 ? 1ull << 40 : 0ull;
                }
                if (spread) {
                    // scatter: entry at + j = this lane and its j-th remaining bit; the merge slot empty
                    // (the lane number from here on: an address formed outside the branch would hold a register
                    // across the products)
                    int wl = lane;
                    asm volatile("" : "+v"(wl));
                    xs_slot[wl] = ~0ull;
                    while (pm) {
                        xs_list[at++] = (uint32_t)lane | (uint32_t)__builtin_ctz(pm) << 8;
                        pm &= pm - 1;
                    }
                    asm volatile("" ::: "memory");  // the wave's LDS operations keep their order
                    // worker trip: lane w < Rw takes entry w (the other lanes entry "lane 0, bit 0", unused)
                    const bool work = lane < Rw - (S.spread_drop ? 1 : 0);
                    const uint32_t e = work ? xs_list[wl] : 0u;
                    const int from = 4 * (int)(e & 63u);
                    Tri tw;
                    tw.idx = __builtin_amdgcn_ds_bpermute(4 * (int)(e >> 8 & 31u), lst);
                    tw.t0 = tri4[3 * tw.idx], tw.t1 = tri4[3 * tw.idx + 1], tw.t2 = tri4[3 * tw.idx + 2];
                    int wtri = tw.idx;  // the pair's triangle index, the key's tie break
                    if constexpr (S.slot_order) wtri = slot_tri[tw.idx];
                    auto pull = [&](float v) {  // lane `from`'s value (ds_bpermute)
                        return __int_as_float(__builtin_amdgcn_ds_bpermute(from, __float_as_int(v)));
                    };
                    const f3 so = mk(pull(o.x), pull(o.y), pull(o.z));
                    const f3 sd = mk(pull(d.x), pull(d.y), pull(d.z));
                    float cbest = pull(best);
                    int cbi = __builtin_amdgcn_ds_bpermute(from, bi);
                    float cbestK = cbest * 1.0009765625f;  // as mt_exact sets it (and as the sweep starts it)
                    if (work) {
                        const MtQ qq = mt_quantities(so, sd, tw.t0, tw.t1, tw.t2);
                        if (mt_pass3(qq, cbestK)) {
                            if constexpr (S.slot_order)
                                mt_exact_slot(qq, tw.idx, slot_tri, cbest, cbi, cbestK);
                            else
                                mt_exact(qq, tw.idx, cbest, cbi, cbestK);
                            // improved on the source's (best, bi): publish (distance, index | slot)
                            if (cbi == tw.idx) {
                                const uint32_t lo = S.slot_order ? (uint32_t)wtri << 16 | (uint32_t)tw.idx
                                                                 : (uint32_t)tw.idx;
                                __hip_atomic_fetch_min(&xs_slot[e & 63u],
                                                       (unsigned long long)__float_as_uint(cbest) << 32 | lo,
                                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                            }
                        }
                    }
                    asm volatile("" ::: "memory");
                    // merge: every published key is below the lane's own (best, index), so is their minimum
                    const unsigned long long key = xs_slot[wl];
                    if (key != ~0ull) {
                        best = __uint_as_float((uint32_t)(key >> 32));
                        bi = (int)((uint32_t)key & (S.slot_order ? 0xffffu : ~0u));
                        bestK = best * 1.0009765625f;
                    }
                } else {
                    // too few leftovers to gain, or more than the wave has lanes: the per-lane loop
                    fetch(ta);
#pragma nounroll
                    while (__ballot(pm != 0)) {
                        step(ta, tb2);
                        if (!__ballot(pm != 0)) break;
                        step(tb2, ta);
                    }
                }
            }
        } else {
            // two steps per trip, the two triangles' registers changing roles (no copies, and no wait for the
            // requested triangle before the trip's end)
#pragma nounroll
            while (__ballot(pm != 0)) {
                step(ta, tb2);
                if (!__ballot(pm != 0)) break;
                step(tb2, ta);
            }
        }
        if (c < 32) break;
    }
    if constexpr (S.diag) xl_counts(dg, pairs, iters, rounds);
    if (more && __ballot(bestK != bk0)) {
        if constexpr (S.diag) tc = __builtin_amdgcn_s_memtime();
        rebuild();
        if constexpr (S.diag) dg.t_pub += __builtin_amdgcn_s_memtime() - tc;
    }
}

// The exact episode of one window of cnt groups from group Gw on: group Gw +
// j's hot mask is lane j of maskv (exact_win = 1: m1).  The groups in
// ascending order, each mask's triangles in ascending index, the same tests as
// exact_group; then one Y rebuild if some lane's bound improved and `more`
// groups follow.  diag: of the episode's clocks, the wait for the first survivor's
// triangle (a touch of its first word; the test's own loads then hit the
// scalar cache) goes to dg.t_issue and the rebuild to dg.t_pub.
template <MfmaSpec S, class Rebuild>
__device__ __forceinline__ void exact_window(uint32_t m1, int maskv, int Gw, int cnt, bool more, int n_tris,
                                             cfloat* tri, const f3& o, const f3& d, float& best, int& bi,
                                             float& bestK, MfmaDiag& dg, Rebuild rebuild) {
    constexpr int W = S.exact_win;
    auto mask_of = [&](int j) { return W == 1 ? m1 : (uint32_t)__builtin_amdgcn_readlane(maskv, j); };
    [[maybe_unused]] unsigned long long tc = 0;
    if constexpr (S.diag) {
        dg.claims += 1;
        tc = __builtin_amdgcn_s_memtime();
        int j = 0;
        while (!mask_of(j)) j++;  // the caller saw a non-zero mask
        const int idx = 32 * (Gw + j) + __builtin_ctz(mask_of(j));
        if (idx < n_tris) asm volatile("" ::"s"(__float_as_int(tri[12 * idx])));
        const unsigned long long t = __builtin_amdgcn_s_memtime();
        dg.t_issue += t - tc;
    }
    const float bk0 = bestK;
    // diag: this lane's pairs that pass the filter's own three conditions
    // (mt_pass3's U, -V and X terms on the exact quantities: what the products
    // decide in a window without Y), and the episode's tested triangles
    [[maybe_unused]] int pairs = 0, tested = 0;
    for (int j = 0; j < cnt; j++) {
        uint32_t m32 = mask_of(j);
        if constexpr (S.diag) dg.hot += m32 != 0;
        while (m32) {
            const int tt = __builtin_ctz(m32);
            m32 &= m32 - 1;
            const int idx = 32 * (Gw + j) + tt;
            if (idx >= n_tris) break;
            if constexpr (S.diag) dg.exact += 1;
            cfloat* tp = tri + 12 * idx;
            const MtQ qq = mt_quantities(o, d, ldc4(tp), ldc4(tp + 4), ldc4(tp + 8));
            if constexpr (S.diag) {
                const float X = __builtin_fmaf(-qq.det, 1.0009765625f, qq.V - qq.U);
                pairs += fmaxf(fmaxf(qq.U, -qq.V), X) <= qq.det * 0x1p-60f;
                tested += 1;
            }
            if (mt_pass3(qq, bestK)) mt_exact(qq, idx, best, bi, bestK);
        }
    }
    if constexpr (S.diag) xl_counts(dg, pairs, pairs, (tested + 31) >> 5);
    if (more && __ballot(bestK != bk0)) {
        if constexpr (S.diag) tc = __builtin_amdgcn_s_memtime();
        rebuild();
        if constexpr (S.diag) dg.t_pub += __builtin_amdgcn_s_memtime() - tc;
    }
}

// MfmaSpec::phase_prio: the wave's issue priority by its phase (the SIMD's
// arbiter issues by priority, then age): 1 = the products' phase high, the
// exact phase and shading low; 2 = the exact phase high; 3 = shading high;
// 4 = both VALU phases (exact phase, shading) high
template <MfmaSpec S>
__device__ __forceinline__ void phase_prio(int phase) {  // 0 products, 1 exact phase, 2 shading
    if constexpr (S.phase_prio > 0) {
        const bool hi = (S.phase_prio == 1 && phase == 0) || (S.phase_prio == 2 && phase == 1) ||
                        (S.phase_prio == 3 && phase == 2) || (S.phase_prio == 4 && phase != 0);
        if (hi)
            __builtin_amdgcn_s_setprio(1);
        else
            __builtin_amdgcn_s_setprio(0);
    }
}

// Closest hit of every lane's ray over all triangles, records from LDS: 8
// independent products per group with a zero accumulator (kt_group).  res_l2:
// groups [kResGroups, ng) are read from the scene's kt records in L2 after the
// resident ones, in the same (index) order.  Returns false (wave-uniform,
// nothing computed) when a ray is outside the filter's range.
// MfmaSpec::cluster_rows, diag: per (wave, compact cluster) of a sweep, the
// three cases and the rays that needed the cluster
struct ClusterDiag {
    unsigned long long skipped = 0, one = 0, two = 0, rays = 0;
    unsigned long long r16 = 0;  // ... of `one`, the cases at most 16 rays need (MfmaSpec::cluster_rows16's form)
};
// ... with MfmaSpec::cluster_rows8 (a type of its own: 411's and 416's code stays as it was)
struct ClusterDiag8 : ClusterDiag {
    unsigned long long r8 = 0;  // ... of `one`, the cases at most 8 rays need (MfmaSpec::cluster_rows8's form)
};

// MfmaSpec::cluster_rows.  One 32-row fragment out of a0[0] / a0[1] that holds
// the rays of `need` (at most 32 of them) in its rows 0 .. c - 1; the other
// rows hold other rays of the wave (every row of a0 is a valid ray: lanes
// without one carry a live lane's).  Each block's 32 rows are permuted as a
// whole, its needing rows to the front (block 0's to row 0, block 1's behind
// them) and the rest behind those, cyclically, so every ds_permute is a
// permutation of the 64 lanes; a row below c0 is then taken from block 0's
// result and every other one from block 1's.  Rank by mbcnt, one
// v_permlane32_swap to hand a ray's row to the two lanes that hold its
// k-slots, 8 ds_permute, 4 selects; no LDS.
__device__ __forceinline__ h8 cluster_rows_frag(const h8* a0, unsigned long long need) {
    typedef uint32_t u4 __attribute__((ext_vector_type(4)));
    const int l = (int)lane_id();
    const int c0 = __popc((uint32_t)need), c1 = __popc((uint32_t)(need >> 32));
    const int rk = (int)lanes_below(need);
    const bool nb = (need >> l) & 1ull;
    // rows of this lane's own ray: block 0 (l < 32) and block 1
    const int rest = ((l - rk) + (l < 32 ? c0 : c1 + 2 * c0)) & 31;
    const uint32_t row = (uint32_t)(nb ? rk : rest);
    // sw[0]: lanes l and l + 32 both hold the row of ray l (block 0's layout); sw[1]: of ray l + 32
    const auto sw = __builtin_amdgcn_permlane32_swap(row, row, false, false);
    const int half = l & 32;
    const int to0 = 4 * ((int)sw[0] + half), to1 = 4 * ((int)sw[1] + half);
    const u4 b0 = __builtin_bit_cast(u4, a0[0]), b1 = __builtin_bit_cast(u4, a0[1]);
    const bool first = (l & 31) < c0;
    u4 r;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int x0 = __builtin_amdgcn_ds_permute(to0, (int)b0[k]);
        const int x1 = __builtin_amdgcn_ds_permute(to1, (int)b1[k]);
        r[k] = (uint32_t)(first ? x0 : x1);
    }
    return __builtin_bit_cast(h8, r);
}

// MfmaSpec::cluster_rows16.  The two 16-row fragments of kt_group16 for the
// rays of `need` (at most 16 of them): cluster_rows_frag's ranking with other
// ds_permute destinations.  Row r < 16 of K-half h goes to lane r + 16 h, and
// row r >= 16 to lane r + 16 + 16 h of 32..63, so every permute is still a
// permutation of the 64 lanes.  alo is the result with lanes 32..63 zeroed
// ([rays | 0] over the 32 k-slots), ahi its halves exchanged ([0 | rays]).
// Rows c .. 15 hold other rays of the wave, as rows c .. 31 do there.
__device__ __forceinline__ void cluster_rows_frag16(const h8* a0, unsigned long long need, h8& alo, h8& ahi) {
    typedef uint32_t u4 __attribute__((ext_vector_type(4)));
    const int l = (int)lane_id();
    const int c0 = __popc((uint32_t)need), c1 = __popc((uint32_t)(need >> 32));
    const int rk = (int)lanes_below(need);
    const bool nb = (need >> l) & 1ull;
    const int rest = ((l - rk) + (l < 32 ? c0 : c1 + 2 * c0)) & 31;
    const uint32_t row = (uint32_t)(nb ? rk : rest);
    const uint32_t dst = row + (row & 16);
    const auto sw = __builtin_amdgcn_permlane32_swap(dst, dst, false, false);
    const int half = (l & 32) >> 1;
    const int to0 = 4 * ((int)sw[0] + half), to1 = 4 * ((int)sw[1] + half);
    const u4 b0 = __builtin_bit_cast(u4, a0[0]), b1 = __builtin_bit_cast(u4, a0[1]);
    const bool first = (l & 15) < c0, low = l < 32;
    u4 rl, rh;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int x0 = __builtin_amdgcn_ds_permute(to0, (int)b0[k]);
        const int x1 = __builtin_amdgcn_ds_permute(to1, (int)b1[k]);
        const uint32_t q = (uint32_t)(first ? x0 : x1);
        rl[k] = low ? q : 0u;
        rh[k] = __builtin_amdgcn_permlane32_swap(0u, q, false, false)[0];  // [0 | q's lanes 0..31]
    }
    alo = __builtin_bit_cast(h8, rl);
    ahi = __builtin_bit_cast(h8, rh);
}

// MfmaSpec::cluster_rows8.  kt_group8's fragment for the rays of `need` (at
// most 8 of them): cluster_rows_frag16's ranking and permutes, whose selected
// register q holds row r < 16's two k-quarters in lanes r and r + 16.  Rows
// 0..7 stay there; one v_permlane32_swap into zero and a row shift by 8 copy
// them to lanes r + 40 and r + 56; every other lane is zero:
// a8[l] = l < 32 ? ((l & 15) < 8 ? q[l] : 0) : ((l & 15) >= 8 ? q[l - 40] : 0).
// Rows c .. 7 hold other rays of the wave, as rows c .. 15 do there.  No LDS.
__device__ __forceinline__ h8 cluster_rows_frag8(const h8* a0, unsigned long long need) {
    typedef uint32_t u4 __attribute__((ext_vector_type(4)));
    const int l = (int)lane_id();
    const int c0 = __popc((uint32_t)need), c1 = __popc((uint32_t)(need >> 32));
    const int rk = (int)lanes_below(need);
    const bool nb = (need >> l) & 1ull;
    const int rest = ((l - rk) + (l < 32 ? c0 : c1 + 2 * c0)) & 31;
    const uint32_t row = (uint32_t)(nb ? rk : rest);
    const uint32_t dst = row + (row & 16);
    const auto sw = __builtin_amdgcn_permlane32_swap(dst, dst, false, false);
    const int half = (l & 32) >> 1;
    const int to0 = 4 * ((int)sw[0] + half), to1 = 4 * ((int)sw[1] + half);
    const u4 b0 = __builtin_bit_cast(u4, a0[0]), b1 = __builtin_bit_cast(u4, a0[1]);
    const bool first = (l & 15) < c0, keep = (l & 0x28) == 0;  // l < 32 and (l & 15) < 8
    u4 r;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int x0 = __builtin_amdgcn_ds_permute(to0, (int)b0[k]);
        const int x1 = __builtin_amdgcn_ds_permute(to1, (int)b1[k]);
        const uint32_t q = (uint32_t)(first ? x0 : x1);
        const uint32_t up = __builtin_amdgcn_permlane32_swap(0u, q, false, false)[0];  // [0 | q's lanes 0..31]
        // row_shr:8, out-of-row lanes 0: lanes 40..47 and 56..63 take q[0..7] and q[16..23], every other lane 0
        const uint32_t sh = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)up, 0x118, 0xf, 0xf, true);
        r[k] = keep ? q : sh;
    }
    return __builtin_bit_cast(h8, r);
}

// MfmaSpec::slot_order.  The slot image of a resident scene, one allocation
// that RenderParams::mfma_kt_frag points at: the kt records of the triangles
// in slot order, the table over the slot groups (where the index image has its
// own), the prepared triangles in slot order (3 float4 each) and slot_tri.
struct SlotImage {
    const float4* tri4;
    const int* slot_tri;
};
__device__ __forceinline__ SlotImage slot_image(const RenderParams& p) {
    const int ng = (p.n_tris + 31) >> 5;
    const char* tab = reinterpret_cast<const char*>(reinterpret_cast<const h8*>(p.mfma_kt_frag) + (size_t)ng * (kKtOps * 64));
    const float4* t4 = reinterpret_cast<const float4*>(tab + sizeof(rt2_cluster_table));
    return {t4, reinterpret_cast<const int*>(t4 + 3 * (size_t)p.n_tris)};
}

template <MfmaSpec S>
__device__ __forceinline__ bool sweep_kt_res(const RenderParams& p, const h8* rec, const f3& o, const f3& d,
                                             float& best, int& bi, float& bestK, MfmaDiag& dg, bool upper,
                                             unsigned long long act = 0, ClusterDiag* cd = nullptr,
                                             [[maybe_unused]] unsigned long long* xs_diag = nullptr,
                                             [[maybe_unused]] int xs_wave = 0) {
    const int lane = (int)lane_id();
    // MfmaSpec::diag: shader clocks of the ray setup (t_wait), the products
    // with their record reads (t_filt), the exact phase with the Y rebuilds
    // (t_exact) and the whole sweep (t_swp)
    [[maybe_unused]] unsigned long long tc = 0, tsw = 0;
    if constexpr (S.diag) tsw = tc = __builtin_amdgcn_s_memtime();
    auto stamp = [&](unsigned long long& acc) {
        if constexpr (S.diag) {
            const unsigned long long t = __builtin_amdgcn_s_memtime();
            acc += t - tc;
            tc = t;
        }
    };
    const f3 m = cross(d, o);
    MfmaScale sc;
    if (!mfma_scale<true>(p.mfma_A, o, d, m, sc)) return false;
    h8 a0[2], y1[2];
    _Float16 tw16;
    kt_frags<S.kt_lane_w>(d, m, sc, a0, tw16);
    constexpr bool per_group = S.exact_win == 1 && !S.y_skip_last && !S.diag;
    // the window path's first window needs no Y fragment (MfmaSpec::y_first)
    if constexpr (per_group || S.y_first) kt_y(d, o, bestK, sc, tw16, y1);
    stamp(dg.t_wait);
    const int ng = (p.n_tris + 31) >> 5, n_tris = p.n_tris;
    const int nres = S.res_l2 ? min(ng, kResGroups) : ng;
    cfloat* const tri = (cfloat*)p.tri;  // held across the sweep (not re-read from the kernel arguments per hot group)
    const h8* tb = rec + lane;
    [[maybe_unused]] const int* slot_tri = nullptr;
    if constexpr (S.slot_order) {
        static_assert(S.cluster_rows && S.exact_lanes && !S.res_l2, "slot_order: 353 / 354's one resident window");
        slot_tri = slot_image(p).slot_tri;
    }
    if constexpr (per_group) {
        // one exact episode per hot group, the bound rebuilt after each
        for (int G = 0; G < nres; G++) {
            const h8 b0 = tb[0], b1 = tb[64], b2 = tb[128], b3 = tb[192];
            tb += kKtOps * 64;
            const unsigned long long M = kt_group(a0, y1, b0, b1, b2, b3, upper);
            if (M) {
                phase_prio<S>(1);
                if (exact_group<S>(M, G, n_tris, tri, o, d, best, bi, bestK, dg)) kt_y(d, o, bestK, sc, tw16, y1);
                phase_prio<S>(0);
            }
        }
        if constexpr (S.res_l2) {
            const h8* gb = reinterpret_cast<const h8*>(p.mfma_kt_frag) + (size_t)nres * (kKtOps * 64) + lane;
            for (int G = nres; G < ng; G++) {
                const h8 b0 = gb[0], b1 = gb[64], b2 = gb[128], b3 = gb[192];
                gb += kKtOps * 64;
                const unsigned long long M = kt_group(a0, y1, b0, b1, b2, b3, upper);
                if (M && exact_group<S>(M, G, n_tris, tri, o, d, best, bi, bestK, dg)) kt_y(d, o, bestK, sc, tw16, y1);
            }
        }
    } else {
        constexpr int W = S.exact_win;
        static_assert(W >= 1 && W <= 64, "a window's masks are the lanes of one VGPR");
        // One window of the groups from Gw on (below G1), records at tb (LDS
        // or L2; advanced): the window's products back to back, each group's
        // hot mask kept in lane (G - window start) of maskv, then one episode.
        // yp = false_type, the sweep's first window: no ray has a bound yet,
        // so the products run without Y (kt_group<false>; the T1 record is not
        // read) and y1 does not exist.  It is built after the window when
        // groups follow, whether or not a bound improved and whether or not
        // there was an episode: the next window's Y product reads it.
        auto window = [&](auto yp, const h8*& tb, int Gw, int G1, bool resident) {
            constexpr bool YP = decltype(yp)::value;
            const int cnt = W == 1 ? 1 : min(W, G1 - Gw);
            int maskv = 0;
            uint32_t any = 0;
            if constexpr (S.pair_loop && W > 1) {
                // MfmaSpec::pair_loop.  Two groups per trip: the second one's
                // records sit a constant 4 KiB behind the first's, so its
                // ds_read_b128 take immediate offsets and the pointer steps
                // once per pair.  The ballot's mask and the group's number are
                // wave-uniform, so one v_writelane puts the mask into lane j
                // (the loop below pays a v_mov, a compare and a select).
                // kt_group keeps its own basic blocks and scheduling groups.
                auto group = [&](const h8* t, int j, bool up) {
                    const h8 b0 = t[0], b1 = t[64], b2 = t[128];
                    h8 b3 = {};
                    if constexpr (YP) b3 = t[192];
                    const unsigned long long M = kt_group<YP>(a0, y1, b0, b1, b2, b3, up);
                    const uint32_t m32 = (uint32_t)(M | M >> 32);
                    maskv = rt2_writelane((int)m32, j, maskv);
                    any |= m32;
                };
                // groups [j, j1) in the two-block form, two per trip
                auto two_block = [&](int j, int j1, bool up) {
                    for (; j + 1 < j1; j += 2) {
                        group(tb, j, up);
                        group(tb + kKtOps * 64, j + 1, up);
                        tb += 2 * kKtOps * 64;
                    }
                    if (j < j1) {
                        group(tb, j, up);
                        tb += kKtOps * 64;
                    }
                };
                bool clustered = false;
                [[maybe_unused]] cfloat* ct = nullptr;  // the scene's rt2_cluster_table, behind the records
                // (a window with Y is instantiated but never run in these kernels)
                if constexpr (S.cluster_rows && !YP) {
                    static_assert(!S.res_l2 && W >= kResGroups && !S.y_first,
                                  "cluster_rows: one window of every group, no distance bound in it");
                    ct = (cfloat*)(reinterpret_cast<const h8*>(p.mfma_kt_frag) + (size_t)ng * (kKtOps * 64));
                    clustered = __float_as_int(ct[1]) != 0;
                }
                if (!clustered) two_block(0, cnt, upper);
                if constexpr (S.cluster_rows && !YP) {
                    if (clustered) {
                        // MfmaSpec::cluster_rows (DESIGN.md "Compact clusters").
                        // The need test, once per sweep: for every compact
                        // cluster the live rays (act) whose half line can meet
                        // its padded box (rt2_cluster.h; the bounds by scalar
                        // loads), parked in lanes kNeedLane + 2 k and + 1 of
                        // maskv, which the at most kResGroups hot masks leave
                        // free (no VGPR added; cleared again before the
                        // episode); the reciprocals die with this block.
                        const int ncl = __float_as_int(ct[1]);
                        const float far_o = ct[0];
                        ct += 8;  // the entries
                        constexpr int kNeedLane = 64 - 2 * RT2_MAX_CLUSTERS;
                        static_assert(kNeedLane >= kResGroups, "the need masks share maskv with the hot masks");
                        {
                            const float of[3] = {o.x, o.y, o.z}, df[3] = {d.x, d.y, d.z};
                            float inv[3];
                            rt2_cluster_inv(df, inv);
                            const bool always = rt2_cluster_always(of, df, far_o);
#pragma nounroll
                            for (int k = 0; k < ncl; k++) {
                                const float4 c0 = ldc4(ct + 8 * k), c1 = ldc4(ct + 8 * k + 4);
                                unsigned long long nm = act;
                                if (__float_as_int(c1.w) & RT2_CLUSTER_COMPACT) {
                                    const float lo[3] = {c0.x, c0.y, c0.z}, hi[3] = {c1.x, c1.y, c1.z};
                                    nm &= __ballot(always || rt2_cluster_need_box(lo, hi, of, inv));
                                }
                                maskv = rt2_writelane((int)(uint32_t)nm, kNeedLane + 2 * k, maskv);
                                maskv = rt2_writelane((int)(uint32_t)(nm >> 32), kNeedLane + 2 * k + 1, maskv);
                            }
                        }
                        // groups [j, j1) in the one-block form with fragment af, two per trip
                        auto one_block = [&](const h8& af, int j, int j1) {
                            for (; j + 1 < j1; j += 2) {
                                const h8* t = tb;
                                unsigned long long M0, M1;
                                kt_group_one2(af, t[0], t[64], t[128], t[kKtOps * 64], t[kKtOps * 64 + 64],
                                              t[kKtOps * 64 + 128], M0, M1);
                                const uint32_t m0 = (uint32_t)(M0 | M0 >> 32), m1 = (uint32_t)(M1 | M1 >> 32);
                                maskv = rt2_writelane((int)m0, j, maskv);
                                maskv = rt2_writelane((int)m1, j + 1, maskv);
                                any |= m0 | m1;
                                tb += 2 * kKtOps * 64;
                            }
                            if (j < j1) {
                                const h8 b0 = tb[0], b1 = tb[64], b2 = tb[128], b3 = {};
                                const unsigned long long M = kt_group<false>(&af, y1, b0, b1, b2, b3, false);
                                const uint32_t m32 = (uint32_t)(M | M >> 32);
                                maskv = rt2_writelane((int)m32, j, maskv);
                                any |= m32;
                                tb += kKtOps * 64;
                            }
                        };
                        // MfmaSpec::cluster_rows16: groups [j, j1) in the 16-row form with fragments
                        // alo / ahi, two per trip; the lane's own pointer into the same records
                        // (kt16_record_lane: one ds_read_b128 per quantity, as above)
                        [[maybe_unused]] auto one_block16 = [&](const h8& alo, const h8& ahi, int j, int j1) {
                            const int d16 = kt16_record_lane(lane) - lane;
                            const h8* t = tb + d16;
                            for (; j + 1 < j1; j += 2) {
                                uint32_t m0, m1;
                                kt_group16_2(alo, ahi, t[0], t[64], t[128], t[kKtOps * 64], t[kKtOps * 64 + 64],
                                             t[kKtOps * 64 + 128], m0, m1);
                                maskv = rt2_writelane((int)m0, j, maskv);
                                maskv = rt2_writelane((int)m1, j + 1, maskv);
                                any |= m0 | m1;
                                t += 2 * kKtOps * 64;
                            }
                            if (j < j1) {
                                const uint32_t m32 = kt_group16(alo, ahi, t[0], t[64], t[128]);
                                maskv = rt2_writelane((int)m32, j, maskv);
                                any |= m32;
                                t += kKtOps * 64;
                            }
                            tb = t - d16;
                        };
                        // MfmaSpec::cluster_rows8: groups [j, j1) in the 8-row form with fragment a8, two per
                        // trip; the records as in the 16-row form
                        [[maybe_unused]] auto one_block8 = [&](const h8& a8, int j, int j1) {
                            const int d16 = kt16_record_lane(lane) - lane;
                            const h8* t = tb + d16;
                            for (; j + 1 < j1; j += 2) {
                                uint32_t m0, m1;
                                kt_group8_2(a8, t[0], t[64], t[128], t[kKtOps * 64], t[kKtOps * 64 + 64],
                                            t[kKtOps * 64 + 128], m0, m1);
                                maskv = rt2_writelane((int)m0, j, maskv);
                                maskv = rt2_writelane((int)m1, j + 1, maskv);
                                any |= m0 | m1;
                                t += 2 * kKtOps * 64;
                            }
                            if (j < j1) {
                                const uint32_t m32 = kt_group8(a8, t[0], t[64], t[128]);
                                maskv = rt2_writelane((int)m32, j, maskv);
                                any |= m32;
                                t += kKtOps * 64;
                            }
                            tb = t - d16;
                        };
#pragma nounroll
                        for (int k = 0; k < ncl; k++) {
                            const int g0 = __float_as_int(ct[8 * k + 3]), gf = __float_as_int(ct[8 * k + 7]);
                            const int g1 = gf & 0xffff;
                            const unsigned long long need =
                                (unsigned long long)(uint32_t)__builtin_amdgcn_readlane(maskv, kNeedLane + 2 * k) |
                                (unsigned long long)(uint32_t)__builtin_amdgcn_readlane(maskv, kNeedLane + 2 * k + 1) << 32;
                            const int c = __popcll(need);
                            const bool compact = (gf & RT2_CLUSTER_COMPACT) != 0;
                            if constexpr (S.diag)
                                if (compact) {
                                    cd->rays += (unsigned long long)c;
                                    if (!c)
                                        cd->skipped += 1;
                                    else if (!upper || c <= 32)
                                        cd->one += 1;
                                    else
                                        cd->two += 1;
                                    if (c && c <= 16) cd->r16 += 1;
                                    if constexpr (S.cluster_rows8)
                                        if (c && c <= 8) static_cast<ClusterDiag8*>(cd)->r8 += 1;
                                }
                            if (!c) {  // no live ray can meet the box: the groups' hot masks stay 0
                                tb += (g1 - g0) * (kKtOps * 64);
                                continue;
                            }
                            if constexpr (S.cluster_rows8) {
                                static_assert(S.cluster_rows16, "cluster_rows8: the 16-row form takes 9 to 16 rays");
                                if (compact && c <= 8) {  // whether or not `upper`, as below
                                    one_block8(cluster_rows_frag8(a0, need), g0, g1);
                                    continue;
                                }
                            }
                            if constexpr (S.cluster_rows16)
                                if (compact && c <= 16) {
                                    // whether or not the wave has rays in block 1 (`upper`): the ranking is the
                                    // same text, and 12 vector instructions fewer per group outweigh the
                                    // fragment's 40 from a cluster's fourth group on (config B's have 7 and 11)
                                    h8 alo, ahi;
                                    cluster_rows_frag16(a0, need, alo, ahi);
                                    one_block16(alo, ahi, g0, g1);
                                    continue;
                                }
                            if (upper && !(compact && c <= 32)) {
                                // `upper` is true here, but kt_group is to keep the branch on it: folded
                                // away, a group's products and its fold share a basic block with their
                                // neighbours, the scheduling groups no longer hold and the products take 96
                                // registers instead of 48
                                int up = 1;
                                asm volatile("" : "+s"(up));
                                two_block(g0, g1, up != 0);
                            } else {
                                // a wave of at most 32 live rays has them in block 0 already
                                h8 af = a0[0];
                                if (upper) af = cluster_rows_frag(a0, need);
                                one_block(af, g0, g1);
                            }
                        }
                        maskv = lane < kNeedLane ? maskv : 0;  // the episode reads every lane as a hot mask
                    }
                }
            } else {
                for (int j = 0; j < cnt; j++) {
                    const h8 b0 = tb[0], b1 = tb[64], b2 = tb[128];
                    h8 b3 = {};
                    if constexpr (YP) b3 = tb[192];
                    tb += kKtOps * 64;
                    const unsigned long long M = kt_group<YP>(a0, y1, b0, b1, b2, b3, upper);
                    const uint32_t m32 = (uint32_t)(M | M >> 32);
                    if constexpr (W > 1) maskv = lane == j ? (int)m32 : maskv;
                    any |= m32;
                }
            }
            if constexpr (S.diag) dg.groups += (unsigned long long)cnt;
            if (resident) stamp(dg.t_filt);
            if (any) {
                const bool more = YP && (Gw + cnt < ng || (W == 1 && !S.y_skip_last));
                if (resident) phase_prio<S>(1);
                if constexpr (S.exact_lanes) {
                    static_assert(W > 1, "exact_lanes reads the window's masks from maskv");
                    const float4* tri4 = reinterpret_cast<const float4*>(p.tri);
                    if constexpr (S.slot_order) tri4 = slot_image(p).tri4;
                    auto rebuild = [&] { kt_y(d, o, bestK, sc, tw16, y1); };
                    // a first window is resident; the L2 loop's windows gather from the scene's records
                    if (!YP || resident)
                        exact_window_lanes<S, YP, true>(maskv, Gw, more, n_tris, tri4, a0, y1, rec, upper, o, d, best,
                                                        bi, bestK, dg, rebuild, slot_tri, xs_diag, xs_wave);
                    else if constexpr (YP)
                        exact_window_lanes<S, YP, false>(maskv, Gw, more, n_tris, tri4, a0, y1,
                                                         reinterpret_cast<const h8*>(p.mfma_kt_frag), upper, o, d, best,
                                                         bi, bestK, dg, rebuild);
                } else {
                    exact_window<S>(any, maskv, Gw, cnt, more, n_tris, tri, o, d, best, bi, bestK, dg,
                                    [&] { kt_y(d, o, bestK, sc, tw16, y1); });
                }
                if (resident) phase_prio<S>(0);
            }
            // a window of kResGroups is the whole sweep of a kernel without the L2 loop
            if constexpr (!YP && (S.res_l2 || W < kResGroups))
                if (Gw + cnt < ng) {
                    [[maybe_unused]] unsigned long long ty = 0;
                    if constexpr (S.diag) ty = __builtin_amdgcn_s_memtime();
                    kt_y(d, o, bestK, sc, tw16, y1);
                    if constexpr (S.diag) dg.t_pub += __builtin_amdgcn_s_memtime() - ty;
                }
            if (resident) stamp(dg.t_exact);
        };
        // The windows over the groups [G0, G1); yfirst = false_type: the first
        // one, peeled, takes the form without Y.
        auto windows = [&](auto yfirst, const h8* tb, int G0, int G1, bool resident) {
            constexpr bool YF = decltype(yfirst)::value;
            int Gw = G0;
            if constexpr (!YF) {
                if (Gw < G1) window(std::false_type{}, tb, Gw, G1, resident);
                Gw += W;
            }
            // ... and a window of kResGroups is the whole resident stretch
            if constexpr (YF || W < kResGroups)
                for (; Gw < G1; Gw += W) window(std::true_type{}, tb, Gw, G1, resident);
        };
        windows(std::bool_constant<S.y_first>{}, tb, 0, nres, true);
        if constexpr (S.res_l2)
            windows(std::true_type{}, reinterpret_cast<const h8*>(p.mfma_kt_frag) + (size_t)nres * (kKtOps * 64) + lane,
                    nres, ng, false);
    }
    // MfmaSpec::slot_order: the hit's slot becomes its triangle's index, once per sweep
    if constexpr (S.slot_order)
        if (bi >= 0) bi = slot_tri[bi];
    if constexpr (S.diag) dg.t_swp += __builtin_amdgcn_s_memtime() - tsw;
    return true;
}

// The resident frame's preamble for trace_rays_k5r (rt2_query.h): every
// resident group's 4 operands by LDS-DMA (1-KiB pieces, coalesced 16 B per
// lane, no VGPRs), dealt round-robin over the workgroup's waves; then one
// barrier: every wave's pieces have landed.  render_mfma_k5r below keeps the
// same text inline: calling this function there gives the render kernels
// other register assignments and another schedule of the preamble than the
// code DESIGN.md's measurements are of.
template <MfmaSpec S>
__device__ __forceinline__ void res_load_records(K5Resident& rs) {
    constexpr int NW = S.block / 64;
    const RenderParams& p = kargs<RenderParams>();
    const int ng = min((p.n_tris + 31) >> 5, kResGroups);
    const int lane = (int)lane_id(), wave = (int)(threadIdx.x >> 6);
    // The T1 records (every fourth piece) are read by the Y product only,
    // which the resident groups never see when they are all one first
    // window and nothing follows it: those pieces stay away (their LDS is
    // never read; the layout is unchanged).
    constexpr bool no_t1 = !S.y_first && S.exact_win >= kResGroups && !S.res_l2;
    for (int i = wave; i < (no_t1 ? 3 : 4) * ng; i += NW) {
        const int pc = no_t1 ? i + i / 3 : i;  // 4 G + op of U, -V, X's i = 3 G + op
        const h8* src = reinterpret_cast<const h8*>(p.mfma_kt_frag) + (size_t)pc * 64 + lane;  // [G][4 ops] contiguous
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)&rs.rec[pc * 64], 16, 0, 0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
}

// render_mfma's segment loop with free-running waves (no barrier after the
// records have landed) around sweep_kt_res; the path state stays in
// registers.  The launcher takes it only for scenes of at most kResGroups
// groups (res_l2: at most 256).
template <MfmaSpec S>
__global__ __launch_bounds__(S.block) __attribute__((amdgpu_waves_per_eu(S.waves))) void render_mfma_k5r(RenderParams p_arg) {
    constexpr int NW = S.block / 64;
    __shared__ K5Resident rs;
    {
        // every resident group's 4 operands by LDS-DMA (1-KiB pieces, coalesced
        // 16 B per lane, no VGPRs), dealt round-robin over the waves; then one
        // barrier: every wave's pieces have landed
        const RenderParams& p = kargs<RenderParams>();
        const int ng = min((p.n_tris + 31) >> 5, kResGroups);
        const int lane = (int)lane_id(), wave = (int)(threadIdx.x >> 6);
        // The T1 records (every fourth piece) are read by the Y product only,
        // which the resident groups never see when they are all one first
        // window and nothing follows it: those pieces stay away (their LDS is
        // never read; the layout is unchanged).
        constexpr bool no_t1 = !S.y_first && S.exact_win >= kResGroups && !S.res_l2;
        for (int i = wave; i < (no_t1 ? 3 : 4) * ng; i += NW) {
            const int pc = no_t1 ? i + i / 3 : i;  // 4 G + op of U, -V, X's i = 3 G + op
            const h8* src = reinterpret_cast<const h8*>(p.mfma_kt_frag) + (size_t)pc * 64 + lane;  // [G][4 ops] contiguous
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                             (__attribute__((address_space(3))) void*)&rs.rec[pc * 64], 16, 0, 0);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    Lane L;
    lane_init(L);
    MfmaDiag dg;
    struct NoClusterDiag {};
    [[maybe_unused]] std::conditional_t<S.cluster_rows8, ClusterDiag8,
                                        std::conditional_t<S.cluster_rows, ClusterDiag, NoClusterDiag>> cdg;
    [[maybe_unused]] PathDiagSlot<S.diag> pds;
    // MfmaSpec::exact_spread, diag: [0] the rounds' leftover pairs (Rw) summed, [1] rounds that took the spread
    // path, + 2^40 per round that fell back because Rw > 64
    struct SpreadDiag {
        unsigned long long n[2] = {};
    };
    [[maybe_unused]] std::conditional_t<S.exact_spread && S.diag, SpreadDiag, NoClusterDiag> xsd;
    if constexpr (S.exact_spread) {
        // exact_window_lanes keeps wave w's list and merge slots in the T1 piece of group 16 + w: behind cam_park's
        // pieces (groups 0 .. NW - 1), never loaded, no LDS added, no other wave touches it, no barrier
        constexpr bool no_t1 = !S.y_first && S.exact_win >= kResGroups && !S.res_l2;
        static_assert(no_t1 && NW <= 16 && 2 * NW <= kResGroups && S.exact_lanes,
                      "exact_spread works in T1 pieces that nothing else uses");
    }
    const int wave = (int)(threadIdx.x >> 6);
    [[maybe_unused]] int xs_wave = 0;  // MfmaSpec::exact_spread: the wave's number in a scalar register
    if constexpr (S.exact_spread) xs_wave = __builtin_amdgcn_readfirstlane(wave);
    // MfmaSpec::lean: the wave counts its lanes' segments (no per-lane counter)
    [[maybe_unused]] unsigned long long segs_w = 0;
    // diag wave timeline (p.wave_log, 10 words per wave: start, first lane out
    // of items, end (s_memrealtime, 100 MHz), segment rounds with two 32-ray
    // blocks / one / - / cooperative drain, HW_ID | XCC_ID << 32, shader clocks
    // (s_memtime) at start and end)
    [[maybe_unused]] unsigned long long wl_t0 = 0, wl_c0 = 0, wl_dry = 0, wl_r2 = 0, wl_r1 = 0, wl_coop = 0;
    if constexpr (S.diag) {
        wl_t0 = __builtin_amdgcn_s_memrealtime();
        wl_c0 = __builtin_amdgcn_s_memtime();
    }
    for (;;) {
        const RenderParams& p = kargs<RenderParams>();
        if constexpr (S.cam_park) {
            // MfmaSpec::cam_park.  This kernel never loads the T1 pieces
            // (no_t1 above; piece 4 G + 3 of group G) and K5Resident holds
            // kResGroups >= NW groups whatever the scene's size, so wave w
            // keeps its lanes' end points in the T1 piece of group w: no LDS
            // added, no other wave reads or writes it, no barrier.
            constexpr bool no_t1 = !S.y_first && S.exact_win >= kResGroups && !S.res_l2;
            static_assert(no_t1 && S.lean && NW <= kResGroups, "cam_park parks in T1 pieces that nothing else uses");
            float4* park = reinterpret_cast<float4*>(&rs.rec[(4 * wave + 3) * 64 + (int)lane_id()]);
            if constexpr (S.diag)
                advance<1, false, true, true, S.linear>(L, p, park, pds.get());
            else
                advance<1, false, true, false, S.linear>(L, p, park);
        } else if constexpr (S.diag) {
            advance<1, !S.lean, false, true, S.linear>(L, p, nullptr, pds.get());
        } else {
            advance<1, !S.lean, false, false, S.linear>(L, p);
        }
        unsigned long long act = __ballot(L.st == ST_TRACE);
        if constexpr (S.lean) segs_w += (unsigned long long)__popcll(act);
        if constexpr (S.diag) {
            if (!wl_dry && __any(L.st == ST_DONE)) wl_dry = __builtin_amdgcn_s_memrealtime();
            if (act) {
                if (__popcll(act) <= (unsigned)S.tail_lanes && __any(L.st == ST_DONE))
                    wl_coop++;
                else if (__popcll(act) <= 32)
                    wl_r1++;
                else
                    wl_r2++;
            }
        }
        if (!act) break;  // every lane is done and the pool is dry
        if (__popcll(act) <= (unsigned)S.tail_lanes && __any(L.st == ST_DONE)) {
            float mybest = 1e38f;
            int mybi = -1;
            coop_each(act, L.o, L.d, p, mybest, mybi);
            if (L.st == ST_TRACE) {
                L.bounce += 1;
                if constexpr (!S.lean) L.segs += 1;
                if constexpr (S.diag)
                    shade<1, true, S.linear>(L, p, mybest, mybi, pds.get());
                else
                    shade<1, false, S.linear>(L, p, mybest, mybi);
            }
            continue;
        }
        if constexpr (S.fair_prio) {
            // MfmaSpec::fair_prio.  A SIMD's four waves start together, and
            // in a rank slab each lane holds about one item (a pixel's 64
            // rays, one after another): the SIMD is done when its slowest
            // wave is.  The arbiter issues by priority, then age, so with
            // equal priorities the oldest wave runs ahead and the youngest
            // ends alone, latency-bound, for ~3 ms of a 25-ms 1/8 slab.  Here
            // a wave's priority rises with the rays its slowest lane has left
            // (quartiles of the rays per pixel): waves that fall behind take
            // the issue slots back, and the SIMD's waves end together.
            const float left = wave_max((float)(L.st == ST_TRACE ? p.R - L.ray : 0));
            const int q = (int)(left * 4.0f - 1.0f) / p.R;
            if (q >= 3)
                __builtin_amdgcn_s_setprio(3);
            else if (q == 2)
                __builtin_amdgcn_s_setprio(2);
            else if (q == 1)
                __builtin_amdgcn_s_setprio(1);
            else
                __builtin_amdgcn_s_setprio(0);
        }
        // at most 32 live rays: move them to lanes 0..31 and sweep the first
        // 32-ray block only
        bool upper = true;
        if (__popcll(act) <= 32) {
            if (act >> 32) {
                const uint32_t l = lane_id(), nl = (uint32_t)__popcll(act);
                const bool live = (act >> l) & 1ull;
                const int to = 4 * (int)(live ? lanes_below(act) : nl + lanes_below(~act));
                lane_permute<!S.lean, !S.lean>(L, to);
                if constexpr (S.cam_park) {  // the parked end point travels with its path state
                    float4* park = reinterpret_cast<float4*>(&rs.rec[(4 * wave + 3) * 64 + (int)lane_id()]);
                    const float4 e = *park;
                    *park = make_float4(perm_f(to, e.x), perm_f(to, e.y), perm_f(to, e.z), 0.0f);
                }
                act = __ballot(L.st == ST_TRACE);
            }
            upper = false;
        }
        // lanes without a ray carry the first live lane's (ST_DONE lanes never
        // read their o, d again)
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
        phase_prio<S>(0);
        bool swept;
        if constexpr (S.exact_spread && S.diag)
            swept = sweep_kt_res<S>(p, rs.rec, ro, rd, best, bi, bestK, dg, upper, act, &cdg, xsd.n, xs_wave);
        else if constexpr (S.exact_spread)
            swept = sweep_kt_res<S>(p, rs.rec, ro, rd, best, bi, bestK, dg, upper, act, &cdg, nullptr, xs_wave);
        else if constexpr (S.cluster_rows)
            swept = sweep_kt_res<S>(p, rs.rec, ro, rd, best, bi, bestK, dg, upper, act, &cdg);
        else
            swept = sweep_kt_res<S>(p, rs.rec, ro, rd, best, bi, bestK, dg, upper);
        // a ray outside the filter's range (wave-uniform): the drain's code
        if (!swept) coop_each(act, ro, rd, p, best, bi);
        phase_prio<S>(2);
        if (mine) {
            L.bounce += 1;
            if constexpr (!S.lean) L.segs += 1;
            if constexpr (S.diag)
                shade<1, true, S.linear>(L, p, best, bi, pds.get());
            else
                shade<1, false, S.linear>(L, p, best, bi);
        }
    }
    const RenderParams& p = kargs<RenderParams>();
    if constexpr (S.lean) {
        if (lane_id() == 0) atomicAdd(p.seg_counter, segs_w);
    } else {
        flush_counters(L, p);
    }
    if constexpr (S.diag)
        if (p.wave_log) {
            const uint32_t gw = blockIdx.x * NW + (uint32_t)wave;
            const unsigned long long c1 = __builtin_amdgcn_s_memtime();
            const unsigned long long hw = (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4) |
                                          (unsigned long long)__builtin_amdgcn_s_getreg((15 << 11) | 20) << 32;
            if (lane_id() == 0 && gw < p.wave_log_n) {
                unsigned long long* e = p.wave_log + 10 * (size_t)gw;
                e[0] = wl_t0;
                e[1] = wl_dry;
                e[2] = __builtin_amdgcn_s_memrealtime();
                e[3] = wl_r2;
                e[4] = wl_r1;
                e[5] = 0;
                e[6] = wl_coop;
                e[7] = hw;
                e[8] = wl_c0;
                e[9] = c1;
            }
        }
    if constexpr (S.diag) {  // PathDiag: rnd_dir calls and loop trips of the wave (the lanes' counts summed)
        unsigned long long calls = pds.d.rd_calls, trips = pds.d.rd_trips;
        for (int off = 32; off > 0; off >>= 1) {
            calls += __shfl_xor(calls, off);
            trips += __shfl_xor(trips, off);
        }
        if (lane_id() == 0) {
            atomicAdd(p.seg_counter + 20, calls);
            atomicAdd(p.seg_counter + 21, trips);
        }
    }
    if constexpr (S.diag)
        if (lane_id() == 0) {
            atomicAdd(p.seg_counter + 1, dg.groups);  // (wave, triangle group) sweeps
            atomicAdd(p.seg_counter + 2, dg.hot);     // ... with a passing pair
            atomicAdd(p.seg_counter + 3, dg.exact);   // ... (wave, triangle) exact tests
            atomicAdd(p.seg_counter + 12, dg.t_wait);  // shader clocks: the sweep's ray setup
            atomicAdd(p.seg_counter + 13, dg.t_filt);  // ... products + record reads
            atomicAdd(p.seg_counter + 14, dg.t_exact); // ... exact phase + Y rebuilds
            atomicAdd(p.seg_counter + 15, dg.t_swp);   // ... whole sweeps
            atomicAdd(p.seg_counter + 16, __builtin_amdgcn_s_memtime() - wl_c0);  // ... the wave's life
            atomicAdd(p.seg_counter + 17, dg.t_issue);  // ... of the exact phase: waiting for an episode's first triangle
            atomicAdd(p.seg_counter + 18, dg.t_pub);    // ... of the exact phase: the Y rebuilds
            atomicAdd(p.seg_counter + 19, dg.claims);   // exact episodes
            atomicAdd(p.seg_counter + 7, dg.xl[0]);     // per episode (MfmaDiag::xl): (ray, triangle) pairs
            atomicAdd(p.seg_counter + 8, dg.xl[1]);     // ... the largest count of one ray
            atomicAdd(p.seg_counter + 9, dg.xl[2]);     // ... rounds of 32 hot triangles
            atomicMax(p.seg_counter + 10, dg.xl[3]);    // the largest count of one ray in any episode
            atomicAdd(p.seg_counter + 22, pds.d.new_ray);  // PathDiag: advance's new-ray block, executions
            atomicAdd(p.seg_counter + 23, pds.d.new_px);   // ... its new-frame block
            if constexpr (S.cluster_rows) {  // ClusterDiag: (wave, compact cluster) cases of the sweeps
                atomicAdd(p.seg_counter + 24, cdg.skipped);  // ... no ray needs it
                atomicAdd(p.seg_counter + 25, cdg.one);      // ... swept in the one-block form
                atomicAdd(p.seg_counter + 26, cdg.two);      // ... more than 32 rays need it: two blocks
                atomicAdd(p.seg_counter + 27, cdg.rays);     // ... the rays that need it, summed
                atomicAdd(p.seg_counter + 28, cdg.r16);      // ... at most 16 rays need it (and at least one)
                // (slot 29 is the scene's scratch word for the record preparation's flags)
                if constexpr (S.cluster_rows8) atomicAdd(p.seg_counter + 30, cdg.r8);  // ... at most 8 (and at least one)
            }
            if constexpr (S.exact_spread) {  // SpreadDiag: per round of an episode
                atomicAdd(p.seg_counter + 4, xsd.n[0]);   // ... the pairs left after every lane's first (Rw), summed
                // (two counts in one word: 4 and 11 are this kernel's only free slots; 5 and 6 are preset per render,
                // 29 and 30 taken)
                atomicAdd(p.seg_counter + 11, xsd.n[1]);  // ... spread rounds, + 2^40 per fallback with Rw > 64
            }
        }
}

}  // namespace
