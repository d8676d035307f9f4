// The cluster table of the resident matrix-filter kernel (include/rt2_cluster.h;
// DESIGN.md "Compact clusters"): the scene's 32-triangle groups, in index order,
// cut into at most RT2_MAX_CLUSTERS contiguous ranges, each either full (swept
// by all the wave's rays, as before) or compact (swept by the rays whose
// segment can meet its padded box).  The rule reads the triangles only.
// rt2_cluster_order_build also chooses which triangles share a group and in
// which order the groups are swept (DESIGN.md "Slot order").
#include <algorithm>
#include <array>
#include <cmath>
#include <cstring>
#include <numeric>
#include <vector>

#include "../../../include/rt2_cluster.h"
#include "host_internal.h"

namespace {

struct Box {
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    void add(const rt2_vec4& p) {
        const double v[3] = {p.x, p.y, p.z};
        for (int k = 0; k < 3; k++) {
            lo[k] = std::min(lo[k], v[k]);
            hi[k] = std::max(hi[k], v[k]);
        }
    }
    void add(const Box& b) {
        for (int k = 0; k < 3; k++) {
            lo[k] = std::min(lo[k], b.lo[k]);
            hi[k] = std::max(hi[k], b.hi[k]);
        }
    }
    double area() const {
        const double x = hi[0] - lo[0], y = hi[1] - lo[1], z = hi[2] - lo[2];
        return 2.0 * (x * y + y * z + z * x);
    }
};

// The instruction counts the rule weighs (vector instructions per wave and
// sweep; DESIGN.md "Compact clusters" has where each comes from).
constexpr double kFullGroup = 50.5;  // a group in the two-block form
constexpr double kOneGroup = 26.5;   // ... in the one-block form
constexpr double kNeedTest = 23.0;   // a compact cluster's need test
constexpr double kCompact = 20.0;    // the row compaction
constexpr double kPerCluster = 4.0;  // loop overhead of any cluster

// Expected cost of groups [i, j) as a compact cluster whose box has the share
// r of the scene box's surface area.  For lines that cross a convex body, the
// share that also crosses a convex body inside it is the ratio of the surface
// areas, so r bounds the share of a wave's rays that need the cluster; the
// wave stays in the one-block form while at most half of them do, which the
// rule takes as certain up to r = 1/4 and as lost at r = 1/2.
double compact_cost(int n, double r) {
    const double q = std::min(1.0, std::max(0.0, (r - 0.25) / 0.25));
    return kNeedTest + kCompact + n * (kOneGroup + (kFullGroup - kOneGroup) * q);
}

// The prices of the slot-order rule (DESIGN.md "Slot order": the listings of
// "Compact clusters", "16-row products" and "8-row products"), per wave and
// sweep.  A compact cluster of n groups pays its need test and loop share,
// then by the number c of rays that need it: nothing (c = 0), the 8-row
// products (c <= 8) and the 16-row products (c <= 16) where they are cheaper,
// the one-block form (c <= 32), the two-block form.
constexpr double kSlotCompact = 31.0, kSlotFull = 8.0, kSlotGroup = 51.5;
double price32(int n) { return 28.0 + 53.0 * (n / 2) + 27.0 * (n % 2); }
double price16(int n) { return std::min(38.0 + 31.0 * (n / 2) + 16.0 * (n % 2), price32(n)); }
double price8(int n) { return std::min(45.0 + 17.0 * (n / 2) + 9.0 * (n % 2), price16(n)); }
// c is taken as binomial over a wave's 64 rays that each need the cluster
// with probability r, the area share of compact_cost above.  Dead lanes only
// lower c, which makes a compact cluster cheaper and never dearer.
constexpr int kSlotRays = 64;
double slot_compact_cost(int n, double r) {
    r = std::min(1.0, std::max(0.0, r));
    if (r >= 1.0) return kSlotCompact + kSlotGroup * n;
    double pm = std::pow(1.0 - r, kSlotRays), e = 0.0;  // pm = P(c = 0): the skip term
    for (int c = 1; c <= kSlotRays; c++) {
        pm *= (double)(kSlotRays - c + 1) / c * (r / (1.0 - r));
        e += pm * (c <= 8 ? price8(n) : c <= 16 ? price16(n) : c <= 32 ? price32(n) : kSlotGroup * n);
    }
    return kSlotCompact + e;
}
double slot_full_cost(int n) { return kSlotFull + kSlotGroup * n; }

struct Groups {
    std::vector<Box> gb;
    Box scene;
    double m_abs = 0.0;
    bool finite = true;
};
Groups group_boxes(const rt2_triangle* tris, int32_t n_tris) {
    Groups g;
    g.gb.resize((n_tris + 31) / 32);
    for (int i = 0; i < n_tris; i++)
        for (const rt2_vec4* p : {&tris[i].a, &tris[i].b, &tris[i].c}) {
            g.gb[i >> 5].add(*p);
            for (float v : {p->x, p->y, p->z}) {
                g.finite = g.finite && std::isfinite(v);
                g.m_abs = std::max(g.m_abs, (double)std::fabs(v));
            }
        }
    for (const Box& b : g.gb) g.scene.add(b);
    return g;
}
Box range_box(const Groups& g, int i, int j) {
    Box b;
    for (int k = i; k < j; k++) b.add(g.gb[k]);
    return b;
}

// The slot-order prices of a table over these groups (n = 0: the loop without clusters)
double slot_table_cost(const Groups& g, const rt2_cluster_table& t) {
    const int ng = (int)g.gb.size();
    if (t.n == 0) return kSlotGroup * ng;
    const double sa = g.scene.area();
    double v = 0.0;
    for (int k = 0; k < t.n; k++) {
        const int i = t.c[k].g0, j = t.c[k].g1_flags & 0xffff;
        const double r = sa > 0.0 ? range_box(g, i, j).area() / sa : 1.0;
        v += (t.c[k].g1_flags & RT2_CLUSTER_COMPACT) ? slot_compact_cost(j - i, r) : slot_full_cost(j - i);
    }
    return v;
}

// The dynamic programme of rt2_cluster_table_build with the slot-order prices; returns the table's price
double slot_table_build(const Groups& g, rt2_cluster_table* out) {
    std::memset(out, 0, sizeof(*out));
    const int ng = (int)g.gb.size();
    const double sa = g.scene.area();
    constexpr int K = RT2_MAX_CLUSTERS;
    const double inf = 1e300;
    std::vector<std::vector<double>> cost(K + 1, std::vector<double>(ng + 1, inf));
    std::vector<std::vector<int>> from(K + 1, std::vector<int>(ng + 1, -1));
    std::vector<std::vector<char>> cmp(K + 1, std::vector<char>(ng + 1, 0));
    cost[0][0] = 0.0;
    for (int j = 1; j <= ng; j++)
        for (int i = 0; i < j; i++) {
            const double r = sa > 0.0 ? range_box(g, i, j).area() / sa : 1.0;
            const double full = slot_full_cost(j - i), comp = slot_compact_cost(j - i, r);
            const bool c = comp < full;
            for (int k = 1; k <= K; k++) {
                if (cost[k - 1][i] >= inf) continue;
                const double v = cost[k - 1][i] + (c ? comp : full);
                if (v < cost[k][j]) {
                    cost[k][j] = v;
                    from[k][j] = i;
                    cmp[k][j] = c;
                }
            }
        }
    int bk = 1;
    for (int k = 2; k <= K; k++)
        if (cost[k][ng] < cost[bk][ng]) bk = k;
    const float pad = std::max((float)(g.m_abs * 0x1p-10), 0x1p-60f);
    out->far_o = std::max((float)(g.m_abs * 0x1p6), 1.0f);
    out->pad_abs = pad;
    bool any = false;
    for (int k = bk, j = ng; k >= 1; k--) {
        const int i = from[k][j];
        rt2_cluster& c = out->c[k - 1];
        const Box b = range_box(g, i, j);
        c.g0 = i;
        c.g1_flags = j | (cmp[k][j] ? RT2_CLUSTER_COMPACT : 0);
        any = any || cmp[k][j];
        for (int a = 0; a < 3; a++) {
            c.lo[a] = (float)b.lo[a] - pad;
            c.hi[a] = (float)b.hi[a] + pad;
        }
        j = i;
    }
    if (!any) {
        std::memset(out->c, 0, sizeof(out->c));
        return kSlotGroup * ng;
    }
    out->n = bk;
    return cost[bk][ng];
}

// The order with the `large` triangles of the largest boxes in front (ascending
// index) and the others cut by recursive median splits of their centroids
// along the longest axis of the centroids' box, every cut at a multiple of 32
// triangles; a leaf is one group in ascending index.  Ties by index throughout.
void slot_order(const rt2_triangle* tris, int32_t n_tris, int large, std::vector<int32_t>& slot) {
    std::vector<double> area(n_tris);
    std::vector<std::array<double, 3>> cen(n_tris);
    for (int i = 0; i < n_tris; i++) {
        Box b;
        b.add(tris[i].a), b.add(tris[i].b), b.add(tris[i].c);
        area[i] = b.area();
        for (int k = 0; k < 3; k++) cen[i][k] = 0.5 * (b.lo[k] + b.hi[k]);
    }
    slot.resize(n_tris);
    std::iota(slot.begin(), slot.end(), 0);
    large = std::min(large, (int)n_tris);
    auto by_area = [&](int32_t a, int32_t b) { return area[a] != area[b] ? area[a] > area[b] : a < b; };
    if (large > 0 && large < n_tris) std::nth_element(slot.begin(), slot.begin() + large, slot.end(), by_area);
    std::sort(slot.begin(), slot.begin() + large);
    struct Rec {
        static void split(std::vector<int32_t>& s, int lo, int hi, const std::vector<std::array<double, 3>>& cen) {
            const int n = hi - lo, ng = (n + 31) / 32;
            if (ng <= 1) {
                std::sort(s.begin() + lo, s.begin() + hi);
                return;
            }
            double mn[3] = {1e300, 1e300, 1e300}, mx[3] = {-1e300, -1e300, -1e300};
            for (int i = lo; i < hi; i++)
                for (int k = 0; k < 3; k++) {
                    mn[k] = std::min(mn[k], cen[s[i]][k]);
                    mx[k] = std::max(mx[k], cen[s[i]][k]);
                }
            int ax = 0;
            for (int k = 1; k < 3; k++)
                if (mx[k] - mn[k] > mx[ax] - mn[ax]) ax = k;
            const int mid = lo + 32 * (ng / 2);
            std::nth_element(s.begin() + lo, s.begin() + mid, s.begin() + hi, [&](int32_t a, int32_t b) {
                return cen[a][ax] != cen[b][ax] ? cen[a][ax] < cen[b][ax] : a < b;
            });
            split(s, lo, mid, cen);
            split(s, mid, hi, cen);
        }
    };
    Rec::split(slot, large, n_tris, cen);
}

}  // namespace

extern "C" int rt2_cluster_order_build(const rt2_triangle* tris, int32_t n_tris, int32_t* slot_tri,
                                       rt2_cluster_table* out) {
    if (!out || n_tris < 0 || (n_tris > 0 && (!tris || !slot_tri))) {
        rt2h::set_error("rt2_cluster_order_build: bad argument");
        return -1;
    }
    // the identity order and today's table, unless the rule's own projects cheaper
    std::iota(slot_tri, slot_tri + n_tris, 0);
    const int rc = rt2_cluster_table_build(tris, n_tris, out);
    if (rc < 0) return rc;
    const int ng = (n_tris + 31) / 32;
    if (ng < 2 || ng > 38) return out->n;  // one group has no order to choose; larger scenes are not resident
    const Groups g0 = group_boxes(tris, n_tris);
    if (!g0.finite || g0.m_abs > 0x1p20) return out->n;
    double best = slot_table_cost(g0, *out);
    std::vector<int32_t> slot;
    std::vector<rt2_triangle> perm(n_tris);
    for (int large : {32, 0}) {
        slot_order(tris, n_tris, large, slot);
        for (int s = 0; s < n_tris; s++) perm[s] = tris[slot[s]];
        rt2_cluster_table t;
        const double v = slot_table_build(group_boxes(perm.data(), n_tris), &t);
        if (t.n > 0 && v < best) {
            best = v;
            *out = t;
            std::copy(slot.begin(), slot.end(), slot_tri);
        }
    }
    return out->n;
}

extern "C" int rt2_cluster_table_build(const rt2_triangle* tris, int32_t n_tris, rt2_cluster_table* out) {
    if (!out || n_tris < 0 || (n_tris > 0 && !tris)) {
        rt2h::set_error("rt2_cluster_table_build: bad argument");
        return -1;
    }
    std::memset(out, 0, sizeof(*out));
    const int ng = (n_tris + 31) / 32;
    if (ng == 0) return 0;
    std::vector<Box> gb(ng);
    Box scene;
    double m_abs = 0.0;
    bool finite = true;
    for (int i = 0; i < n_tris; i++) {
        for (const rt2_vec4* p : {&tris[i].a, &tris[i].b, &tris[i].c}) {
            gb[i >> 5].add(*p);
            for (float v : {p->x, p->y, p->z}) {
                finite = finite && std::isfinite(v);
                m_abs = std::max(m_abs, (double)std::fabs(v));
            }
        }
    }
    // a scene outside the matrix filter's range never reaches the kernel
    if (!finite || m_abs > 0x1p20) return 0;
    for (int g = 0; g < ng; g++) scene.add(gb[g]);
    const double sa = scene.area();
    // boxes of every range [i, j)
    auto range_box = [&](int i, int j) {
        Box b;
        for (int g = i; g < j; g++) b.add(gb[g]);
        return b;
    };
    // cost[k][j]: the cheapest cover of groups [0, j) by k clusters
    constexpr int K = RT2_MAX_CLUSTERS;
    const double inf = 1e300;
    std::vector<std::vector<double>> cost(K + 1, std::vector<double>(ng + 1, inf));
    std::vector<std::vector<int>> from(K + 1, std::vector<int>(ng + 1, -1));
    std::vector<std::vector<char>> cmp(K + 1, std::vector<char>(ng + 1, 0));
    cost[0][0] = 0.0;
    for (int k = 1; k <= K; k++)
        for (int j = 1; j <= ng; j++)
            for (int i = k - 1; i < j; i++) {
                if (cost[k - 1][i] >= inf) continue;
                const double r = sa > 0.0 ? range_box(i, j).area() / sa : 1.0;
                const double full = kFullGroup * (j - i), comp = compact_cost(j - i, r);
                const bool c = comp < full;
                const double v = cost[k - 1][i] + kPerCluster + (c ? comp : full);
                if (v < cost[k][j]) {
                    cost[k][j] = v;
                    from[k][j] = i;
                    cmp[k][j] = c;
                }
            }
    int bk = 1;
    for (int k = 2; k <= K; k++)
        if (cost[k][ng] < cost[bk][ng]) bk = k;
    std::vector<rt2_cluster> cl(bk);
    bool any = false;
    // The padding: 2^-10 of the scene's largest |coordinate| on every side (and
    // never zero).  far_o = 2^6 of the same: within it the padding covers the
    // reference test's rounding, which grows with the origin's distance.
    const float pad = std::max((float)(m_abs * 0x1p-10), 0x1p-60f);
    for (int k = bk, j = ng; k >= 1; k--) {
        const int i = from[k][j];
        rt2_cluster& c = cl[k - 1];
        const Box b = range_box(i, j);
        c.g0 = i;
        c.g1_flags = j | (cmp[k][j] ? RT2_CLUSTER_COMPACT : 0);
        any = any || cmp[k][j];
        for (int a = 0; a < 3; a++) {
            c.lo[a] = (float)b.lo[a] - pad;
            c.hi[a] = (float)b.hi[a] + pad;
        }
        j = i;
    }
    out->far_o = std::max((float)(m_abs * 0x1p6), 1.0f);
    out->pad_abs = pad;
    if (!any) return 0;
    out->n = bk;
    std::copy(cl.begin(), cl.end(), out->c);
    return bk;
}

extern "C" int rt2_cluster_need(const rt2_cluster_table* t, const rt2_ray* rays, int64_t n_rays, uint32_t* bits) {
    if (!t || n_rays < 0 || (n_rays > 0 && (!rays || !bits)) || t->n < 0 || t->n > RT2_MAX_CLUSTERS) {
        rt2h::set_error("rt2_cluster_need: bad argument");
        return -1;
    }
    const uint32_t all = t->n ? (t->n == 32 ? ~0u : (1u << t->n) - 1u) : 0u;
    for (int64_t i = 0; i < n_rays; i++) {
        const float* o = rays[i].o;
        const float* d = rays[i].d;
        const float om = std::max(std::max(std::fabs(o[0]), std::fabs(o[1])), std::fabs(o[2]));
        const float dm = std::max(std::max(std::fabs(d[0]), std::fabs(d[1])), std::fabs(d[2]));
        // outside the filter's range (rt2_mfma.h mfma_scale; NaN too): the kernel's drain takes the wave
        if (!(om <= 0x1p20f && dm <= 1.0001f) || rt2_cluster_always(o, d, t->far_o)) {
            bits[i] = all;
            continue;
        }
        float inv[3];
        rt2_cluster_inv(d, inv);
        uint32_t m = 0;
        for (int k = 0; k < t->n; k++) {
            const rt2_cluster& c = t->c[k];
            if (!(c.g1_flags & RT2_CLUSTER_COMPACT) || rt2_cluster_need_box(c.lo, c.hi, o, inv)) m |= 1u << k;
        }
        bits[i] = m;
    }
    return 0;
}
