// The cluster table of the resident matrix-filter kernel (include/rt2_cluster.h;
// DESIGN.md "Compact clusters"): the scene's 32-triangle groups, in index order,
// cut into at most RT2_MAX_CLUSTERS contiguous ranges, each either full (swept
// by all the wave's rays, as before) or compact (swept by the rays whose
// segment can meet its padded box).  The rule reads the triangles only.
#include <algorithm>
#include <cmath>
#include <cstring>
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

}  // namespace

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
