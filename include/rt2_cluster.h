/* Triangle-group clusters of the resident matrix-filter kernel and the per-ray
 * "need" test that lets a wave sweep a compact cluster with only the rays
 * whose segment can meet it (DESIGN.md "Compact clusters").
 *
 * One text for host and device: plain f32 operations, one correctly rounded
 * division per direction component, no contraction on either side, so the
 * host entry point (rt2_cluster_need) gives the bits the kernel computes.
 *
 * Not part of the drop-in surface of rt2.h: the table is derived data of a
 * scene (rt2_scene_export selector 7) and the two entry points are test hooks.
 */
#ifndef RT2_CLUSTER_H
#define RT2_CLUSTER_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RT2_CLUSTER_HD __host__ __device__ __forceinline__
#else
#define RT2_CLUSTER_HD static inline
#endif

#define RT2_MAX_CLUSTERS 13          /* a sweep's need masks: two lanes each of the VGPR that holds the 38 hot masks */
#define RT2_CLUSTER_COMPACT 0x10000  /* flag in rt2_cluster::g1_flags */

/* groups [g0, g1) of 32 triangles; a compact cluster carries its padded box */
typedef struct rt2_cluster {
    float lo[3];
    int32_t g0;
    float hi[3];
    int32_t g1_flags; /* g1 | RT2_CLUSTER_COMPACT */
} rt2_cluster;        /* 32 B */

typedef struct rt2_cluster_table {
    float far_o;    /* a ray with a |origin component| above this needs every cluster */
    int32_t n;      /* clusters; 0 = no compact cluster (the kernel's loop without clusters) */
    float pad_abs;  /* the padding every box carries (informational) */
    int32_t reserved[5];
    rt2_cluster c[RT2_MAX_CLUSTERS];
} rt2_cluster_table; /* 32 + 32 RT2_MAX_CLUSTERS B */

#define RT2_CLUSTER_DMIN 0x1p-100f      /* a direction component at or below this: the ray needs every cluster */
#define RT2_CLUSTER_SLACK 1.0000152587890625f /* 1 + 2^-16 on the far distance: the test's own rounding (6 x 2^-24) */

RT2_CLUSTER_HD float rt2_cl_min(float a, float b) { return __builtin_fminf(a, b); }
RT2_CLUSTER_HD float rt2_cl_max(float a, float b) { return __builtin_fmaxf(a, b); }
RT2_CLUSTER_HD float rt2_cl_abs(float a) { return __builtin_fabsf(a); }

/* Rays the box arithmetic is not trusted with: a direction component of +-0
 * or below 2^-100 in magnitude (its reciprocal overflows or its products
 * with box distances do; NaN fails the comparison too), or an origin beyond
 * the distance the boxes' padding is sized for.  They need every cluster. */
RT2_CLUSTER_HD int rt2_cluster_always(const float o[3], const float d[3], float far_o) {
    const float dm = rt2_cl_min(rt2_cl_min(rt2_cl_abs(d[0]), rt2_cl_abs(d[1])), rt2_cl_abs(d[2]));
    const float om = rt2_cl_max(rt2_cl_max(rt2_cl_abs(o[0]), rt2_cl_abs(o[1])), rt2_cl_abs(o[2]));
    return !(dm > RT2_CLUSTER_DMIN) || !(om <= far_o);
}

RT2_CLUSTER_HD void rt2_cluster_inv(const float d[3], float inv[3]) {
    inv[0] = 1.0f / d[0];
    inv[1] = 1.0f / d[1];
    inv[2] = 1.0f / d[2];
}

/* The slab test of the half line o + t d, t >= 0, against the padded box, for
 * a ray rt2_cluster_always() does not claim: every value is finite.  Only a
 * box wholly behind the origin (far < 0) or an empty intersection of the
 * three slabs (far (1 + 2^-16) < near) says "does not need". */
RT2_CLUSTER_HD int rt2_cluster_need_box(const float lo[3], const float hi[3], const float o[3], const float inv[3]) {
    const float ax = (lo[0] - o[0]) * inv[0], bx = (hi[0] - o[0]) * inv[0];
    const float ay = (lo[1] - o[1]) * inv[1], by = (hi[1] - o[1]) * inv[1];
    const float az = (lo[2] - o[2]) * inv[2], bz = (hi[2] - o[2]) * inv[2];
    const float tn = rt2_cl_max(rt2_cl_max(rt2_cl_min(ax, bx), rt2_cl_min(ay, by)), rt2_cl_min(az, bz));
    const float tf = rt2_cl_min(rt2_cl_min(rt2_cl_max(ax, bx), rt2_cl_max(ay, by)), rt2_cl_max(az, bz));
    return !(tf < 0.0f) && !(tf * RT2_CLUSTER_SLACK < tn);
}

#ifdef __cplusplus
extern "C" {
#endif
struct rt2_triangle;
struct rt2_ray;
/* The cluster table of a triangle list (what rt2_scene_create derives for a
 * scene of at most 38 groups).  Returns the number of clusters, < 0 on a bad
 * argument.  Host only: no device is touched. */
int rt2_cluster_table_build(const struct rt2_triangle* tris, int32_t n_tris, rt2_cluster_table* out);
/* The slot order of a scene of at most 38 groups (DESIGN.md "Slot order"):
 * slot_tri is a permutation of [0, n_tris), slot s holds triangle slot_tri[s],
 * group g the slots 32 g .. 32 g + 31, and `out` is the table over those slot
 * groups.  The rule reads the vertices only and is deterministic.  Where its
 * own order does not project cheaper than the index order, the result is the
 * identity and rt2_cluster_table_build's table.  Returns the number of
 * clusters, < 0 on a bad argument.  Host only. */
int rt2_cluster_order_build(const struct rt2_triangle* tris, int32_t n_tris, int32_t* slot_tri, rt2_cluster_table* out);
/* bits[i]: bit k set when ray i needs cluster k (a full cluster's bit is always
 * set; a ray outside the filter's range, which the kernel hands to its drain,
 * gets every bit).  Host only. */
int rt2_cluster_need(const rt2_cluster_table* t, const struct rt2_ray* rays, int64_t n_rays, uint32_t* bits);
#ifdef __cplusplus
}
#endif

#endif
