// MI355X (gfx950) render path: the per-pixel Monte-Carlo loop of
// RayTracing/Assets/Shaders/compute.glsl:472-701 as persistent HIP kernels,
// plus the device half of the C-ABI (include/rt2.h).
//
// Unit of work ("item") = one pixel-frame of the shard: its numRaysPerPixel
// rays run in order on one lane, like one compute.glsl invocation (the rays of
// a pixel-frame share one sequential RNG stream, compute.glsl:668/683).
//
// Execution model:
//   - one lane = one item at a time; every loop iteration each lane traces ONE
//     segment (closest-hit query + scatter) of its current ray, and a lane
//     whose item ends is refilled from a global counter (one atomic per wave);
//   - closest hit: brute force over all triangles (rt2_sweep.h, rt2_brute.h)
//     or the reference BVH's traversal order (rt2_bvh.h); both bit-identical
//     to the CPU oracle under the numerics contract of rt2_math.h;
//   - traceBasic preview, frame accumulation, cost-ordered scheduling and the
//     8-bit resolve live in rt2_misc_kernels.h.
//
// The headers are parts of this one translation unit (anonymous namespace,
// included below in dependency order), split only for reading.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <numeric>
#include <string>
#include <type_traits>
#include <vector>

#include "../../../include/rt2.h"
#include "../../../include/rt2_cluster.h"
#include "rt2_math.h"

using namespace rt2d;

#include "rt2_sweep.h"
#include "rt2_path.h"
#include "rt2_brute.h"
#include "rt2_mfma.h"
#include "rt2_k5_tiles.h"
#include "rt2_k5_resident.h"
#include "rt2_assist.h"
#include "rt2_bvh.h"
#include "rt2_misc_kernels.h"
#include "rt2_query.h"
#include "rt2_occluded.h"
#include "rt2_surface.h"
#include "rt2_shade.h"
#include "rt2_radiance.h"

/* =========================================================================
 * C-ABI, device half
 * ======================================================================= */
namespace rt2h {
void set_error(const std::string& msg);
}

#define HIPCHECK(expr)                                                                         \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) {                                                                \
            rt2h::set_error(std::string(#expr) + ": " + hipGetErrorString(e_));                \
            return -1;                                                                         \
        }                                                                                      \
    } while (0)

constexpr int kCounters = 32;  // [0] items, [1..7] stats + wave-end, [8..] kernel diagnostics
struct Staging {  // a device buffer grown on demand (staging_grow), freed with the scene
    void* ptr = nullptr;
    size_t cap = 0;  // bytes
    template <class T>
    T* as() const {
        return static_cast<T*>(ptr);
    }
};
struct rt2_scene {
    int device = 0;
    int n_tris = 0, n_mats = 0, n_nodes = 0;
    rt2_triangle* d_raw = nullptr;
    float4* d_tri = nullptr;
    float4* d_unit_n = nullptr;                 // per-triangle unit normal (prep_unit_normals)
    int* d_mtl = nullptr;
    rt2_material* d_mats = nullptr;
    rt2_node* d_nodes = nullptr;
    float4* d_recs = nullptr;                   // BVH v2 child-pair records
    float4* d_plk = nullptr;                    // sweep_plk filter records (4 float4 per triangle)
    int plk_ok = 0;                             // sweep_plk usable: <= 1/64 of the triangles outside its range
    int plk_outside = 0;                        // triangles with an always-pass record
    float plk_A = 0.0f;                         // max |a_i| over the triangles
    _Float16* d_mfma = nullptr;                 // 16x16x32 filter records (the filter probe's layout 0; ensure_mfma16)
    float* d_mfma_tau = nullptr;                // per-triangle record scale
    _Float16* d_mfma_k16 = nullptr;             // sweep_k16 records (32-triangle groups, 7 KiB each)
    float* d_mfma_k16_tau = nullptr;            // per-triangle record scale (same values as d_mfma_tau)
    float2* d_mfma_k16_bnd = nullptr;           // per-triangle m.z residual bounds of the 5-product form (k5)
    _Float16* d_mfma_kt = nullptr;              // kthr records (threshold in the K-slots: 4 KiB per 32 triangles)
    int mfma_ok = 0;                            // render_mfma usable (records built, scene in range)
    rt2_cluster_table clusters = {};            // MfmaSpec::cluster_rows: the groups' clusters (n = 0: none compact)
    void* d_slot = nullptr;                     // MfmaSpec::slot_order: the slot image of a scene of <= kResGroups groups
                                                // (kt records, slot table, prepared triangles, slot_tri, in slot order)
    rt2_cluster_table slot_table = {};          // ... its table over the slot groups
    std::vector<int32_t> slot_tri;              // ... slot s holds triangle slot_tri[s]
    float mfma_A = 0.0f;                        // max |a_i| over the in-range triangles
    uchar4* d_texels = nullptr;                 // textures, RGBA8
    int4* d_tex_desc = nullptr;
    int n_tex = 0;
    int bvh_root = 0;                           // BVH v2 stack entry of node 0
    int recs_ok = 0;                            // BVH v3 fast-path precondition on the boxes
    int split_frames = 1;                       // frame-major (frame, pixel) items when F > 1
    unsigned long long frame_scratch_cap = 2ull << 30;  // bytes of per-frame planes per launch
    int cost_order = 0;                         // order items by the previous launch's per-pixel cost (opt-in)
    unsigned long long cost_npix = 0;           // pixels the cost map describes (0 = none)
    int cost_key[4] = {0, 0, 0, 0};             // W, tile_rows, rank, nranks the map belongs to
    hipEvent_t last_launch = nullptr;           // renders of one scene are ordered (shared scratch)
    bool last_launch_valid = false;
    unsigned long long* d_counters = nullptr;  // [0] item counter, [1] segments
    unsigned long long samples = 0, tests_per_seg = 0;
    int variant = 0;
    int last_variant = -1;
    int traversal = RT2_TRAVERSAL_BRUTE;
    int bvh_depth = 0;              // longest root-to-leaf path (nodes)
    int last_kind = 0;              // kind of the last launch (stats: tests)
    unsigned long long diag[kCounters] = {};
    int num_cus = 256;
    size_t max_lds = 65536;
    // Scratch of the launches, grown inside a launch on the caller's stream (DESIGN.md "The render launcher"):
    Staging fb;                     // frame_split scratch (per-frame colours; linear renders: moment slots)
    Staging cost, order, hist;      // cost order: per-pixel cost map of the last launch, pixel order for the next
                                    // launch, 32 counters
    Staging region_ctr;             // 8 item-region counters, 128 B apart
    // The stream the blocking wrappers run on, and their device buffers, reused across calls.  One set of images
    // serves rt2_render_host and rt2_render_linear_host, and one set of staging the ray queries' and ray generators'
    // seven *_host entry points, because every one of those calls runs on host_stream and ends in
    // hipStreamSynchronize: no buffer is in use when the next call starts.
    hipStream_t host_stream = nullptr;
    Staging host_img[4];            // float sums; 8-bit sums or second moments; the two resolved outputs
    Staging stage_rays, stage_rng, stage_out;  // the rays, the RNG words and the output bytes
    int query_arm = 0;                // experiment build: A/B arm of the resident query kernel
    int occluded_arm = 0;             // experiment build: A/B arm of occluded_k5r
    unsigned long long* wave_log = nullptr;  // diagnostic wave timeline (rt2_scene_set_wave_log)
    uint32_t wave_log_n = 0;
};

// Validates a reference node array (BVH.h layout) against the triangle count
// and returns its depth; < 0 on a malformed array (child out of range, cycle,
// leaf range outside the triangles).
static int bvh_depth_check(const rt2_node* nodes, int n_nodes, int n_tris, std::string& err) {
    if (n_nodes < 1) {
        err = "empty node array";
        return -1;
    }
    std::vector<int> depth(n_nodes, 0);
    std::vector<int> stack;
    stack.push_back(0);
    depth[0] = 1;
    int maxd = 1;
    long long visited = 0;
    while (!stack.empty()) {
        const int i = stack.back();
        stack.pop_back();
        if (++visited > n_nodes) {
            err = "node graph is not a tree";
            return -1;
        }
        const rt2_node& n = nodes[i];
        if (n.childIndex == -1) {
            if (n.triangleCount > 0 && (n.triangleIndex < 0 || (long long)n.triangleIndex + n.triangleCount > n_tris)) {
                err = "leaf " + std::to_string(i) + " references triangles outside [0, " + std::to_string(n_tris) + ")";
                return -1;
            }
            continue;
        }
        if (n.childIndex <= 0 || n.childIndex + 1 >= n_nodes) {
            err = "node " + std::to_string(i) + " has child index " + std::to_string(n.childIndex) + " out of range";
            return -1;
        }
        for (int c = n.childIndex; c <= n.childIndex + 1; c++) {
            depth[c] = depth[i] + 1;
            maxd = std::max(maxd, depth[c]);
            stack.push_back(c);
        }
    }
    return maxd;
}

// Child-pair records for render_bvh2 (layout: see bvh_step).  Interior nodes
// are numbered in depth-first pre-order (parents before children, left
// subtree first) so records of a subtree are contiguous.
static int bvh_records(const rt2_node* nodes, int n_nodes, std::vector<float4>& rec, int& root, std::string& err) {
    if (n_nodes >= (1 << 26)) {
        err = "more than 2^26 nodes";
        return -1;
    }
    std::vector<int> rid(n_nodes, -1);
    int n_int = 0;
    std::vector<int> stack{0};
    while (!stack.empty()) {
        const int i = stack.back();
        stack.pop_back();
        if (nodes[i].childIndex == -1) continue;
        rid[i] = n_int++;
        stack.push_back(nodes[i].childIndex + 1);
        stack.push_back(nodes[i].childIndex);
    }
    auto enc = [&](int i) -> int {
        const rt2_node& n = nodes[i];
        if (n.childIndex != -1) return rid[i];
        const int cnt = std::max(n.triangleCount, 0);
        const int start = cnt > 0 ? n.triangleIndex : 0;
        if (cnt <= 30 && start >= 0 && start < (1 << 26)) return ~((start << 5) | cnt);
        return ~((i << 5) | 31);
    };
    rec.assign((size_t)std::max(n_int, 1) * 4, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    for (int i = 0; i < n_nodes; i++) {
        if (rid[i] < 0) continue;
        const rt2_node& A = nodes[nodes[i].childIndex];
        const rt2_node& B = nodes[nodes[i].childIndex + 1];
        float4* r = &rec[(size_t)rid[i] * 4];
        r[0] = make_float4(A.bmin[0], A.bmin[1], A.bmin[2], A.bmax[0]);
        r[1] = make_float4(A.bmax[1], A.bmax[2], B.bmin[0], B.bmin[1]);
        r[2] = make_float4(B.bmin[2], B.bmax[0], B.bmax[1], B.bmax[2]);
        int e[4] = {enc(nodes[i].childIndex), enc(nodes[i].childIndex + 1), 0, 0};
        std::memcpy(&r[3], e, sizeof(e));
    }
    root = enc(0);
    return n_int;
}

// GL's unpack of a tightly packed stb image (GL_UNPACK_ALIGNMENT 4: rows
// start every align4(w*n) bytes; bytes past the buffer read as 0 — the
// reference reads past its allocation there) into RGBA8, with the swizzles of
// Texture2D(path) (1 channel: r,r,r,1; GL_RG: r,g,0,1; GL_RGB: r,g,b,1).
static void gl_unpack_rgba8(const rt2_image& im, uchar4* out) {
    const size_t n = (size_t)im.channels, stride = ((size_t)im.width * n + 3) & ~(size_t)3;
    const size_t total = (size_t)im.width * im.height * n;
    auto at = [&](size_t i) -> uint8_t { return i < total ? im.pixels[i] : (uint8_t)0; };
    for (int j = 0; j < im.height; j++)
        for (int i = 0; i < im.width; i++) {
            const size_t b = (size_t)j * stride + (size_t)i * n;
            uchar4 t;
            if (n == 1) t = make_uchar4(at(b), at(b), at(b), 255);
            else if (n == 2) t = make_uchar4(at(b), at(b + 1), 0, 255);
            else if (n == 3) t = make_uchar4(at(b), at(b + 1), at(b + 2), 255);
            else t = make_uchar4(at(b), at(b + 1), at(b + 2), at(b + 3));
            out[(size_t)j * im.width + i] = t;
        }
}

extern "C" int rt2_scene_set_textures(rt2_scene* s, const rt2_image* images, int32_t n) {
    if (!s || n < 0 || (n > 0 && !images)) {
        rt2h::set_error("rt2_scene_set_textures: bad argument");
        return -1;
    }
    size_t total = 0;
    for (int i = 0; i < n; i++) {
        const rt2_image& im = images[i];
        if (im.width < 1 || im.height < 1 || im.channels < 1 || im.channels > 4 || !im.pixels) {
            rt2h::set_error("rt2_scene_set_textures: image " + std::to_string(i) + " is empty or has " +
                            std::to_string(im.channels) + " channels");
            return -1;
        }
        total += (size_t)im.width * im.height;
    }
    HIPCHECK(hipSetDevice(s->device));
    HIPCHECK(hipDeviceSynchronize());
    (void)hipFree(s->d_texels);
    (void)hipFree(s->d_tex_desc);
    s->d_texels = nullptr;
    s->d_tex_desc = nullptr;
    s->n_tex = 0;
    if (n == 0) return 0;
    std::vector<uchar4> host(total);
    std::vector<int4> desc(n);
    size_t off = 0;
    for (int i = 0; i < n; i++) {
        gl_unpack_rgba8(images[i], host.data() + off);
        desc[i] = make_int4(images[i].width, images[i].height, (int)(uint32_t)(off & 0xffffffffu), (int)(off >> 32));
        off += (size_t)images[i].width * images[i].height;
    }
    HIPCHECK(hipMalloc(&s->d_texels, total * sizeof(uchar4)));
    HIPCHECK(hipMalloc(&s->d_tex_desc, n * sizeof(int4)));
    HIPCHECK(hipMemcpy(s->d_texels, host.data(), total * sizeof(uchar4), hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(s->d_tex_desc, desc.data(), n * sizeof(int4), hipMemcpyHostToDevice));
    s->n_tex = n;
    return 0;
}

// Not in rt2.h (test hook): bytes of per-frame colour planes one launch may use.
extern "C" int rt2_scene_set_frame_scratch_cap(rt2_scene* s, unsigned long long bytes) {
    if (!s || bytes == 0) return -1;
    s->frame_scratch_cap = bytes;
    return 0;
}

extern "C" int rt2_scene_set_cost_order(rt2_scene* s, int enable) {
    if (!s) {
        rt2h::set_error("rt2_scene_set_cost_order: null scene");
        return -1;
    }
    s->cost_order = enable ? 1 : 0;
    s->cost_npix = 0;  // forget the map
    return 0;
}

// Not in rt2.h (diagnostics): the assist kernel writes a per-wave timeline
// {start, first item-less lane, end, segments} in 10-ns ticks to d_log
// (4 x u64 per wave, n waves; null turns it off).
extern "C" int rt2_scene_set_wave_log(rt2_scene* s, unsigned long long* d_log, uint32_t n) {
    if (!s) return -1;
    s->wave_log = d_log;
    s->wave_log_n = d_log ? n : 0;
    return 0;
}

extern "C" int rt2_scene_set_frame_split(rt2_scene* s, int enable) {
    if (!s) {
        rt2h::set_error("rt2_scene_set_frame_split: null scene");
        return -1;
    }
    s->split_frames = enable ? 1 : 0;
    return 0;
}

extern "C" int rt2_scene_set_traversal(rt2_scene* s, int traversal) {
    if (!s || (traversal != RT2_TRAVERSAL_BRUTE && traversal != RT2_TRAVERSAL_BVH)) {
        rt2h::set_error("rt2_scene_set_traversal: bad argument");
        return -1;
    }
    if (traversal == RT2_TRAVERSAL_BVH && s->n_nodes == 0) {
        rt2h::set_error("rt2_scene_set_traversal: BVH traversal needs the node array (rt2_scene_create nodes)");
        return -1;
    }
    s->traversal = traversal;
    return 0;
}

static int scene_init(rt2_scene* s, const rt2_triangle* tris, int32_t n_tris, const rt2_material* mats,
                      int32_t n_mats, const rt2_node* nodes, int32_t n_nodes, int32_t device);
static int build_slot_image(rt2_scene* s);

extern "C" int rt2_scene_create(const rt2_triangle* tris, int32_t n_tris, const rt2_material* mats, int32_t n_mats,
                                const rt2_node* nodes, int32_t n_nodes, int32_t device, rt2_scene** out) {
    if (!out || n_tris < 0 || n_mats < 1 || !mats || (n_tris > 0 && !tris)) {
        rt2h::set_error("rt2_scene_create: bad argument");
        return -1;
    }
    for (int i = 0; i < n_tris; i++) {
        if (tris[i].materialIndex < 0 || tris[i].materialIndex >= n_mats) {
            rt2h::set_error("rt2_scene_create: triangle " + std::to_string(i) + " has material index " +
                            std::to_string(tris[i].materialIndex) + " outside [0, " + std::to_string(n_mats) + ")");
            return -1;
        }
    }
    int ndev = 0;
    HIPCHECK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) {
        rt2h::set_error("rt2_scene_create: no HIP device " + std::to_string(device));
        return -1;
    }
    HIPCHECK(hipSetDevice(device));
    rt2_scene* s = new rt2_scene();
    if (scene_init(s, tris, n_tris, mats, n_mats, nodes, n_nodes, device) != 0) {
        rt2_scene_destroy(s);  // frees whatever was allocated before the failure
        return -1;
    }
    *out = s;
    return 0;
}

// Uploads and derived device arrays of rt2_scene_create; on failure returns
// -1 with the error set and leaves the partial scene to the caller to destroy.
static int scene_init(rt2_scene* s, const rt2_triangle* tris, int32_t n_tris, const rt2_material* mats,
                      int32_t n_mats, const rt2_node* nodes, int32_t n_nodes, int32_t device) {
    s->device = device;
    s->n_tris = n_tris;
    s->n_mats = n_mats;
    s->n_nodes = nodes ? n_nodes : 0;
    hipDeviceProp_t prop;
    HIPCHECK(hipGetDeviceProperties(&prop, device));
    s->num_cus = prop.multiProcessorCount;
    s->max_lds = prop.maxSharedMemoryPerMultiProcessor ? prop.maxSharedMemoryPerMultiProcessor : 65536;
    const size_t nt = (size_t)std::max(n_tris, 1);
    HIPCHECK(hipMalloc(&s->d_raw, nt * sizeof(rt2_triangle)));
    HIPCHECK(hipMalloc(&s->d_tri, nt * 3 * sizeof(float4)));
    HIPCHECK(hipMalloc(&s->d_unit_n, nt * sizeof(float4)));
    HIPCHECK(hipMalloc(&s->d_mtl, nt * sizeof(int)));
    HIPCHECK(hipMalloc(&s->d_mats, (size_t)n_mats * sizeof(rt2_material)));
    HIPCHECK(hipMalloc(&s->d_counters, kCounters * sizeof(unsigned long long)));
    HIPCHECK(hipMemset(s->d_counters, 0, kCounters * sizeof(unsigned long long)));
    if (n_tris > 0) HIPCHECK(hipMemcpy(s->d_raw, tris, (size_t)n_tris * sizeof(rt2_triangle), hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(s->d_mats, mats, (size_t)n_mats * sizeof(rt2_material), hipMemcpyHostToDevice));
    if (s->n_nodes > 0) {
        std::string err;
        s->bvh_depth = bvh_depth_check(nodes, n_nodes, n_tris, err);
        if (s->bvh_depth < 0 || s->bvh_depth > 62) {
            if (s->bvh_depth > 62) err = "BVH deeper than compute.glsl's 64-entry stack";
            rt2h::set_error("rt2_scene_create: bad node array: " + err);
            return -1;
        }
        HIPCHECK(hipMalloc(&s->d_nodes, (size_t)n_nodes * sizeof(rt2_node)));
        HIPCHECK(hipMemcpy(s->d_nodes, nodes, (size_t)n_nodes * sizeof(rt2_node), hipMemcpyHostToDevice));
        std::vector<float4> rec;
        if (bvh_records(nodes, n_nodes, rec, s->bvh_root, err) < 0) {
            rt2h::set_error("rt2_scene_create: bad node array: " + err);
            return -1;
        }
        // the first three float4 of a record are box coordinates (the 4th: stack entries)
        s->recs_ok = 1;
        for (size_t i = 0; i < rec.size(); i++) {
            if (i % 4 == 3) continue;
            for (float c : {rec[i].x, rec[i].y, rec[i].z, rec[i].w})
                if (!(c == 0.0f || (std::fabs(c) >= 0x1p-37f && std::fabs(c) <= 0x1p59f))) s->recs_ok = 0;
        }
        HIPCHECK(hipMalloc(&s->d_recs, rec.size() * sizeof(float4)));
        HIPCHECK(hipMemcpy(s->d_recs, rec.data(), rec.size() * sizeof(float4), hipMemcpyHostToDevice));
    }
    if (n_tris > 0) {
        hipLaunchKernelGGL(prep_triangles, dim3((n_tris + 255) / 256), dim3(256), 0, 0, s->d_raw, n_tris, s->d_tri,
                           s->d_mtl);
        HIPCHECK(hipGetLastError());
        hipLaunchKernelGGL(prep_unit_normals, dim3((n_tris + 255) / 256), dim3(256), 0, 0, s->d_tri, n_tris,
                           s->d_unit_n);
        HIPCHECK(hipGetLastError());
#ifdef RT2_EXPERIMENTS
        HIPCHECK(hipMalloc(&s->d_plk, nt * 4 * sizeof(float4)));
        // two scratch words in an unused counter slot (zeroed again below)
        uint32_t* d_flags = reinterpret_cast<uint32_t*>(s->d_counters + kCounters - 2);
        HIPCHECK(hipMemset(d_flags, 0, 2 * sizeof(uint32_t)));
        hipLaunchKernelGGL(prep_plk, dim3((n_tris + 255) / 256), dim3(256), 0, 0, s->d_tri, n_tris, s->d_plk, d_flags);
        HIPCHECK(hipGetLastError());
        uint32_t flags[2];
        HIPCHECK(hipMemcpy(flags, d_flags, sizeof(flags), hipMemcpyDeviceToHost));
        HIPCHECK(hipMemset(d_flags, 0, 2 * sizeof(uint32_t)));
        s->plk_outside = (int)flags[0];
        s->plk_ok = (unsigned long long)flags[0] * 64 <= (unsigned long long)n_tris;  // <= 1/64 always-pass records
        std::memcpy(&s->plk_A, &flags[1], sizeof(float));
#endif
        // matrix-core filter records in the k16 layout (sweep_k16 and its
        // 5-product form): 7 KiB per 32 triangles; the prep's flags give the
        // scene's largest |a_i|, the filter's range check.  (The 16x16x32
        // layout of the probe's layout 0 is built on first use: ensure_mfma16.)
        const int n_pad32 = (n_tris + 31) / 32 * 32;
        HIPCHECK(hipMalloc(&s->d_mfma_k16, (size_t)n_pad32 * kK16Ops * 16 * sizeof(_Float16)));
        HIPCHECK(hipMalloc(&s->d_mfma_k16_tau, (size_t)n_pad32 * sizeof(float)));
        HIPCHECK(hipMalloc(&s->d_mfma_k16_bnd, (size_t)n_pad32 * sizeof(float2)));
        uint32_t* d_mflags = reinterpret_cast<uint32_t*>(s->d_counters + kCounters - 2);
        HIPCHECK(hipMemset(d_mflags, 0, 2 * sizeof(uint32_t)));
        hipLaunchKernelGGL(prep_mfma_k16, dim3((n_pad32 + 255) / 256), dim3(256), 0, 0, s->d_tri, n_tris, n_pad32,
                           s->d_mfma_k16, s->d_mfma_k16_tau, s->d_mfma_k16_bnd, d_mflags);
        HIPCHECK(hipGetLastError());
        uint32_t mflags[2];
        HIPCHECK(hipMemcpy(mflags, d_mflags, sizeof(mflags), hipMemcpyDeviceToHost));
        HIPCHECK(hipMemset(d_mflags, 0, 2 * sizeof(uint32_t)));
        std::memcpy(&s->mfma_A, &mflags[1], sizeof(float));
        s->mfma_ok = s->mfma_A <= 0x1p20f;
        // the kthr records (rt2_mfma.h prep_mfma_kt: the threshold in the
        // K-slots), 4 KiB per 32 triangles; its flags duplicate the above
        // ... and behind them the cluster table of a scene the resident kernel holds whole (MfmaSpec::cluster_rows;
        // rt2_cluster.h), n = 0 for every other scene
        const size_t kt_bytes = (size_t)n_pad32 * kKtOps * 16 * sizeof(_Float16);
        if (n_pad32 / 32 <= kResGroups && rt2_cluster_table_build(tris, n_tris, &s->clusters) < 0) return -1;
        HIPCHECK(hipMalloc(&s->d_mfma_kt, kt_bytes + sizeof(s->clusters)));
        HIPCHECK(hipMemcpy(reinterpret_cast<char*>(s->d_mfma_kt) + kt_bytes, &s->clusters, sizeof(s->clusters),
                           hipMemcpyHostToDevice));
        hipLaunchKernelGGL(prep_mfma_kt, dim3((n_pad32 + 255) / 256), dim3(256), 0, 0, s->d_tri, n_tris, n_pad32,
                           s->d_mfma_kt, d_mflags);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipDeviceSynchronize());
        HIPCHECK(hipMemset(d_mflags, 0, 2 * sizeof(uint32_t)));
        // MfmaSpec::cluster_rows16 multiplies every record slot of a resident scene by a zero of the other
        // triangle half's fragment: every f16 must be finite, the padding columns' too (0 x inf is NaN).
        // mfma_slots makes them from coefficients the range check bounds; this checks the bits once per scene.
        // A scene that fails leaves the matrix filter's range like one with a coordinate above 2^20.
        if (s->mfma_ok && n_pad32 / 32 <= kResGroups) {
            std::vector<uint16_t> rec(kt_bytes / sizeof(uint16_t));
            HIPCHECK(hipMemcpy(rec.data(), s->d_mfma_kt, kt_bytes, hipMemcpyDeviceToHost));
            for (uint16_t h : rec)
                if ((h & 0x7c00u) == 0x7c00u) s->mfma_ok = 0;
            // the slot order of 353 / 354 (MfmaSpec::slot_order; DESIGN.md "Slot order") and its image
            s->slot_tri.resize((size_t)n_tris);
            if (rt2_cluster_order_build(tris, n_tris, s->slot_tri.data(), &s->slot_table) < 0) return -1;
            if (build_slot_image(s) != 0) return -1;
        }
    }
    HIPCHECK(hipDeviceSynchronize());
    return 0;
}

// The slot image of a resident scene (rt2_k5_resident.h slot_image): the kt records of the triangles in the order
// s->slot_tri, s->slot_table, the prepared triangles in that order and slot_tri itself, in one allocation.  The
// finite-f16 check of the index image's records covers these too.
static int build_slot_image(rt2_scene* s) {
    const int n = s->n_tris, n_pad32 = (n + 31) / 32 * 32;
    if (n <= 0 || n_pad32 / 32 > kResGroups || !s->d_mfma_kt || (int)s->slot_tri.size() != n) return 0;
    const size_t kt_bytes = (size_t)n_pad32 * kKtOps * 16 * sizeof(_Float16), tab = sizeof(rt2_cluster_table);
    const size_t tri_bytes = (size_t)n * 3 * sizeof(float4);
    const size_t total = kt_bytes + tab + tri_bytes + (size_t)n * sizeof(int32_t);
    if (!s->d_slot) HIPCHECK(hipMalloc(&s->d_slot, total));
    char* base = reinterpret_cast<char*>(s->d_slot);
    std::vector<float4> tri((size_t)n * 3), perm((size_t)n * 3);
    HIPCHECK(hipMemcpy(tri.data(), s->d_tri, tri_bytes, hipMemcpyDeviceToHost));
    for (int k = 0; k < n; k++) std::copy_n(&tri[3 * (size_t)s->slot_tri[k]], 3, &perm[3 * (size_t)k]);
    HIPCHECK(hipMemcpy(base + kt_bytes, &s->slot_table, tab, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(base + kt_bytes + tab, perm.data(), tri_bytes, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(base + kt_bytes + tab + tri_bytes, s->slot_tri.data(), (size_t)n * sizeof(int32_t),
                       hipMemcpyHostToDevice));
    uint32_t* d_mflags = reinterpret_cast<uint32_t*>(s->d_counters + kCounters - 2);
    hipLaunchKernelGGL(prep_mfma_kt, dim3((n_pad32 + 255) / 256), dim3(256), 0, 0,
                       reinterpret_cast<const float4*>(base + kt_bytes + tab), n, n_pad32,
                       reinterpret_cast<_Float16*>(base), d_mflags);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipDeviceSynchronize());
    HIPCHECK(hipMemset(d_mflags, 0, 2 * sizeof(uint32_t)));
    if (s->mfma_ok) {
        std::vector<uint16_t> rec(kt_bytes / sizeof(uint16_t));
        HIPCHECK(hipMemcpy(rec.data(), base, kt_bytes, hipMemcpyDeviceToHost));
        for (uint16_t h : rec)
            if ((h & 0x7c00u) == 0x7c00u) s->mfma_ok = 0;
    }
    return 0;
}

// The 16x16x32 record layout (5 KiB per 16 triangles: the filter probe's
// layout 0 and rt2_scene_export), built on first use
// so that a product scene does not keep 320 B per triangle it never reads.
static int ensure_mfma16(rt2_scene* s) {
    if (s->d_mfma || s->n_tris <= 0) return 0;
    HIPCHECK(hipSetDevice(s->device));
    const int n_pad = (s->n_tris + 15) / 16 * 16;
    HIPCHECK(hipMalloc(&s->d_mfma, (size_t)n_pad * kMfmaQ * 32 * sizeof(_Float16)));
    HIPCHECK(hipMalloc(&s->d_mfma_tau, (size_t)n_pad * sizeof(float)));
    HIPCHECK(hipDeviceSynchronize());  // the scratch flags below are the counters' last two words
    uint32_t* d_mflags = reinterpret_cast<uint32_t*>(s->d_counters + kCounters - 2);
    HIPCHECK(hipMemset(d_mflags, 0, 2 * sizeof(uint32_t)));
    hipLaunchKernelGGL(prep_mfma, dim3((n_pad + 255) / 256), dim3(256), 0, 0, s->d_tri, s->n_tris, n_pad, s->d_mfma,
                       s->d_mfma_tau, d_mflags);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemset(d_mflags, 0, 2 * sizeof(uint32_t)));
    HIPCHECK(hipDeviceSynchronize());
    return 0;
}

extern "C" void rt2_scene_destroy(rt2_scene* s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    (void)hipFree(s->d_raw);
    (void)hipFree(s->d_tri);
    (void)hipFree(s->d_unit_n);
    (void)hipFree(s->d_mtl);
    (void)hipFree(s->d_mats);
    (void)hipFree(s->d_nodes);
    (void)hipFree(s->d_recs);
    (void)hipFree(s->d_plk);
    (void)hipFree(s->d_mfma);
    (void)hipFree(s->d_mfma_tau);
    (void)hipFree(s->d_mfma_k16);
    (void)hipFree(s->d_mfma_k16_tau);
    (void)hipFree(s->d_mfma_k16_bnd);
    (void)hipFree(s->d_mfma_kt);
    (void)hipFree(s->d_slot);
    if (s->last_launch) (void)hipEventDestroy(s->last_launch);
    (void)hipFree(s->d_texels);
    (void)hipFree(s->d_tex_desc);
    (void)hipFree(s->d_counters);
    for (const Staging* b : {&s->fb, &s->cost, &s->order, &s->hist, &s->region_ctr, &s->host_img[0], &s->host_img[1],
                             &s->host_img[2], &s->host_img[3], &s->stage_rays, &s->stage_rng, &s->stage_out})
        (void)hipFree(b->ptr);
    if (s->host_stream) (void)hipStreamDestroy(s->host_stream);
    delete s;
}

extern "C" int32_t rt2_shard_rows(int32_t height, rt2_shard sh) {
    if (sh.tile_rows < 1 || sh.nranks < 1 || sh.rank < 0 || sh.rank >= sh.nranks || height < 0) return -1;
    int32_t n = 0;
    for (int32_t t = sh.rank; (int64_t)t * sh.tile_rows < height; t += sh.nranks)
        n += std::min(sh.tile_rows, height - t * sh.tile_rows);
    return n;
}

extern "C" int32_t rt2_shard_row(int32_t local_row, rt2_shard sh) {
    int32_t t = local_row / sh.tile_rows;
    return (t * sh.nranks + sh.rank) * sh.tile_rows + local_row % sh.tile_rows;
}


namespace {
constexpr int kTileTris = 1024;  // 48 KiB of LDS per tile

// Kernel variants (rt2_scene_set_variant).  Ids are stable across builds: the
// product build carries the variants the launcher chooses automatically; the
// A/B experiments measured in DESIGN.md ("Tried and measured") are compiled
// only with -DRT2_EXPERIMENTS (make EXPERIMENTS=1).
enum Kind : int {
    K_TILED = 1, K_SMEM = 2, K_SPLIT = 3, K_ASSIST = 4, K_MFMA = 9,  // brute force
    K_BVH = 5, K_BVH2 = 6, K_BVH3 = 7, K_BVH4 = 8                                     // BVH (kind >= K_BVH)
};
struct Variant {
    int id;
    int kind;
    int block;
    hipError_t (*launch)(const RenderParams&, int blocks, size_t lds, hipStream_t st);
    void (*kernel)(RenderParams);
    const char* name;
    int max_groups = 0;  // largest scene the kernel holds, in 32-triangle groups (0 = no limit)
    bool slot = false;   // MfmaSpec::slot_order: RenderParams::mfma_kt_frag is the scene's slot image
};

// Linear twins (rt2_render_linear): variant id + kLinearTwin is the same kernel template on the same spec with
// `linear` set, i.e. the same schedule and sweeps with end_path_linear as the sink (rt2_path.h).
constexpr int kLinearTwin = 1000;
template <class Spec>
constexpr Spec lin(Spec x) {
    x.linear = true;
    return x;
}

template <auto K, int BLOCK>
hipError_t launch_k(const RenderParams& p, int blocks, size_t lds, hipStream_t st) {
    hipLaunchKernelGGL(K, dim3(blocks), dim3(BLOCK), lds, st, p);
    return hipGetLastError();
}
#define RT2_VARIANT(ID, KIND, KERNEL, BLOCK, NAME, ...) \
    Variant { ID, KIND, BLOCK, launch_k<KERNEL, BLOCK>, KERNEL, NAME __VA_OPT__(, ) __VA_ARGS__ }
// A product kernel and its linear twin, written once: TEMPLATE<SPEC> as ID and TEMPLATE<lin(SPEC)> as
// ID + kLinearTwin, with the parent's block, max_groups and slot flag and its name plus "/lin".
#define RT2_PRODUCT(ID, KIND, TEMPLATE, SPEC, BLOCK, NAME, ...)                  \
    RT2_VARIANT(ID, KIND, TEMPLATE<SPEC>, BLOCK, NAME __VA_OPT__(, ) __VA_ARGS__), \
        RT2_VARIANT(ID + kLinearTwin, KIND, TEMPLATE<lin(SPEC)>, BLOCK, NAME "/lin" __VA_OPT__(, ) __VA_ARGS__)

// product kernels
constexpr SmemSpec kSmemDefault{.block = 256, .group = 8, .filter = Filter::Max3, .tail = Tail::Coop,
                                .tail_lanes = 32, .waves = 6, .stats = false, .lockstep = true};
#ifdef RT2_EXPERIMENTS
constexpr SmemSpec kSmemMid{.block = 256, .group = 8, .filter = Filter::Max3, .tail = Tail::Coop, .tail_lanes = 32,
                            .waves = 1, .stats = false};
constexpr SplitSpec kSplitSmall{.waves_per_ray = 4, .group = 8, .filter = Filter::Max3, .waves = 6};
constexpr SmemSpec kSmemFree{.block = 256, .group = 8, .filter = Filter::Max3, .tail = Tail::Coop, .tail_lanes = 32,
                             .waves = 6, .stats = false, .lockstep = false};
constexpr AssistSpec assist12_x(int coop) {
    return AssistSpec{.waves_per_block = 12, .group = 8, .filter = Filter::Max3, .waves = 6, .coop_rays = coop};
}
#endif
constexpr TiledSpec kTiledLarge{.block = 512, .group = 4, .filter = Filter::Max3};
constexpr AssistSpec kAssist12{.waves_per_block = 12, .group = 8, .filter = Filter::Max3, .waves = 6, .coop_rays = 32};
// the 5-product form, every wave reading the records from L2 (rt2_mfma.h render_mfma)
constexpr MfmaSpec kMfmaK5{.block = 256, .waves = 3, .tail_lanes = 8};
// records resident in LDS (rt2_k5_resident.h): one 16-wave workgroup per CU, the lean lane state; l2 = the L2
// continuation (39..256 groups), fair = fair-share issue priority (rank slabs), lane_w = each ray's own W in the bound
constexpr MfmaSpec kt_res(bool l2, bool fair, bool lane_w, int phase_prio = 0, bool diag = false) {
    return MfmaSpec{.block = 1024, .waves = 4, .tail_lanes = 4, .diag = diag, .fair_prio = fair,
                    .phase_prio = phase_prio, .kt_lane_w = lane_w, .lean = true, .res_l2 = l2};
}
// ... with the exact phase once per window of `win` groups (rt2_k5_resident.h exact_window); skip_last: per group, but
// no Y rebuild after the last group
constexpr MfmaSpec kt_win(MfmaSpec x, int win, bool skip_last = false) {
    x.exact_win = win;
    x.y_skip_last = skip_last;
    return x;
}
#ifdef RT2_EXPERIMENTS
// ... with the Y product in the sweep's first window too (the A/B arms of MfmaSpec::y_first)
constexpr MfmaSpec kt_yw(MfmaSpec x) {
    x.y_first = true;
    return x;
}
#endif
// ... with the exact tests per ray (MfmaSpec::exact_lanes; rt2_k5_resident.h exact_window_lanes)
constexpr MfmaSpec kt_xl(MfmaSpec x) {
    x.exact_lanes = true;
    return x;
}
// ... with two groups per trip of the products' loop and the hot masks by v_writelane (MfmaSpec::pair_loop), and with
// the camera end point parked per pixel-frame (MfmaSpec::cam_park; kernels without the T1 pieces only)
constexpr MfmaSpec kt_pair(MfmaSpec x) {
    x.pair_loop = true;
    return x;
}
constexpr MfmaSpec kt_park(MfmaSpec x) {
    x.cam_park = true;
    return x;
}
// ... following the scene's cluster table: compact clusters swept with only the rays that need them
// (MfmaSpec::cluster_rows; DESIGN.md "Compact clusters")
constexpr MfmaSpec kt_cr(MfmaSpec x) {
    x.cluster_rows = true;
    return x;
}
// ... and a compact cluster that at most 16 rays need with 16-row products (MfmaSpec::cluster_rows16; DESIGN.md
// "16-row products")
constexpr MfmaSpec kt_cr16(MfmaSpec x) {
    x.cluster_rows = true;
    x.cluster_rows16 = true;
    return x;
}
// ... and a compact cluster that at most 8 rays need with 8-row products (MfmaSpec::cluster_rows8; DESIGN.md "8-row
// products")
constexpr MfmaSpec kt_cr8(MfmaSpec x) {
    x.cluster_rows8 = true;
    return x;
}
// ... on the scene's slot image: triangles regrouped by place, groups swept in slot order (MfmaSpec::slot_order;
// DESIGN.md "Slot order")
constexpr MfmaSpec kt_slot(MfmaSpec x) {
    x.slot_order = true;
    return x;
}
// ... its rounds' leftover pairs dealt out over all lanes (MfmaSpec::exact_spread; DESIGN.md "Leftover pairs on all
// lanes")
constexpr MfmaSpec kt_spread(MfmaSpec x) {
    x.exact_spread = true;
    return x;
}
constexpr int kResWin = 38;  // the window of 353-356 (and the diagnostic 350): the whole resident sweep, then one episode
constexpr int kResL2Groups = 256;  // render_mfma_k5r with res_l2: kResGroups groups resident, the rest from L2
// records streamed through LDS tiles (rt2_k5_tiles.h): 19-group tiles, each ray's own W, issue priority by
// finishing rank; 3 waves per SIMD
constexpr MfmaSpec kt_tiles_flow() {
    return MfmaSpec{.block = 768, .waves = 3, .tail_lanes = 0, .tile_groups = 19, .flow_prio = true, .kt_lane_w = true};
}
// ... at 4 waves per SIMD (1,024 threads) with the lean lane state (128 VGPRs, 1 spilled): the default
constexpr MfmaSpec kt_tiles_flow4() {
    MfmaSpec x = kt_tiles_flow();
    x.block = 1024;
    x.waves = 4;
    x.lean = true;
    return x;
}
// The shipped matrix-filter specs (353 .. 356, 380; the comments in kVariants).  The ray queries take the resident
// frame of 353 before its per-ray, pair-loop, cluster and slot pieces, and 355's as it is (kQueryRes, kQueryResL2).
constexpr MfmaSpec kResFrame = kt_win(kt_res(false, false, true, 4), kResWin);
constexpr MfmaSpec kResSlabFrame = kt_win(kt_res(false, true, true), kResWin);
constexpr MfmaSpec kt_product(MfmaSpec frame) {
    return kt_spread(kt_slot(kt_cr8(kt_cr16(kt_park(kt_pair(kt_xl(frame)))))));
}
constexpr MfmaSpec kRes = kt_product(kResFrame);
constexpr MfmaSpec kResSlab = kt_product(kResSlabFrame);
constexpr MfmaSpec kResL2 = kt_win(kt_res(true, false, true, 4), kResWin);
constexpr MfmaSpec kResL2Slab = kt_win(kt_res(true, true, true), kResWin);
constexpr MfmaSpec kTiles = kt_tiles_flow4();
constexpr Bvh3Spec kBvhDefault{.block = 256, .thresh = 16, .slab = Slab::Markstein, .waves = 5, .diag = false};

#ifdef RT2_EXPERIMENTS
constexpr SmemSpec smem_x(int g, Filter f, Tail t, int lanes, int w, bool stats = false) {
    return SmemSpec{.block = 256, .group = g, .filter = f, .tail = t, .tail_lanes = lanes, .waves = w, .stats = stats};
}
constexpr SplitSpec split_x(int s, Filter f, int w) {
    return SplitSpec{.waves_per_ray = s, .group = 8, .filter = f, .waves = w};
}
constexpr Bvh3Spec bvh3_x(int t, Slab sl, int w, bool diag = false) {
    return Bvh3Spec{.block = 256, .thresh = t, .slab = sl, .waves = w, .diag = diag};
}
#endif

constexpr Variant kVariants[] = {
    RT2_VARIANT(0, K_SMEM, render_smem<kSmemDefault>, 256, "smem/256/max3f8/coop32/w6/lockstep"),  // default (<= kSmemMaxTris)
    // every product kernel with its linear twin (kLinearTwin; 0's is 136's)
    RT2_PRODUCT(109, K_BVH4, render_bvh4, kBvhDefault, 256, "bvh4/256/t16/w5"),           // default (BVH traversal)
    RT2_PRODUCT(86, K_TILED, render_tiled, kTiledLarge, 512, "tiled/512/max3f4"),          // > kSmemMaxTris
    RT2_PRODUCT(92, K_ASSIST, render_assist, kAssist12, 768, "assist12/max3f8/w6"),        // < 4 items per lane
    RT2_PRODUCT(136, K_SMEM, render_smem, kSmemDefault, 256, "smem/256/max3f8/coop32/w6/lockstep"),  // variant 0 forced (id 0 = automatic)
    // the matrix filter with every wave reading the records from L2 (DESIGN.md "The 5-product form"): U, -V, X from
    // the first K-half, the left-out m.z slots bounded in the threshold; 3 waves per SIMD
    RT2_PRODUCT(227, K_MFMA, render_mfma, kMfmaK5, 256, "mfma/256/k5/coop8/w3/imax/minred/ymma/t12/llds/ser4/cmp"),
    // scenes of <= 256 groups (8,192 triangles; config B: 38, W: 57, K: 89): the resident kernel (rt2_k5_resident.h:
    // records in LDS for the whole launch, 38 groups, the rest read from L2) with the threshold in the K-slots
    // (DESIGN.md "The threshold in the K-slots"), each ray's own W, issue priority by phase; fair-share issue
    // priority instead for rank slabs; the exact phase once per window of kResWin groups, the first window of a sweep
    // without the Y product (DESIGN.md "No Y product without a bound"); 353 / 354 run the exact tests per ray
    // (DESIGN.md "Exact tests per ray"), two groups per trip of the products' loop with the hot masks by v_writelane
    // (DESIGN.md "Two groups per loop trip") and keep each pixel's camera end point in LDS instead of recomputing it
    // per ray (DESIGN.md "The camera end point once per pixel")
    // and sweep the scene's slot image (DESIGN.md "Slot order"), a compact cluster that at most 8 rays need with 8-row
    // products (DESIGN.md "8-row products"), and deal a round's leftover exact pairs out over all 64 lanes (DESIGN.md
    // "Leftover pairs on all lanes")
    RT2_PRODUCT(353, K_MFMA, render_mfma_k5r, kRes, 1024, "mfmar/1024/kt4/res38/coop4/w4/cmp/dpp/lean/lw/pp4", kResGroups, true),
    RT2_PRODUCT(354, K_MFMA, render_mfma_k5r, kResSlab, 1024, "mfmar/1024/kt4/res38/coop4/w4/cmp/fair/dpp/lean/lw", kResGroups, true),
    RT2_PRODUCT(355, K_MFMA, render_mfma_k5r, kResL2, 1024, "mfmarl2/1024/kt4/res38l2/coop4/w4/cmp/dpp/lean/lw/pp4", kResL2Groups),
    RT2_PRODUCT(356, K_MFMA, render_mfma_k5r, kResL2Slab, 1024, "mfmarl2/1024/kt4/res38l2/coop4/w4/cmp/fair/dpp/lean/lw", kResL2Groups),
    // the default above 8,192 triangles: the LDS-tiled kernel (rt2_k5_tiles.h; 19-group tiles, fragments in
    // registers) with the threshold in the K-slots, each ray's own W in the bound
    RT2_PRODUCT(380, K_MFMA, render_mfma_k5t, kTiles, 1024, "mfmat5/1024/kt4/tile19/coop0/w4/cmp/regs/perm/lw/flowp/lean"),
#ifdef RT2_EXPERIMENTS
    // One knob away from a shipping matrix-filter kernel, plus one diagnostic build per template (DESIGN.md "Tried
    // and measured"; earlier generations are in git history).
    // the resident kernel with the wave's W in the bound (353-356 take each ray's own)
    RT2_VARIANT(342, K_MFMA, render_mfma_k5r<kt_win(kt_res(false, false, false), kResWin)>, 1024, "mfmar/1024/kt4/res38/coop4/w4/cmp/dpp/lean", kResGroups),
    RT2_VARIANT(344, K_MFMA, render_mfma_k5r<kt_win(kt_res(false, true, false), kResWin)>, 1024, "mfmar/1024/kt4/res38/coop4/w4/cmp/fair/dpp/lean", kResGroups),
    RT2_VARIANT(345, K_MFMA, render_mfma_k5r<kt_win(kt_res(true, false, false), kResWin)>, 1024, "mfmarl2/1024/kt4/res38l2/coop4/w4/cmp/dpp/lean", kResL2Groups),
    RT2_VARIANT(346, K_MFMA, render_mfma_k5r<kt_win(kt_res(true, true, false), kResWin)>, 1024, "mfmarl2/1024/kt4/res38l2/coop4/w4/cmp/fair/dpp/lean", kResL2Groups),
    // ... issue priority by phase 1 / 2 / 3 (353 takes 4) and without it; its diagnostic counters
    RT2_VARIANT(387, K_MFMA, render_mfma_k5r<kt_win(kt_res(false, false, true, 1), kResWin)>, 1024, "mfmar/1024/kt4/res38/coop4/w4/cmp/dpp/lean/lw/pp1", kResGroups),
    RT2_VARIANT(388, K_MFMA, render_mfma_k5r<kt_win(kt_res(false, false, true, 2), kResWin)>, 1024, "mfmar/1024/kt4/res38/coop4/w4/cmp/dpp/lean/lw/pp2", kResGroups),
    RT2_VARIANT(389, K_MFMA, render_mfma_k5r<kt_win(kt_res(false, false, true, 3), kResWin)>, 1024, "mfmar/1024/kt4/res38/coop4/w4/cmp/dpp/lean/lw/pp3", kResGroups),
    RT2_VARIANT(391, K_MFMA, render_mfma_k5r<kt_win(kt_res(false, false, true), kResWin)>, 1024, "mfmar/1024/kt4/res38/coop4/w4/cmp/dpp/lean/lw", kResGroups),
    RT2_VARIANT(350, K_MFMA, render_mfma_k5r<kt_win(kt_res(false, false, true, 0, true), kResWin)>, 1024, "mfmar/1024/kt4/res38/coop4/w4/cmp/diag/dpp/lean/lw", kResGroups),
    // ... its per-group form with the same clocks
    RT2_VARIANT(390, K_MFMA, render_mfma_k5r<kt_win(kt_res(false, false, true, 0, true), 1)>, 1024, "mfmar/1024/kt4/res38/coop4/w4/cmp/diag/dpp/lean/lw/xw1", kResGroups),
    // the exact phase per window of W groups (353-356 take kResWin = 38): per group (xw1: the form before the window),
    // per group without the Y rebuild after the last group (xw1s), W = 2, 4, 8, 19; the L2 continuation's and the
    // fair-share kernel's per-group forms
    RT2_VARIANT(392, K_MFMA, render_mfma_k5r<kt_win(kt_res(false, false, true, 4), 1)>, 1024, "mfmar/1024/kt4/res38/coop4/w4/cmp/dpp/lean/lw/pp4/xw1", kResGroups),
    RT2_VARIANT(393, K_MFMA, render_mfma_k5r<kt_win(kt_res(false, false, true, 4), 1, true)>, 1024, "mfmar/1024/kt4/res38/coop4/w4/cmp/dpp/lean/lw/pp4/xw1s", kResGroups),
    RT2_VARIANT(394, K_MFMA, render_mfma_k5r<kt_win(kt_res(false, false, true, 4), 2)>, 1024, "mfmar/1024/kt4/res38/coop4/w4/cmp/dpp/lean/lw/pp4/xw2", kResGroups),
    RT2_VARIANT(395, K_MFMA, render_mfma_k5r<kt_win(kt_res(false, false, true, 4), 4)>, 1024, "mfmar/1024/kt4/res38/coop4/w4/cmp/dpp/lean/lw/pp4/xw4", kResGroups),
    RT2_VARIANT(396, K_MFMA, render_mfma_k5r<kt_win(kt_res(false, false, true, 4), 8)>, 1024, "mfmar/1024/kt4/res38/coop4/w4/cmp/dpp/lean/lw/pp4/xw8", kResGroups),
    RT2_VARIANT(399, K_MFMA, render_mfma_k5r<kt_win(kt_res(false, false, true, 4), 19)>, 1024, "mfmar/1024/kt4/res38/coop4/w4/cmp/dpp/lean/lw/pp4/xw19", kResGroups),
    RT2_VARIANT(397, K_MFMA, render_mfma_k5r<kt_win(kt_res(true, false, true, 4), 1)>, 1024, "mfmarl2/1024/kt4/res38l2/coop4/w4/cmp/dpp/lean/lw/pp4/xw1", kResL2Groups),
    RT2_VARIANT(398, K_MFMA, render_mfma_k5r<kt_win(kt_res(false, true, true), 1)>, 1024, "mfmar/1024/kt4/res38/coop4/w4/cmp/fair/dpp/lean/lw/xw1", kResGroups),
    // the Y product in a sweep's first window too (yw: the form before MfmaSpec::y_first; 353, 355 and 350 leave it out)
    RT2_VARIANT(351, K_MFMA, render_mfma_k5r<kt_yw(kt_win(kt_res(false, false, true, 4), kResWin))>, 1024, "mfmar/1024/kt4/res38/coop4/w4/cmp/dpp/lean/lw/pp4/yw", kResGroups),
    RT2_VARIANT(352, K_MFMA, render_mfma_k5r<kt_yw(kt_win(kt_res(true, false, true, 4), kResWin))>, 1024, "mfmarl2/1024/kt4/res38l2/coop4/w4/cmp/dpp/lean/lw/pp4/yw", kResL2Groups),
    RT2_VARIANT(357, K_MFMA, render_mfma_k5r<kt_yw(kt_win(kt_res(false, false, true, 0, true), kResWin))>, 1024, "mfmar/1024/kt4/res38/coop4/w4/cmp/diag/dpp/lean/lw/yw", kResGroups),
    // the exact tests per ray from a compacted hot-triangle pass (MfmaSpec::exact_lanes; 353 / 354 take it): the
    // wave-wide episode on 353's and 354's spec (xwave: the form before), the per-ray one on 355's, 350's and 356's (xl)
    RT2_VARIANT(400, K_MFMA, render_mfma_k5r<kt_win(kt_res(false, false, true, 4), kResWin)>, 1024, "mfmar/1024/kt4/res38/coop4/w4/cmp/dpp/lean/lw/pp4/xwave", kResGroups),
    RT2_VARIANT(401, K_MFMA, render_mfma_k5r<kt_xl(kt_win(kt_res(true, false, true, 4), kResWin))>, 1024, "mfmarl2/1024/kt4/res38l2/coop4/w4/cmp/dpp/lean/lw/pp4/xl", kResL2Groups),
    RT2_VARIANT(402, K_MFMA, render_mfma_k5r<kt_xl(kt_win(kt_res(false, false, true, 0, true), kResWin))>, 1024, "mfmar/1024/kt4/res38/coop4/w4/cmp/diag/dpp/lean/lw/xl", kResGroups),
    RT2_VARIANT(403, K_MFMA, render_mfma_k5r<kt_win(kt_res(false, true, true), kResWin)>, 1024, "mfmar/1024/kt4/res38/coop4/w4/cmp/fair/dpp/lean/lw/xwave", kResGroups),
    RT2_VARIANT(404, K_MFMA, render_mfma_k5r<kt_xl(kt_win(kt_res(true, true, true), kResWin))>, 1024, "mfmarl2/1024/kt4/res38l2/coop4/w4/cmp/fair/dpp/lean/lw/xl", kResL2Groups),
    // two groups per loop trip with the masks by v_writelane, and the parked camera end point (MfmaSpec::pair_loop,
    // cam_park; 353 / 354 take both): 353's spec with neither (the form before), with pair_loop only, with cam_park
    // only; 354's with neither
    RT2_VARIANT(405, K_MFMA, render_mfma_k5r<kt_xl(kt_win(kt_res(false, false, true, 4), kResWin))>, 1024, "mfmar/1024/kt4/res38/coop4/w4/cmp/dpp/lean/lw/pp4/nopair/nopark", kResGroups),
    RT2_VARIANT(406, K_MFMA, render_mfma_k5r<kt_pair(kt_xl(kt_win(kt_res(false, false, true, 4), kResWin)))>, 1024, "mfmar/1024/kt4/res38/coop4/w4/cmp/dpp/lean/lw/pp4/nopark", kResGroups),
    RT2_VARIANT(407, K_MFMA, render_mfma_k5r<kt_park(kt_xl(kt_win(kt_res(false, false, true, 4), kResWin)))>, 1024, "mfmar/1024/kt4/res38/coop4/w4/cmp/dpp/lean/lw/pp4/nopair", kResGroups),
    RT2_VARIANT(408, K_MFMA, render_mfma_k5r<kt_xl(kt_win(kt_res(false, true, true), kResWin))>, 1024, "mfmar/1024/kt4/res38/coop4/w4/cmp/fair/dpp/lean/lw/nopair/nopark", kResGroups),
    // the cluster table followed (MfmaSpec::cluster_rows; 353 / 354 take it): 353's and 354's specs without it (nocr:
    // the form before), and the diagnostic build that counts the skipped / one-block / two-block cases
    RT2_VARIANT(409, K_MFMA, render_mfma_k5r<kt_park(kt_pair(kt_xl(kt_win(kt_res(false, false, true, 4), kResWin))))>, 1024, "mfmar/1024/kt4/res38/coop4/w4/cmp/dpp/lean/lw/pp4/nocr", kResGroups),
    RT2_VARIANT(410, K_MFMA, render_mfma_k5r<kt_park(kt_pair(kt_xl(kt_win(kt_res(false, true, true), kResWin))))>, 1024, "mfmar/1024/kt4/res38/coop4/w4/cmp/fair/dpp/lean/lw/nocr", kResGroups),
    RT2_VARIANT(411, K_MFMA, render_mfma_k5r<kt_cr16(kt_pair(kt_xl(kt_win(kt_res(false, false, true, 0, true), kResWin))))>, 1024, "mfmar/1024/kt4/res38/coop4/w4/cmp/diag/dpp/lean/lw/xl/cr16", kResGroups),
    // the 16-row products for clusters that at most 16 rays need (MfmaSpec::cluster_rows16; 353 / 354 and the
    // diagnostic 411 take it): 353's and 354's specs with the cluster table alone (cr32: the form before)
    RT2_VARIANT(412, K_MFMA, render_mfma_k5r<kt_cr(kt_park(kt_pair(kt_xl(kt_win(kt_res(false, false, true, 4), kResWin)))))>, 1024, "mfmar/1024/kt4/res38/coop4/w4/cmp/dpp/lean/lw/pp4/cr32", kResGroups),
    RT2_VARIANT(413, K_MFMA, render_mfma_k5r<kt_cr(kt_park(kt_pair(kt_xl(kt_win(kt_res(false, true, true), kResWin)))))>, 1024, "mfmar/1024/kt4/res38/coop4/w4/cmp/fair/dpp/lean/lw/cr32", kResGroups),
    // the slot image (MfmaSpec::slot_order; 353 / 354 take it): 353's and 354's specs on the index image (idx: the form
    // before), and 411's counters on the slot image
    RT2_VARIANT(414, K_MFMA, render_mfma_k5r<kt_cr16(kt_park(kt_pair(kt_xl(kt_win(kt_res(false, false, true, 4), kResWin)))))>, 1024, "mfmar/1024/kt4/res38/coop4/w4/cmp/dpp/lean/lw/pp4/idx", kResGroups),
    RT2_VARIANT(415, K_MFMA, render_mfma_k5r<kt_cr16(kt_park(kt_pair(kt_xl(kt_win(kt_res(false, true, true), kResWin)))))>, 1024, "mfmar/1024/kt4/res38/coop4/w4/cmp/fair/dpp/lean/lw/idx", kResGroups),
    RT2_VARIANT(416, K_MFMA, render_mfma_k5r<kt_slot(kt_cr16(kt_pair(kt_xl(kt_win(kt_res(false, false, true, 0, true), kResWin)))))>, 1024, "mfmar/1024/kt4/res38/coop4/w4/cmp/diag/dpp/lean/lw/xl/cr16/slot", kResGroups, true),
    // the 8-row products for clusters that at most 8 rays need (MfmaSpec::cluster_rows8; 353 / 354 take it): 353's and
    // 354's specs with the 16-row products alone (r16: the form before), and 416's counters with the 8-row count
    RT2_VARIANT(417, K_MFMA, render_mfma_k5r<kt_slot(kt_cr16(kt_park(kt_pair(kt_xl(kt_win(kt_res(false, false, true, 4), kResWin))))))>, 1024, "mfmar/1024/kt4/res38/coop4/w4/cmp/dpp/lean/lw/pp4/r16", kResGroups, true),
    RT2_VARIANT(418, K_MFMA, render_mfma_k5r<kt_slot(kt_cr16(kt_park(kt_pair(kt_xl(kt_win(kt_res(false, true, true), kResWin))))))>, 1024, "mfmar/1024/kt4/res38/coop4/w4/cmp/fair/dpp/lean/lw/r16", kResGroups, true),
    RT2_VARIANT(419, K_MFMA, render_mfma_k5r<kt_slot(kt_cr8(kt_cr16(kt_pair(kt_xl(kt_win(kt_res(false, false, true, 0, true), kResWin))))))>, 1024, "mfmar/1024/kt4/res38/coop4/w4/cmp/diag/dpp/lean/lw/xl/cr8/slot", kResGroups, true),
    // a round's leftover pairs on all lanes (MfmaSpec::exact_spread; 353 / 354 take it): 353's and 354's specs with the
    // per-lane loop alone (loop: the form before), 419's counters with the spread path and its three, and the tests'
    // negative control (drop: a spread round's last list entry is not tested; its image is wrong on purpose)
    RT2_VARIANT(420, K_MFMA, render_mfma_k5r<kt_slot(kt_cr8(kt_cr16(kt_park(kt_pair(kt_xl(kResFrame))))))>, 1024, "mfmar/1024/kt4/res38/coop4/w4/cmp/dpp/lean/lw/pp4/loop", kResGroups, true),
    RT2_VARIANT(421, K_MFMA, render_mfma_k5r<kt_slot(kt_cr8(kt_cr16(kt_park(kt_pair(kt_xl(kResSlabFrame))))))>, 1024, "mfmar/1024/kt4/res38/coop4/w4/cmp/fair/dpp/lean/lw/loop", kResGroups, true),
    RT2_VARIANT(422, K_MFMA, render_mfma_k5r<kt_spread(kt_slot(kt_cr8(kt_cr16(kt_pair(kt_xl(kt_win(kt_res(false, false, true, 0, true), kResWin)))))))>, 1024, "mfmar/1024/kt4/res38/coop4/w4/cmp/diag/dpp/lean/lw/xl/cr8/slot/spread", kResGroups, true),
    RT2_VARIANT(423, K_MFMA, render_mfma_k5r<[] { MfmaSpec x = kRes; x.spread_drop = true; return x; }()>, 1024, "mfmar/1024/kt4/res38/coop4/w4/cmp/dpp/lean/lw/pp4/drop", kResGroups, true),
    // the tile stream at 3 waves per SIMD (380 takes 4 with the lean lane state): with its diagnostic clocks; without
    // flow_prio; with the lean lane state
    RT2_VARIANT(370, K_MFMA, render_mfma_k5t<kt_tiles_flow()>, 768, "mfmat5/768/kt4/tile19/coop0/w3/cmp/regs/perm/lw/flowp"),
    RT2_VARIANT(368, K_MFMA, render_mfma_k5t<[] { MfmaSpec x = kt_tiles_flow(); x.diag = true; return x; }()>, 768, "mfmat5/768/kt4/tile19/coop0/w3/cmp/regs/perm/lw/flowp/diag"),
    RT2_VARIANT(369, K_MFMA, render_mfma_k5t<[] { MfmaSpec x = kt_tiles_flow(); x.flow_prio = false; return x; }()>, 768, "mfmat5/768/kt4/tile19/coop0/w3/cmp/regs/perm/lw/flow"),
    RT2_VARIANT(382, K_MFMA, render_mfma_k5t<[] { MfmaSpec x = kt_tiles_flow(); x.lean = true; return x; }()>, 768, "mfmat5/768/kt4/tile19/coop0/w3/cmp/regs/perm/lw/flowp/lean"),
    // ... 380 with 16-group tiles; without flow_prio; with the cooperative drain at 4
    RT2_VARIANT(381, K_MFMA, render_mfma_k5t<[] { MfmaSpec x = kt_tiles_flow4(); x.tile_groups = 16; return x; }()>, 1024, "mfmat5/1024/kt4/tile16/coop0/w4/cmp/regs/perm/lw/flowp/lean"),
    RT2_VARIANT(385, K_MFMA, render_mfma_k5t<[] { MfmaSpec x = kt_tiles_flow4(); x.flow_prio = false; return x; }()>, 1024, "mfmat5/1024/kt4/tile19/coop0/w4/cmp/regs/perm/lw/flow/lean"),
    RT2_VARIANT(386, K_MFMA, render_mfma_k5t<[] { MfmaSpec x = kt_tiles_flow4(); x.tail_lanes = 4; return x; }()>, 1024, "mfmat5/1024/kt4/tile19/coop4/w4/cmp/regs/perm/lw/flowp/lean"),
    // scalar-path and BVH kernels of rounds 1-2 (DESIGN.md "Tried and measured"; parity-tested in the experiment build)
    RT2_VARIANT(67, K_SMEM, render_smem<kSmemMid>, 256, "smem/256/max3f8/coop32"),         // round-1 choice, 1-4 items per lane
    RT2_VARIANT(85, K_SPLIT, render_split<kSplitSmall>, 256, "split4/max3f8/w6"),          // round-1 choice, < 1 item per lane
    RT2_VARIANT(53, K_BVH3, render_bvh3<kBvhDefault>, 256, "bvh3/256/t16/w5"),            // round-1/2 BVH default
    RT2_VARIANT(106, K_SMEM, render_smem<kSmemFree>, 256, "smem/256/max3f8/coop32/w6/free"),  // round-1 default
    RT2_VARIANT(37, K_BVH, render_bvh<BvhSpec{256}>, 256, "bvh/256"),
    RT2_VARIANT(40, K_BVH2, (render_bvh2<Bvh2Spec{256, 16}>), 256, "bvh2/256/t16"),
    RT2_VARIANT(41, K_BVH2, (render_bvh2<Bvh2Spec{256, 8}>), 256, "bvh2/256/t8"),
    RT2_VARIANT(43, K_BVH2, (render_bvh2<Bvh2Spec{128, 16}>), 128, "bvh2/128/t16"),
    RT2_VARIANT(45, K_BVH2, (render_bvh2<Bvh2Spec{256, 1}>), 256, "bvh2/256/t1"),
    RT2_VARIANT(46, K_BVH3, render_bvh3<bvh3_x(16, Slab::Markstein, 1)>, 256, "bvh3/256/t16"),
    RT2_VARIANT(47, K_BVH3, render_bvh3<bvh3_x(8, Slab::Markstein, 1)>, 256, "bvh3/256/t8"),
    RT2_VARIANT(48, K_BVH3, render_bvh3<bvh3_x(24, Slab::Markstein, 1)>, 256, "bvh3/256/t24"),
    RT2_VARIANT(50, K_BVH3, render_bvh3<bvh3_x(16, Slab::Binary64, 1)>, 256, "bvh3/256/t16/div64"),
    RT2_VARIANT(54, K_BVH3, render_bvh3<bvh3_x(8, Slab::Markstein, 5)>, 256, "bvh3/256/t8/w5"),
    RT2_VARIANT(55, K_BVH3, render_bvh3<bvh3_x(16, Slab::Filtered, 5)>, 256, "bvh3/256/t16/filt/w5"),
    RT2_VARIANT(58, K_BVH3, render_bvh3<bvh3_x(16, Slab::Markstein, 5, true)>, 256, "bvh3/256/t16/w5/DIAG"),
    RT2_VARIANT(64, K_SMEM, render_smem<smem_x(8, Filter::Five, Tail::Team, 32, 1)>, 256, "smem/256/masked8/team32"),
    RT2_VARIANT(66, K_SMEM, render_smem<smem_x(8, Filter::Five, Tail::Team, 64, 1)>, 256, "smem/256/masked8/team64"),
    RT2_VARIANT(74, K_SMEM, render_smem<smem_x(4, Filter::Plk, Tail::Coop, 32, 1)>, 256, "smem/256/plk4/coop32"),
    RT2_VARIANT(76, K_SMEM, render_smem<smem_x(8, Filter::Plk, Tail::Coop, 32, 1)>, 256, "smem/256/plk8/coop32"),
    RT2_VARIANT(79, K_SMEM, render_smem<smem_x(8, Filter::Plk, Tail::Coop, 32, 6)>, 256, "smem/256/plk8/coop32/w6"),
    RT2_VARIANT(80, K_SMEM, render_smem<smem_x(2, Filter::Plk, Tail::Coop, 32, 1)>, 256, "smem/256/plk2/coop32"),
    RT2_VARIANT(82, K_SMEM, render_smem<smem_x(8, Filter::Max3, Tail::Coop, 32, 1, true)>, 256,
                "smem/256/max3f8/coop32/STATS"),
#endif
};
constexpr bool variant_ids_unique() {
    for (const Variant& a : kVariants)
        for (const Variant& b : kVariants)
            if (&a != &b && a.id == b.id) return false;
    return true;
}
static_assert(variant_ids_unique(), "two entries of kVariants share an id");

constexpr int kSmemMaxTris = 131072;  // scalar path up to 6.3 MB of records (config C: 781 vs 817 ms tiled; config E: tiled 1,704 vs 2,312 ms)
constexpr int kDefaultBrute = 0;
constexpr int kDefaultBvh = 109;
constexpr int kLargeScene = 86;  // tiled/512/max3f4: LDS tiles above kSmemMaxTris triangles
constexpr int kSlab = 92;        // assist12/max3f8/w6: fewer than 4 items per lane (multi-GPU slabs)
// the matrix filter (scenes inside its range; DESIGN.md "The threshold in the K-slots", "LDS record tiles")
constexpr int kMfmaSlabMaxTris = 8192;  // = kResL2Groups x 32: the resident kernel with its L2 continuation
constexpr int kMfmaRes = 353;      // <= kResGroups groups (config B): every record resident in LDS
constexpr int kMfmaResSlab = 354;  // ... launches with < kResSlabItems items per resident lane (rank slabs):
                                   // fair-share issue priority
constexpr unsigned long long kResSlabItems = 6;
constexpr int kMfmaResL2 = 355;    // 39..256 groups (configs W, K): kResGroups groups resident, the rest read from L2
constexpr int kMfmaResL2Slab = 356;  // ... its rank slabs
constexpr int kMfmaTiles = 380;    // larger scenes: the records streamed through LDS tiles, one 16-wave workgroup per CU
constexpr int kMfma = 227;         // every wave reads the records from L2; taken when kMfmaTiles is not in the build

constexpr bool is_bvh(int kind) { return kind >= K_BVH && kind <= K_BVH4; }

const Variant* find_variant(int id) {
    for (const Variant& v : kVariants)
        if (v.id == id) return &v;
    return nullptr;
}
// The twin rt2_render_linear launches in place of v (null: v has none); the automatic id 0 is 136's kernel.
const Variant* linear_twin(const Variant& v) { return find_variant(kLinearTwin + (v.id == 0 ? 136 : v.id)); }
hipError_t variant_occupancy(const Variant& v, int* occ, size_t lds) {
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(occ, reinterpret_cast<const void*>(v.kernel), v.block, lds);
}
}  // namespace

extern "C" int rt2_scene_set_variant(rt2_scene* s, int variant) {
    if (!s) {
        rt2h::set_error("rt2_scene_set_variant: null scene");
        return -1;
    }
    if (variant != 0 && !find_variant(variant)) {
        rt2h::set_error("rt2_scene_set_variant: variant " + std::to_string(variant) +
                        " is not in this build (experiment variants need make EXPERIMENTS=1)");
        return -1;
    }
    if (variant >= kLinearTwin) {
        rt2h::set_error("rt2_scene_set_variant: variant " + std::to_string(variant) +
                        " is a linear twin: set its parent, rt2_render_linear launches the twin");
        return -1;
    }
    s->variant = variant;
    return variant;
}

extern "C" const char* rt2_variant_name(int v) {
    const Variant* V = find_variant(v);
    return V ? V->name : nullptr;
}

// Not in rt2.h (diagnostics): the occupancy API's blocks per CU and the
// kernel's register counts (hipFuncGetAttributes) for variant v.
extern "C" int rt2_variant_occupancy(int v, int* api_blocks, int* num_regs, int* local_bytes) {
    const Variant* V = find_variant(v);
    if (!V) return -1;
    int occ = 0;
    HIPCHECK(variant_occupancy(*V, &occ, 0));
    hipFuncAttributes a;
    HIPCHECK(hipFuncGetAttributes(&a, reinterpret_cast<const void*>(V->kernel)));
    if (api_blocks) *api_blocks = occ;
    if (num_regs) *num_regs = a.numRegs;
    if (local_bytes) *local_bytes = (int)a.localSizeBytes;
    return 0;
}

/* -------------------------------------------------------------------------
 * What every launch shares (renders and ray queries): the scene's RenderParams, the scratch, the launch order
 * ----------------------------------------------------------------------- */
namespace {
// Grows one of the scene's buffers to `bytes`.  `drain`: the stream whose work may still use the old buffer, drained
// before it is freed (the blocking wrappers' host_stream).  Null for the scratch a launch grows on its caller's
// stream: there hipFree's own device synchronisation is the wait.
int staging_grow(Staging& b, size_t bytes, const hipStream_t* drain = nullptr) {
    if (bytes <= b.cap) return 0;
    if (drain) HIPCHECK(hipStreamSynchronize(*drain));
    (void)hipFree(b.ptr);
    b.ptr = nullptr;
    b.cap = 0;
    HIPCHECK(hipMalloc(&b.ptr, bytes));
    b.cap = bytes;
    return 0;
}

// What every launch's search reads.
RenderParams scene_params(const rt2_scene* s) {
    RenderParams p;
    std::memset(&p, 0, sizeof(p));
    p.tri = s->d_tri;
    p.n_tris = s->n_tris;
    p.mfma_A = s->mfma_A;
    p.mfma_kt_frag = s->d_mfma_kt;
    p.nodes = s->d_nodes;
    p.stack_slots = s->bvh_depth + 2;
    p.item_counter = s->d_counters;
    p.seg_counter = s->d_counters + 1;
    return p;
}

// ... and what the shaders read of the materials and textures (the renders, surface_record, shade_step and
// radiance_step).
void scene_shading_params(const rt2_scene* s, RenderParams& p) {
    p.unit_n = s->d_unit_n;
    p.tri_mtl = s->d_mtl;
    p.mats = s->d_mats;
    p.n_mats = s->n_mats;
    p.raw = s->d_raw;
    p.texels = s->d_texels;
    p.tex_desc = s->d_tex_desc;
    p.n_tex = s->n_tex;
    p.num_textures = std::min(s->n_tex, 5);  // a ray query has no uniforms: the images bound, at most the five units
}

void copy3(float* d, const rt2_vec4& v) {
    d[0] = v.x;
    d[1] = v.y;
    d[2] = v.z;
}

// Launches of one scene share its counters and scratch (frame planes, cost map, pixel order): a launch waits for
// the scene's previous one, whatever stream that was issued on ...
int launch_begin(rt2_scene* s, hipStream_t st) {
    if (s->last_launch_valid) HIPCHECK(hipStreamWaitEvent(st, s->last_launch, 0));
    return 0;
}
// ... and leaves the event the next one waits on.
int launch_end(rt2_scene* s, hipStream_t st) {
    if (!s->last_launch) HIPCHECK(hipEventCreateWithFlags(&s->last_launch, hipEventDisableTiming));
    HIPCHECK(hipEventRecord(s->last_launch, st));
    s->last_launch_valid = true;
    s->tests_per_seg = (unsigned long long)s->n_tris;
    return 0;
}
}  // namespace

/* -------------------------------------------------------------------------
 * The render launcher (DESIGN.md "The render launcher"): render_launch and its steps, in the order they run
 * ----------------------------------------------------------------------- */
namespace {
// A render's RenderParams: the scene's, the uniforms' view and image, the shard's slab.
RenderParams render_params(const rt2_scene* s, const rt2_uniforms* u, uint32_t frame_begin, uint32_t frame_count,
                           rt2_shard sh, int rows) {
    RenderParams p = scene_params(s);
    scene_shading_params(s, p);
    p.num_textures = u->numTextures;
    p.plk = s->plk_ok ? s->d_plk : nullptr;
    p.plk_A = s->plk_A;
    p.mfma_k16_frag = s->d_mfma_k16;
    p.mfma_k16_tau = s->d_mfma_k16_tau;
    p.mfma_k16_bnd = s->d_mfma_k16_bnd;
    p.wave_log = s->wave_log;
    p.wave_log_n = s->wave_log_n;
    p.tile_tris = kTileTris;
    p.W = (int)u->width;
    p.H = (int)u->height;
    p.maxBounce = u->maxBounceCount;
    p.R = u->numRaysPerPixel;
    p.envLight = u->environmentalLight;
    copy3(p.cam, u->cameraPos);
    copy3(p.vpRight, u->viewportRight);
    copy3(p.vpUp, u->viewportUp);
    copy3(p.vpFront, u->viewportFront);
    copy3(p.pixR, u->pixelRight);
    copy3(p.pixU, u->pixelUp);
    copy3(p.defR, u->defocusDiskRight);
    copy3(p.defU, u->defocusDiskUp);
    p.frame_begin = frame_begin;
    p.frame_count = frame_count;
    p.tile_rows = sh.tile_rows;
    p.rank = sh.rank;
    p.nranks = sh.nranks;
    p.n_pix = (unsigned long long)rows * (unsigned long long)p.W;
    p.n_items = p.n_pix;
    return p;
}

// The counters a render starts from: items, the 8 item regions, the diagnostic wave ends.
int counters_reset(rt2_scene* s, RenderParams& p, hipStream_t st) {
    HIPCHECK(hipMemsetAsync(s->d_counters, 0, sizeof(unsigned long long), st));
    // items in 8 contiguous regions, one per group of workgroups sharing an
    // XCD's L2 (blockIdx % 8): neighbouring pixels' rays walk the same BVH
    // lines in one L2 (config C BVH: 2,701 vs 2,783 ms; brute force ±0)
    if (staging_grow(s->region_ctr, 8 * 128) != 0) return -1;
    HIPCHECK(hipMemsetAsync(s->region_ctr.ptr, 0, 8 * 128, st));
    p.region_ctr = s->region_ctr.as<unsigned long long>();
    HIPCHECK(hipMemsetAsync(s->d_counters + 6, 0xff, sizeof(unsigned long long), st));  // diag: min wave end
    HIPCHECK(hipMemsetAsync(s->d_counters + 7, 0, sizeof(unsigned long long), st));     // diag: max wave end
    return 0;
}

// The traceBasic preview: one thread per pixel, every frame the same image.
int launch_basic(rt2_scene* s, const rt2_uniforms* u, RenderParams& p, uint32_t frame_count, hipStream_t st) {
    p.basicShadow = u->basicShadingShadow;
    copy3(p.light, u->basicShadingLightPosition);
    constexpr int kBasicBlock = 256;
    const unsigned long long blocks = (p.n_items + kBasicBlock - 1) / kBasicBlock;
    if (s->traversal == RT2_TRAVERSAL_BVH) {
        const size_t lds = (size_t)p.stack_slots * kBasicBlock * sizeof(int);
        hipLaunchKernelGGL((render_basic<kBasicBlock, true>), dim3((unsigned)blocks), dim3(kBasicBlock), lds, st, p);
        s->last_kind = K_BVH;
    } else {
        hipLaunchKernelGGL((render_basic<kBasicBlock, false>), dim3((unsigned)blocks), dim3(kBasicBlock), 0, st, p);
        s->last_kind = K_SMEM;
    }
    HIPCHECK(hipGetLastError());
    if (launch_end(s, st) != 0) return -1;
    s->last_variant = -1;
    s->samples += p.n_items * (unsigned long long)frame_count;
    return 0;
}

// Several frames: frame-major (frame, pixel) items into a scratch buffer, then frame_accumulate (finer work items:
// a shorter tail).  The scratch holds the frames' colour planes and, for a linear render with moments, their moment
// planes behind them; without frame split such a render keeps the moment slots of its whole-pixel items in one plane.
int frame_scratch(rt2_scene* s, RenderParams& p, uint32_t frame_count, bool moments) {
    p.frame_split = frame_count > 1 && s->split_frames && p.n_pix * frame_count < 0xffffffffull;
    if (!p.frame_split && !moments) return 0;
    const size_t planes = p.frame_split ? (size_t)frame_count * (moments ? 2u : 1u) : 1u;
    if (staging_grow(s->fb, (size_t)p.n_pix * planes * sizeof(float4)) != 0) return -1;
    p.frame_buf = s->fb.as<float4>();
    if (p.frame_split) p.n_items = p.n_pix * frame_count;
    return 0;
}

// Cost-ordered items: the previous launch's per-pixel costs (same slab) give this launch's pixel order, most
// expensive first (a shorter tail).
int cost_order_prepare(rt2_scene* s, RenderParams& p, const rt2_uniforms* u, rt2_shard sh, hipStream_t st) {
    if (!s->cost_order) return 0;
    const size_t bytes = (size_t)p.n_pix * sizeof(uint32_t);
    if (bytes > s->cost.cap) s->cost_npix = 0;  // a new map describes nothing yet
    if (staging_grow(s->cost, bytes) != 0 || staging_grow(s->order, bytes) != 0 ||
        staging_grow(s->hist, 32 * sizeof(uint32_t)) != 0)
        return -1;
    uint32_t *d_cost = s->cost.as<uint32_t>(), *d_order = s->order.as<uint32_t>(), *d_hist = s->hist.as<uint32_t>();
    const int key[4] = {(int)u->width, sh.tile_rows, sh.rank, sh.nranks};
    const bool valid = s->cost_npix == p.n_pix && std::memcmp(key, s->cost_key, sizeof(key)) == 0;
    const unsigned long long runs = p.n_pix / 64;
    if (valid && runs > 0) {
        const unsigned blocks = (unsigned)std::min<unsigned long long>((runs + 255) / 256, 2048);
        HIPCHECK(hipMemsetAsync(d_hist, 0, 32 * sizeof(uint32_t), st));
        hipLaunchKernelGGL(cost_histogram, dim3(blocks), dim3(256), 0, st, d_cost, runs, d_hist);
        hipLaunchKernelGGL(cost_offsets, dim3(1), dim3(64), 0, st, d_hist);
        hipLaunchKernelGGL(cost_scatter, dim3(blocks), dim3(256), 0, st, d_cost, runs, d_hist, d_order);
        HIPCHECK(hipGetLastError());
        p.order = d_order;
        p.n_runs = (uint32_t)runs;
    }
    // the cost map keeps each item's start clock in the pixel's own slot:
    // with frame-major items several frames of one pixel run at once, so
    // only frame 0's item of each pixel measures (one
    // writer per slot; a frame-split launch's map is its frame 0's cost)
    p.cost_out = d_cost;
    s->cost_npix = p.n_pix;
    std::memcpy(s->cost_key, key, sizeof(key));
    return 0;
}

// The variant rt2_scene_set_variant asked for, or null: none set, or one this launch cannot take.
const Variant* forced_variant(const rt2_scene* s, bool linear) {
    const Variant* V = s->variant > 0 ? find_variant(s->variant) : nullptr;
    if (!V) return nullptr;
    const int n_groups = (s->n_tris + 31) / 32;
    const bool refused = (s->traversal == RT2_TRAVERSAL_BVH) != is_bvh(V->kind)  // the other traversal's kernel
                         || (V->max_groups > 0 && n_groups > V->max_groups)      // cannot hold this scene
                         || (V->kind == K_MFMA && !s->mfma_ok)                   // scene outside the filter's range
                         || (linear && !linear_twin(*V));                        // an experiment variant without a twin
    return refused ? nullptr : V;
}

// The kernel of a launch of n_items items: the explicit variant (rt2_scene_set_variant) when it exists in this
// build, matches the traversal and can hold the scene; otherwise the automatic choice: the matrix-core filter
// kernels (the scalar-path kernel when the scene is outside the filter's range).  A linear render takes the
// choice's twin.
int choose_variant(const rt2_scene* s, unsigned long long n_items, bool linear, const Variant** out) {
    const Variant* VP = forced_variant(s, linear);
    if (!VP && s->traversal == RT2_TRAVERSAL_BVH) VP = find_variant(kDefaultBvh);
    if (!VP) {
        const int n_groups = (s->n_tris + 31) / 32;
        int vi = s->n_tris <= kSmemMaxTris ? kDefaultBrute : kLargeScene;
        if (s->mfma_ok && find_variant(kMfma)) {
            // the filter on the matrix cores (rt2_mfma.h) for whole images and
            // rank slabs alike (its compaction of <= 32 live rays serves the
            // slabs' tails) and every scene size: config E's 1M triangles too
            // (3.9 vs 6.9 s for kLargeScene on a 480x270 sample)
            vi = kMfma;
            // Scenes of up to 256 groups: the resident kernel (its path state
            // in registers: no packed-field limits).  Larger scenes stream
            // their records from the MALL unless the workgroup shares them:
            // the LDS-tiled kernel (one 12-wave workgroup per CU), without the
            // -tn term (config C 26.94 vs 29.19 s with it; config E sample
            // 1.56 vs 1.60 s); its path state stays in registers too
            if (s->n_tris <= kMfmaSlabMaxTris) {
                // the resident kernel: every group resident in LDS (<= 38) or
                // the first 38 resident and the rest read from L2 (<= 256);
                // a SIMD's waves start together with a few items per lane:
                // fair share, so that they also end together (DESIGN.md
                // "Fair-share issue priority")
                const unsigned long long lanes = (unsigned long long)s->num_cus * (unsigned long long)find_variant(kMfmaRes)->block;
                const bool slab = n_items < kResSlabItems * lanes;
                vi = n_groups <= kResGroups ? (slab ? kMfmaResSlab : kMfmaRes) : (slab ? kMfmaResL2Slab : kMfmaResL2);
            } else if (find_variant(kMfmaTiles)) {
                vi = kMfmaTiles;
            }
        } else if (vi == kDefaultBrute) {
            // scenes outside the matrix filter's range (mfma_ok = 0):
            // items per resident lane decide the tail: a lane ends on a whole
            // item (a pixel-frame's rays share one RNG stream), so with few
            // items per lane the last round runs partly empty.  At >= 4 per
            // lane (a full config B image) the 6-wave scalar-path kernel; below
            // (the 1/2, 1/4, 1/8 slabs of config B on 2, 4, 8 GPUs) the assist
            // kernel, whose idle waves sweep triangle chunks of the busy
            // waves' rays
            const Variant* W = find_variant(kSlab);
            int occ0 = 0;
            HIPCHECK(variant_occupancy(*W, &occ0, 0));
            const unsigned long long lanes = (unsigned long long)s->num_cus * (unsigned long long)std::max(occ0, 1) * W->block;
            if (n_items < 4 * lanes) vi = kSlab;
        }
        VP = find_variant(vi);
    }
    *out = linear ? linear_twin(*VP) : VP;  // every variant chosen above has a twin
    return 0;
}

// V's launch geometry for the items of p: the item regions, the LDS bytes and the BVH stack, the workgroups, the
// assist kernel's shares and the slot image.
int launch_geometry(rt2_scene* s, const Variant& V, RenderParams& p, size_t* lds_out, unsigned long long* blocks_out) {
    // XCD-group item regions serve the BVH walk's L2 locality; the brute-force
    // kernels read the same records for every ray, so they take items from one
    // counter in dispatch order, which spreads neighbouring 64-pixel runs over
    // the XCDs (with <= 1 item per lane a region is one XCD's whole share: an
    // expensive band of rows would set the launch's end).  RT2_ITEM_REGIONS=0/1
    // forces the choice (A/B runs).
    static const int regions_env = [] {
        const char* e = std::getenv("RT2_ITEM_REGIONS");
        return e && *e ? std::atoi(e) : -1;
    }();
    if (regions_env == 0 || (regions_env < 0 && !is_bvh(V.kind))) p.region_ctr = nullptr;
    size_t lds = 0;
    if (V.kind == K_TILED)
        lds = (size_t)3 * sizeof(float4) * kTileTris;
    else if (is_bvh(V.kind)) {
        if (V.kind == K_BVH4) p.stack_slots = std::max(s->bvh_depth, 1);  // next entry in a register
        lds = (size_t)p.stack_slots * V.block * sizeof(int);
    }
    p.bvh_recs = s->d_recs;
    p.bvh_root = s->bvh_root;
    p.recs_ok = s->recs_ok;
    s->last_kind = is_bvh(V.kind) ? K_BVH : V.kind;
    int occ = 0;
    HIPCHECK(variant_occupancy(V, &occ, lds));
    occ = std::max(occ, 1);
    unsigned long long blocks = (unsigned long long)s->num_cus * occ;
    if (V.kind == K_ASSIST) {
        // every resident workgroup is launched: waves without items help the
        // busy waves of their workgroup.  Below 2 items per lane a quarter of
        // the waves take items (each owner has ~3 helpers; 1/4 and 1/8 slabs
        // of config B: 144 / 77 ms against 153 / 81 with half, 151 / 83 with
        // all), otherwise all of them; a chunk job has ~2 chunks per wave.
        const int nw = V.block / 64;
        const unsigned long long lanes = blocks * (unsigned long long)V.block;
        p.assist_cap = p.n_items < 2 * lanes ? std::max(1, nw / 4) : nw;
        constexpr int g = 8;  // the sweep's filter group
        int chunk = (s->n_tris + 2 * nw - 1) / (2 * nw);
        chunk = std::max(g, (chunk + g - 1) / g * g);
        p.assist_chunk = chunk;
        p.assist_nchunks = s->n_tris > 0 ? (s->n_tris + chunk - 1) / chunk : 0;  // <= 2 * nw
    } else {
        const int rays_per_block = V.kind == K_SPLIT ? 64 : V.block;  // split: S waves per 64 rays
        blocks = std::min(blocks, (p.n_items + rays_per_block - 1) / rays_per_block);
    }
    if (V.slot) {
        if (!s->d_slot) {
            rt2h::set_error("rt2_render: the scene has no slot image");
            return -1;
        }
        p.mfma_kt_frag = reinterpret_cast<const _Float16*>(s->d_slot);
    }
    *lds_out = lds;
    *blocks_out = std::max(blocks, 1ull);
    return 0;
}

// frame_accumulate over `planes`: the frames' planes folded into `sum` in frame order.
int frames_fold(const RenderParams& p, const float4* planes, float4* sum, uint4* sum8, hipStream_t st) {
    hipLaunchKernelGGL(frame_accumulate, dim3((unsigned)((p.n_pix + 255) / 256)), dim3(256), 0, st, planes, p.n_pix,
                       p.frame_count, sum, sum8);
    HIPCHECK(hipGetLastError());
    return 0;
}
}  // namespace

// rt2_render (linear = false: d_sumsq is null) and rt2_render_linear (linear =
// true: d_accum is d_sum, d_accum8 null) after their argument checks: one
// selection logic, one schedule; the linear render launches the chosen
// variant's twin (id + kLinearTwin) and folds a second set of frame planes.
static int render_launch(rt2_scene* s, const rt2_uniforms* u, uint32_t frame_begin, uint32_t frame_count, rt2_shard sh,
                         float* d_accum, uint32_t* d_accum8, float* d_sumsq, bool linear, void* stream) {
    const int rows = rt2_shard_rows((int)u->height, sh);
    // frame-major items keep one colour plane per frame: beyond frame_scratch_cap
    // of planes (or 2^32 items), render consecutive frame chunks — the
    // accumulation stays in frame order, so the sums are unchanged
    if (!u->basicShading && s->split_frames && frame_count > 1) {
        const unsigned long long npix = (unsigned long long)rows * u->width;
        // (a linear render with moments keeps two planes per frame)
        const unsigned long long per_frame = npix * sizeof(float4) * (d_sumsq ? 2u : 1u);
        unsigned long long chunk = std::max<unsigned long long>(1, s->frame_scratch_cap / per_frame);
        chunk = std::min<unsigned long long>(chunk, 0xfffffffeull / std::max<unsigned long long>(npix, 1));
        if (chunk < frame_count) {
            for (unsigned long long f0 = 0; f0 < frame_count; f0 += chunk) {
                const uint32_t fc = (uint32_t)std::min<unsigned long long>(chunk, frame_count - f0);
                const int rc = render_launch(s, u, frame_begin + (uint32_t)f0, fc, sh, d_accum, d_accum8, d_sumsq,
                                             linear, stream);
                if (rc != 0) return rc;
            }
            return 0;
        }
    }
    HIPCHECK(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;

    RenderParams p = render_params(s, u, frame_begin, frame_count, sh, rows);
    if (p.n_pix >= 0xffffffffull) {
        rt2h::set_error("rt2_render: more than 2^32-1 pixels in one shard");
        return -1;
    }
    p.accum = reinterpret_cast<float4*>(d_accum);
    // the linear sink never writes 8-bit sums: its kernels read d_sumsq from this field (lin_accum_sq)
    p.accum8 = linear ? reinterpret_cast<uint4*>(d_sumsq) : reinterpret_cast<uint4*>(d_accum8);
    if (launch_begin(s, st) != 0 || counters_reset(s, p, st) != 0) return -1;
    if (u->basicShading) return launch_basic(s, u, p, frame_count, st);
    if (frame_scratch(s, p, frame_count, d_sumsq != nullptr) != 0) return -1;
    if (cost_order_prepare(s, p, u, sh, st) != 0) return -1;
    const Variant* V = nullptr;
    size_t lds = 0;
    unsigned long long blocks = 0;
    if (choose_variant(s, p.n_items, linear, &V) != 0 || launch_geometry(s, *V, p, &lds, &blocks) != 0) return -1;
    s->last_variant = V->id;
    HIPCHECK(V->launch(p, (int)blocks, lds, st));
    HIPCHECK(hipGetLastError());
    if (p.frame_split) {
        if (frames_fold(p, p.frame_buf, p.accum, linear ? nullptr : p.accum8, st) != 0) return -1;
        // the frames' second moments, in the same order
        if (d_sumsq && frames_fold(p, p.frame_buf + (size_t)p.n_pix * frame_count, reinterpret_cast<float4*>(d_sumsq),
                                   nullptr, st) != 0)
            return -1;
    }
    if (launch_end(s, st) != 0) return -1;
    s->samples += p.n_pix * (unsigned long long)p.R * (unsigned long long)frame_count;
    return 0;
}

// How the argument checks of rt2_render, rt2_render_linear and their _host forms differ.
struct RenderArgRules {
    const char* fn;
    const char* out;  // the first output's name; null: both outputs may be null (rt2_render_host)
    bool aligned;     // the two outputs are device sums aligned to 16 bytes (rt2_render_linear)
    bool preview;     // basicShading is a render: the preview, which ignores numRaysPerPixel (rt2_render)
};
// ... and the checks; *rows = the slab's rows.
static int render_args(const RenderArgRules& a, const rt2_scene* s, const rt2_uniforms* u, rt2_shard sh,
                       const void* out0, const void* out1, int* rows) {
    const auto bad = [&](const std::string& what) {
        rt2h::set_error(std::string(a.fn) + ": bad argument: " + what);
        return -1;
    };
    if (!s) return bad("null scene");
    if (!u) return bad("null uniforms");
    if (a.out && !out0) return bad(std::string("null ") + a.out);
    if (a.aligned && (reinterpret_cast<uintptr_t>(out0) % 16 != 0 || reinterpret_cast<uintptr_t>(out1) % 16 != 0))
        return bad("d_sum and d_sumsq must be aligned to 16 bytes");
    if (u->basicShading && !a.preview)
        return bad("basicShading: the preview has no tonemap, rt2_render gives its linear value");
    if (!u->basicShading && u->numRaysPerPixel < 1) return bad("numRaysPerPixel must be >= 1");
    if (u->width < 1 || u->height < 1) return bad("width and height must be >= 1");
    *rows = rt2_shard_rows((int)u->height, sh);
    if (*rows < 0) return bad("bad shard");
    return 0;
}

extern "C" int rt2_render(rt2_scene* s, const rt2_uniforms* u, uint32_t frame_begin, uint32_t frame_count,
                          rt2_shard sh, float* d_accum, uint32_t* d_accum8, void* stream) {
    int rows = 0;
    if (render_args({"rt2_render", "d_accum", false, true}, s, u, sh, d_accum, d_accum8, &rows) != 0) return -1;
    if (frame_count == 0 || rows == 0) return 0;
    return render_launch(s, u, frame_begin, frame_count, sh, d_accum, d_accum8, nullptr, false, stream);
}

extern "C" int rt2_scene_stats(rt2_scene* s, rt2_stats* out, int reset) {
    if (!s || !out) {
        rt2h::set_error("rt2_scene_stats: null argument");
        return -1;
    }
    HIPCHECK(hipSetDevice(s->device));
    HIPCHECK(hipDeviceSynchronize());
    unsigned long long c[kCounters];
    HIPCHECK(hipMemcpy(c, s->d_counters, sizeof(c), hipMemcpyDeviceToHost));
    std::memcpy(s->diag, c, sizeof(c));
    out->samples = s->samples;
    out->segments = c[1];
    // brute force tests every triangle per segment; the BVH kernel counts its
    // leaf tests in c[2]
    out->tests = s->last_kind == K_BVH ? c[2] : c[1] * (unsigned long long)s->n_tris;
    out->node_visits = s->last_kind == K_BVH ? c[3] : 0;
    if (reset) {
        s->samples = 0;
        HIPCHECK(hipMemset(s->d_counters, 0, sizeof(c)));
    }
    return 0;
}

extern "C" int rt2_resolve_rgba32f(const float* d_accum, int64_t n, uint32_t frames, float* d_out, void* stream) {
    if (!d_accum || !d_out || n < 0 || frames == 0) {
        rt2h::set_error("rt2_resolve_rgba32f: bad argument");
        return -1;
    }
    if (n == 0) return 0;
    hipLaunchKernelGGL(resolve_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const float4*>(d_accum), (long long)n, 0.0f, (float)frames,
                       reinterpret_cast<float4*>(d_out));
    HIPCHECK(hipGetLastError());
    return 0;
}

extern "C" int rt2_resolve_rgb8_reference(const uint32_t* acc8, int64_t n, uint32_t frames, uint8_t* out) {
    if (!acc8 || !out || n < 0 || frames == 0) {
        rt2h::set_error("rt2_resolve_rgb8_reference: bad argument");
        return -1;
    }
    const float F = (float)frames;
    for (int64_t i = 0; i < n; i++)
        for (int c = 0; c < 3; c++) {
            float v = std::min(255.0f, (float)acc8[4 * i + c] / F);
            out[3 * i + c] = (uint8_t)v;
        }
    return 0;
}

// The blocking renders' start: the scene's device, host_stream and its four host images for n pixels (16 bytes
// each; out1_bytes for the second resolved output), the float sums zeroed and, with `second`, the second accumulator.
// On failure the images stay owned by the scene (freed by rt2_scene_destroy): no leak on any error path.
static int host_images(rt2_scene* s, size_t n, bool second, size_t out1_bytes) {
    HIPCHECK(hipSetDevice(s->device));
    if (!s->host_stream) HIPCHECK(hipStreamCreateWithFlags(&s->host_stream, hipStreamNonBlocking));
    const size_t bytes[4] = {n * sizeof(float4), n * sizeof(float4), n * sizeof(float4), out1_bytes};
    for (int i = 0; i < 4; i++)
        if (staging_grow(s->host_img[i], bytes[i], &s->host_stream) != 0) return -1;
    HIPCHECK(hipMemsetAsync(s->host_img[0].ptr, 0, bytes[0], s->host_stream));
    if (second) HIPCHECK(hipMemsetAsync(s->host_img[1].ptr, 0, bytes[1], s->host_stream));
    return 0;
}

// The mean over `frames` of the float sums in host image `acc`, resolved into host image `res` and copied to `out`.
static int host_mean(rt2_scene* s, int acc, int res, size_t n, uint32_t frames, float* out) {
    if (rt2_resolve_rgba32f(s->host_img[acc].as<float>(), (int64_t)n, frames, s->host_img[res].as<float>(),
                            s->host_stream) != 0)
        return -1;
    HIPCHECK(hipMemcpyAsync(out, s->host_img[res].ptr, n * sizeof(float4), hipMemcpyDeviceToHost, s->host_stream));
    return 0;
}

extern "C" int rt2_render_host(rt2_scene* s, const rt2_uniforms* u, uint32_t frame_begin, uint32_t frame_count,
                               rt2_shard sh, float* out_rgba, uint8_t* out_rgb8) {
    int rows = 0;
    if (render_args({"rt2_render_host", nullptr, false, true}, s, u, sh, out_rgba, out_rgb8, &rows) != 0) return -1;
    const size_t n = (size_t)rows * u->width;
    if (n == 0 || frame_count == 0) return 0;
    if (host_images(s, n, out_rgb8 != nullptr, n * 3) != 0) return -1;
    hipStream_t st = s->host_stream;
    uint4* const d_acc8 = out_rgb8 ? s->host_img[1].as<uint4>() : nullptr;
    if (rt2_render(s, u, frame_begin, frame_count, sh, s->host_img[0].as<float>(),
                   reinterpret_cast<uint32_t*>(d_acc8), st) != 0)
        return -1;
    if (out_rgba && host_mean(s, 0, 2, n, frame_count, out_rgba) != 0) return -1;
    if (out_rgb8) {
        hipLaunchKernelGGL(resolve_rgb8_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_acc8,
                           (long long)n, (float)frame_count, s->host_img[3].as<uint8_t>());
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipMemcpyAsync(out_rgb8, s->host_img[3].ptr, n * 3, hipMemcpyDeviceToHost, st));
    }
    HIPCHECK(hipStreamSynchronize(st));  // only this render's stream, not the device
    return 0;
}

/* -------------------------------------------------------------------------
 * Linear renders (rt2_path.h end_path_linear; the twins of kVariants)
 * ----------------------------------------------------------------------- */
extern "C" int rt2_render_linear(rt2_scene* s, const rt2_uniforms* u, uint32_t frame_begin, uint32_t frame_count,
                                 rt2_shard sh, float* d_sum, float* d_sumsq, void* stream) {
    int rows = 0;
    if (render_args({"rt2_render_linear", "d_sum", true, false}, s, u, sh, d_sum, d_sumsq, &rows) != 0) return -1;
    if (frame_count == 0 || rows == 0) return 0;
    return render_launch(s, u, frame_begin, frame_count, sh, d_sum, nullptr, d_sumsq, true, stream);
}

extern "C" int rt2_resolve_tonemap(const float* d_linear_sum, int64_t n, uint32_t frames, float* d_out, void* stream) {
    if (!d_linear_sum || !d_out || n < 0 || frames == 0) {
        rt2h::set_error("rt2_resolve_tonemap: bad argument");
        return -1;
    }
    if (n == 0) return 0;
    hipLaunchKernelGGL(resolve_tonemap_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const float4*>(d_linear_sum), (long long)n, (float)frames,
                       reinterpret_cast<float4*>(d_out));
    HIPCHECK(hipGetLastError());
    return 0;
}

extern "C" int rt2_render_linear_host(rt2_scene* s, const rt2_uniforms* u, uint32_t frame_begin, uint32_t frame_count,
                                      rt2_shard sh, float* out_mean, float* out_meansq) {
    int rows = 0;
    if (render_args({"rt2_render_linear_host", "out_mean", false, false}, s, u, sh, out_mean, out_meansq, &rows) != 0)
        return -1;
    const size_t n = (size_t)rows * u->width;
    if (n == 0 || frame_count == 0) return 0;
    if (host_images(s, n, out_meansq != nullptr, n * sizeof(float4)) != 0) return -1;
    if (rt2_render_linear(s, u, frame_begin, frame_count, sh, s->host_img[0].as<float>(),
                          out_meansq ? s->host_img[1].as<float>() : nullptr, s->host_stream) != 0)
        return -1;
    if (host_mean(s, 0, 2, n, frame_count, out_mean) != 0) return -1;
    if (out_meansq && host_mean(s, 1, 3, n, frame_count, out_meansq) != 0) return -1;
    HIPCHECK(hipStreamSynchronize(s->host_stream));  // only this render's stream, not the device
    return 0;
}

/* -------------------------------------------------------------------------
 * Ray queries (rt2_query.h, rt2_occluded.h, rt2_surface.h, rt2_shade.h, rt2_radiance.h)
 *
 * The five families share what is below (DESIGN.md "The query frame"): the argument check, launch_query and the
 * blocking wrappers' staging, and with the renders scene_params, launch_begin and launch_end above; each entry point
 * adds its options and its kernels.
 * ----------------------------------------------------------------------- */
namespace {
// trace_rays_k5r with the arithmetic of 353 (every group resident) and of 355
// (38 groups resident, the rest read from L2: no structural limit at 256
// groups, so it serves every larger scene in the filter's range too)
constexpr MfmaSpec kQueryRes = kResFrame;
constexpr MfmaSpec kQueryResL2 = kResL2;
#ifdef RT2_EXPERIMENTS
// A/B arms of the resident query kernel (rt2_scene_set_query_arm): 1 = its diagnostic counters and clocks (the
// render's 350), 2 = the Y product in the first window too, which a caller's tmax can prune with (the render's 351)
constexpr MfmaSpec kQueryResDiag = kt_win(kt_res(false, false, true, 0, true), kResWin);
constexpr MfmaSpec kQueryResYw = kt_yw(kQueryRes);
constexpr MfmaSpec kQueryResXl = kt_xl(kQueryRes);  // 3 = the exact tests per ray (the render's 400)
#endif
constexpr int kQueryBlock = 256;                  // the *_scalar kernels
constexpr long long kQuerySlice = 1ll << 30;      // rays per *_scalar launch (its grid: 2^22 blocks)

// occluded_k5r: trace_rays_k5r's frame, windows of `win` groups, no Y product (y = false: a frame whose resident
// form leaves the T1 records out of LDS) or the Y product
// from the second window on; wave = the episode per wave (any_window_wave) instead of per ray
constexpr OccSpec occ_spec(bool l2, int win, bool y, bool wave) {
    return OccSpec{kt_win(kt_res(l2, false, true, 4), y ? win : kResWin), win, y, wave};
}
// The shipped window and Y choice (DESIGN.md §Occlusion queries, profiles/occluded_ab.json); the L2 form takes the
// resident form's.
constexpr int kOccWin = 3;
constexpr bool kOccY = false;
constexpr bool kOccWave = true;
constexpr OccSpec kOccRes = occ_spec(false, kOccWin, kOccY, kOccWave);
constexpr OccSpec kOccResL2 = occ_spec(true, kOccWin, kOccY, kOccWave);
static_assert(kQueryRes.block == kQueryResL2.block && kOccRes.m.block == kQueryRes.block, "one block size");

// What rt2_scene_diag reports as the variant last launched after a query (renders: a kVariants id, or -1):
// -2 .. -21, four forms per family.
enum QueryFamily : int { QF_CLOSEST, QF_OCCLUDED, QF_SURFACE, QF_SHADE, QF_RADIANCE };
enum QueryForm : int { QV_RES, QV_RES_L2, QV_SCALAR, QV_BVH };
constexpr int query_code(QueryFamily f, QueryForm v) { return -2 - 4 * f - v; }
static_assert(query_code(QF_CLOSEST, QV_RES) == -2 && query_code(QF_RADIANCE, QV_BVH) == -21, "rt2/__init__.py");

// One array argument of a ray query: device pointers are aligned to `align` bytes.
struct QueryArray {
    const char* name;
    const void* ptr;
    unsigned align;
};

// The argument check of the five ray-array families, before any device call and before the scene is read for
// n = 0.  `device`: the arrays' alignment too.
int query_args(const char* who, const rt2_scene* s, int64_t n, int flags, bool device,
               std::initializer_list<QueryArray> arrays) {
    bool bad = !s || n < 0 || (flags & ~RT2_TRACE_SCALAR);
    std::string need;
    for (const QueryArray& a : arrays) {
        bad = bad || (n > 0 && !a.ptr) || (device && (reinterpret_cast<uintptr_t>(a.ptr) & (a.align - 1)));
        need += std::string(", ") + a.name + (device && a.align > 1 ? " aligned to " + std::to_string(a.align) + " B" : "");
    }
    if (bad) {
        rt2h::set_error(std::string(who) + ": bad argument (a scene, n >= 0" + need + ", flags 0 or RT2_TRACE_SCALAR)");
        return -1;
    }
    if (n > 0 && s->traversal == RT2_TRAVERSAL_BVH && s->n_nodes == 0) {
        rt2h::set_error(std::string(who) + ": bad argument (BVH traversal needs the node array)");
        return -1;
    }
    return 0;
}

// A family's resident or L2 kernel on `blocks` workgroups, and its scalar kernel on the rays of q.
template <auto RES, auto RES_L2, class Q>
void launch_k5r(bool resident, unsigned blocks, hipStream_t st, const RenderParams& p, const Q& q) {
    if (resident)
        hipLaunchKernelGGL(RES, dim3(blocks), dim3(kQueryRes.block), 0, st, p, q);
    else
        hipLaunchKernelGGL(RES_L2, dim3(blocks), dim3(kQueryRes.block), 0, st, p, q);
}
template <auto ARRAY, auto BVH, class Q>
void launch_scalar(bool bvh, hipStream_t st, const RenderParams& p, const Q& q) {
    const unsigned blocks = (unsigned)((q.n + kQueryBlock - 1) / kQueryBlock);
    if (bvh)  // closest_bvh's stack
        hipLaunchKernelGGL(BVH, dim3(blocks), dim3(kQueryBlock), (size_t)p.stack_slots * kQueryBlock * sizeof(int), st,
                           p, q);
    else
        hipLaunchKernelGGL(ARRAY, dim3(blocks), dim3(kQueryBlock), 0, st, p, q);
}

// Launches one query of n > 0 rays on st.  matrix_k(resident, blocks) launches the family's matrix kernel,
// scalar_k(bvh, i0, count) its scalar kernel for the rays [i0, i0 + count).
// RT2_TRACE_AUTO: the matrix kernel at every ray count.  On config B it beat the scalar kernel in every round
// from 2^22 rays down to one 64-ray chunk (closest hit: 36 against 142 us, profiles/trace_rays_ab.json; preview
// shading with the shadow ray: 0.83 against 4.99 ms at 2^22, 52 against 289 us at 64, profiles/shade_ab.json), and
// below 64 rays both kernels are one wave whose time no longer falls: no small-batch threshold is needed.
template <class Matrix, class Scalar>
int launch_query(rt2_scene* s, QueryFamily family, int64_t n, int flags, hipStream_t st, Matrix matrix_k,
                 Scalar scalar_k) {
    const bool bvh = s->traversal == RT2_TRAVERSAL_BVH;
    const bool matrix = !bvh && !(flags & RT2_TRACE_SCALAR) && s->mfma_ok;
    if (launch_begin(s, st) != 0) return -1;  // a query shares the scene's counters with its renders: the same order
    QueryForm form;
    if (matrix) {
        // one 16-wave workgroup per CU, and no more workgroups than have 1,024 rays each:
        // every one of them brings the resident records into its LDS
        const unsigned blocks = (unsigned)std::min<long long>(s->num_cus, (n + 1023) / 1024);
        const bool resident = (s->n_tris + 31) / 32 <= kResGroups;
        matrix_k(resident, blocks);
        HIPCHECK(hipGetLastError());
        form = resident ? QV_RES : QV_RES_L2;
    } else {
        for (long long i0 = 0; i0 < (long long)n; i0 += kQuerySlice) {
            scalar_k(bvh, i0, std::min<long long>(kQuerySlice, (long long)n - i0));
            HIPCHECK(hipGetLastError());
        }
        form = bvh ? QV_BVH : QV_SCALAR;
    }
    s->last_kind = matrix ? K_MFMA : bvh ? K_BVH : K_SMEM;
    s->last_variant = query_code(family, form);
    return launch_end(s, st);
}

// The blocking wrappers' start: the scene's device, host_stream, and staging for n rays, n stream words when
// `rng`, and out_bytes of results.
int staging_begin(rt2_scene* s, size_t n, bool rng, size_t out_bytes) {
    HIPCHECK(hipSetDevice(s->device));
    if (!s->host_stream) HIPCHECK(hipStreamCreateWithFlags(&s->host_stream, hipStreamNonBlocking));
    if (staging_grow(s->stage_rays, n * sizeof(rt2_ray), &s->host_stream) != 0) return -1;
    if (rng && staging_grow(s->stage_rng, n * sizeof(uint32_t), &s->host_stream) != 0) return -1;
    return staging_grow(s->stage_out, out_bytes, &s->host_stream);
}

// A blocking ray-array query over host arrays: rays (and the streams, when rng) in, query(d_rays, d_rng, d_out,
// stream), the records (and the streams) out.
template <class Out, class Query>
int query_host(rt2_scene* s, const rt2_ray* rays, int64_t n, uint32_t* rng, Out* out, Query query) {
    if (staging_begin(s, (size_t)n, rng != nullptr, (size_t)n * sizeof(Out)) != 0) return -1;
    hipStream_t st = s->host_stream;
    rt2_ray* d_rays = static_cast<rt2_ray*>(s->stage_rays.ptr);
    uint32_t* d_rng = static_cast<uint32_t*>(s->stage_rng.ptr);
    Out* d_out = static_cast<Out*>(s->stage_out.ptr);
    HIPCHECK(hipMemcpyAsync(d_rays, rays, (size_t)n * sizeof(rt2_ray), hipMemcpyHostToDevice, st));
    if (rng) HIPCHECK(hipMemcpyAsync(d_rng, rng, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    if (query(d_rays, d_rng, d_out, st) != 0) return -1;
    HIPCHECK(hipMemcpyAsync(out, d_out, (size_t)n * sizeof(Out), hipMemcpyDeviceToHost, st));
    if (rng) HIPCHECK(hipMemcpyAsync(rng, d_rng, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    return 0;
}

// The option checks of both shading and both radiance entry points (whatever n).
int shade_opts_args(const char* who, const rt2_shade_opts* o) {
    if (o && !o->pad[0] && !o->pad[1] && !o->pad[2] && o->max_bounce >= 1 && o->max_bounce <= 256) return 0;
    rt2h::set_error(std::string(who) + ": bad argument (options with pad 0 and max_bounce in 1 .. 256)");
    return -1;
}
int path_opts_args(const char* who, const rt2_path_opts* o) {
    if (o && !o->pad[0] && !o->pad[1] && o->max_bounce >= 1 && o->max_bounce <= 256) return 0;
    rt2h::set_error(std::string(who) + ": bad argument (options with pad 0 and max_bounce in 1 .. 256)");
    return -1;
}
}  // namespace

#ifdef RT2_EXPERIMENTS
// Not in rt2.h (experiment build): 0 = the product kernel, 1 / 2 / 3 = kQueryResDiag / kQueryResYw / kQueryResXl for
// scenes of at most kResGroups groups.
extern "C" int rt2_scene_set_query_arm(rt2_scene* s, int arm) {
    if (!s || arm < 0 || arm > 3) return -1;
    s->query_arm = arm;
    return 0;
}

// Not in rt2.h (experiment build): the A/B arms of occluded_k5r, for the resident and the L2 form alike.  0 = the
// product kernel; 1 = a window of kResWin without Y (no exit inside the resident stretch: the control); 2, 3 =
// windows of 12 and 6 groups without Y; 4, 5 = those windows with the Y product from the second window on; 6 = a
// window of 3 groups without Y; 7 .. 10 = windows of kResWin, 12, 6 and 3 groups without Y and the episode per wave
// instead of per ray.
extern "C" int rt2_scene_set_occluded_arm(rt2_scene* s, int arm) {
    if (!s || arm < 0 || arm > 10) return -1;
    s->occluded_arm = arm;
    return 0;
}
#endif

extern "C" int rt2_trace_rays(rt2_scene* s, const rt2_ray* d_rays, int64_t n, rt2_hit* d_hits, int flags,
                              void* stream) {
    if (query_args("rt2_trace_rays", s, n, flags, true, {{"rays", d_rays, 16}, {"hits", d_hits, 8}}) != 0) return -1;
    if (n == 0) return 0;
    HIPCHECK(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    const RenderParams p = scene_params(s);
    const QueryParams q{d_rays, d_hits, (long long)n};
    return launch_query(
        s, QF_CLOSEST, n, flags, st,
        [&](bool resident, unsigned blocks) {
            constexpr auto l2 = trace_rays_k5r<kQueryResL2>;
#ifdef RT2_EXPERIMENTS
            switch (s->query_arm) {  // the arms replace the resident kernel only
            case 1: return launch_k5r<trace_rays_k5r<kQueryResDiag>, l2>(resident, blocks, st, p, q);
            case 2: return launch_k5r<trace_rays_k5r<kQueryResYw>, l2>(resident, blocks, st, p, q);
            case 3: return launch_k5r<trace_rays_k5r<kQueryResXl>, l2>(resident, blocks, st, p, q);
            }
#endif
            launch_k5r<trace_rays_k5r<kQueryRes>, l2>(resident, blocks, st, p, q);
        },
        [&](bool bvh, long long i0, long long count) {
            launch_scalar<trace_rays_scalar<kQueryBlock, false>, trace_rays_scalar<kQueryBlock, true>>(
                bvh, st, p, QueryParams{d_rays + i0, d_hits + i0, count});
        });
}

extern "C" int rt2_trace_rays_host(rt2_scene* s, const rt2_ray* rays, int64_t n, rt2_hit* hits, int flags) {
    if (query_args("rt2_trace_rays_host", s, n, flags, false, {{"rays", rays, 16}, {"hits", hits, 8}}) != 0) return -1;
    if (n == 0) return 0;
    return query_host(s, rays, n, nullptr, hits, [&](const rt2_ray* d_rays, uint32_t*, rt2_hit* d_hits, hipStream_t st) {
        return rt2_trace_rays(s, d_rays, n, d_hits, flags, st);
    });
}

extern "C" int rt2_occluded(rt2_scene* s, const rt2_ray* d_rays, int64_t n, uint8_t* d_occluded, int flags,
                            void* stream) {
    if (query_args("rt2_occluded", s, n, flags, true, {{"rays", d_rays, 16}, {"occluded", d_occluded, 1}}) != 0)
        return -1;
    if (n == 0) return 0;
    HIPCHECK(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    const RenderParams p = scene_params(s);
    const OccParams q{d_rays, d_occluded, (long long)n};
    return launch_query(
        s, QF_OCCLUDED, n, flags, st,
        [&](bool resident, unsigned blocks) {
#ifdef RT2_EXPERIMENTS
            switch (s->occluded_arm) {
#define RT2_OCC_ARM(A, W, Y, V)                                                                             \
    case A:                                                                                                 \
        return launch_k5r<occluded_k5r<occ_spec(false, W, Y, V)>, occluded_k5r<occ_spec(true, W, Y, V)>>( \
            resident, blocks, st, p, q);
                RT2_OCC_ARM(1, kResWin, false, false)
                RT2_OCC_ARM(2, 12, false, false)
                RT2_OCC_ARM(3, 6, false, false)
                RT2_OCC_ARM(4, 12, true, false)
                RT2_OCC_ARM(5, 6, true, false)
                RT2_OCC_ARM(6, 3, false, false)
                RT2_OCC_ARM(7, kResWin, false, true)
                RT2_OCC_ARM(8, 12, false, true)
                RT2_OCC_ARM(9, 6, false, true)
                RT2_OCC_ARM(10, 3, false, true)
#undef RT2_OCC_ARM
            }
#endif
            launch_k5r<occluded_k5r<kOccRes>, occluded_k5r<kOccResL2>>(resident, blocks, st, p, q);
        },
        [&](bool bvh, long long i0, long long count) {
            launch_scalar<occluded_scalar<kQueryBlock, false>, occluded_scalar<kQueryBlock, true>>(
                bvh, st, p, OccParams{d_rays + i0, d_occluded + i0, count});
        });
}

extern "C" int rt2_occluded_host(rt2_scene* s, const rt2_ray* rays, int64_t n, uint8_t* occluded, int flags) {
    if (query_args("rt2_occluded_host", s, n, flags, false, {{"rays", rays, 16}, {"occluded", occluded, 1}}) != 0)
        return -1;
    if (n == 0) return 0;
    return query_host(s, rays, n, nullptr, occluded, [&](const rt2_ray* d_rays, uint32_t*, uint8_t* d_out, hipStream_t st) {
        return rt2_occluded(s, d_rays, n, d_out, flags, st);
    });
}

extern "C" int rt2_surface_rays(rt2_scene* s, const rt2_ray* d_rays, int64_t n, rt2_surface* d_out, int flags,
                                void* stream) {
    if (query_args("rt2_surface_rays", s, n, flags, true, {{"rays", d_rays, 16}, {"records", d_out, 16}}) != 0)
        return -1;
    if (n == 0) return 0;
    HIPCHECK(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    RenderParams p = scene_params(s);
    scene_shading_params(s, p);
    const SurfaceParams q{d_rays, d_out, (long long)n};
    return launch_query(
        s, QF_SURFACE, n, flags, st,
        [&](bool resident, unsigned blocks) {
            launch_k5r<surface_k5r<kQueryRes>, surface_k5r<kQueryResL2>>(resident, blocks, st, p, q);
        },
        [&](bool bvh, long long i0, long long count) {
            launch_scalar<surface_scalar<kQueryBlock, false>, surface_scalar<kQueryBlock, true>>(
                bvh, st, p, SurfaceParams{d_rays + i0, d_out + i0, count});
        });
}

extern "C" int rt2_surface_rays_host(rt2_scene* s, const rt2_ray* rays, int64_t n, rt2_surface* out, int flags) {
    if (query_args("rt2_surface_rays_host", s, n, flags, false, {{"rays", rays, 16}, {"records", out, 16}}) != 0)
        return -1;
    if (n == 0) return 0;
    return query_host(s, rays, n, nullptr, out, [&](const rt2_ray* d_rays, uint32_t*, rt2_surface* d_out, hipStream_t st) {
        return rt2_surface_rays(s, d_rays, n, d_out, flags, st);
    });
}

extern "C" int rt2_shade_rays(rt2_scene* s, const rt2_ray* d_rays, int64_t n, const rt2_shade_opts* opts,
                              rt2_shaded* d_out, int flags, void* stream) {
    const char* who = "rt2_shade_rays";
    if (query_args(who, s, n, flags, true, {{"rays", d_rays, 16}, {"records", d_out, 16}}) != 0) return -1;
    if (shade_opts_args(who, opts) != 0) return -1;
    if (n == 0) return 0;
    HIPCHECK(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    RenderParams p = scene_params(s);
    scene_shading_params(s, p);
    p.maxBounce = opts->max_bounce;
    p.basicShadow = opts->shadow;
    p.light[0] = opts->light[0];
    p.light[1] = opts->light[1];
    p.light[2] = opts->light[2];
    const ShadeParams q{d_rays, d_out, (long long)n};
    return launch_query(
        s, QF_SHADE, n, flags, st,
        [&](bool resident, unsigned blocks) {
            launch_k5r<shade_rays_k5r<kOccRes>, shade_rays_k5r<kOccResL2>>(resident, blocks, st, p, q);
        },
        [&](bool bvh, long long i0, long long count) {
            launch_scalar<shade_rays_scalar<kQueryBlock, false>, shade_rays_scalar<kQueryBlock, true>>(
                bvh, st, p, ShadeParams{d_rays + i0, d_out + i0, count});
        });
}

extern "C" int rt2_shade_rays_host(rt2_scene* s, const rt2_ray* rays, int64_t n, const rt2_shade_opts* opts,
                                   rt2_shaded* out, int flags) {
    const char* who = "rt2_shade_rays_host";
    if (query_args(who, s, n, flags, false, {{"rays", rays, 16}, {"records", out, 16}}) != 0) return -1;
    if (shade_opts_args(who, opts) != 0) return -1;
    if (n == 0) return 0;
    return query_host(s, rays, n, nullptr, out, [&](const rt2_ray* d_rays, uint32_t*, rt2_shaded* d_out, hipStream_t st) {
        return rt2_shade_rays(s, d_rays, n, opts, d_out, flags, st);
    });
}

extern "C" int rt2_radiance_rays(rt2_scene* s, const rt2_ray* d_rays, int64_t n, const rt2_path_opts* opts,
                                 uint32_t* d_rng, rt2_radiance* d_out, int flags, void* stream) {
    const char* who = "rt2_radiance_rays";
    if (query_args(who, s, n, flags, true, {{"rays", d_rays, 16}, {"rng", d_rng, 4}, {"records", d_out, 16}}) != 0)
        return -1;
    if (path_opts_args(who, opts) != 0) return -1;
    if (n == 0) return 0;
    HIPCHECK(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    RenderParams p = scene_params(s);
    scene_shading_params(s, p);
    p.maxBounce = opts->max_bounce;
    p.envLight = opts->environmental_light;
    const RadianceParams q{d_rays, d_rng, d_out, (long long)n};
    return launch_query(
        s, QF_RADIANCE, n, flags, st,
        [&](bool resident, unsigned blocks) {
            launch_k5r<radiance_rays_k5r<kOccRes>, radiance_rays_k5r<kOccResL2>>(resident, blocks, st, p, q);
        },
        [&](bool bvh, long long i0, long long count) {
            launch_scalar<radiance_rays_scalar<kQueryBlock, false>, radiance_rays_scalar<kQueryBlock, true>>(
                bvh, st, p, RadianceParams{d_rays + i0, d_rng + i0, d_out + i0, count});
        });
}

extern "C" int rt2_radiance_rays_host(rt2_scene* s, const rt2_ray* rays, int64_t n, const rt2_path_opts* opts,
                                      uint32_t* rng, rt2_radiance* out, int flags) {
    const char* who = "rt2_radiance_rays_host";
    if (query_args(who, s, n, flags, false, {{"rays", rays, 16}, {"rng", rng, 4}, {"records", out, 16}}) != 0)
        return -1;
    if (path_opts_args(who, opts) != 0) return -1;
    if (n == 0) return 0;
    return query_host(s, rays, n, rng, out, [&](const rt2_ray* d_rays, uint32_t* d_rng, rt2_radiance* d_out, hipStream_t st) {
        return rt2_radiance_rays(s, d_rays, n, opts, d_rng, d_out, flags, st);
    });
}

/* -------------------------------------------------------------------------
 * Ray generators: the preview camera (rt2_surface.h) and the path tracer's (rt2_radiance.h)
 * ----------------------------------------------------------------------- */
namespace {
// The argument checks of both camera-ray entry points; the slab's pixel count in *n.
int camera_rays_args(const char* who, const rt2_scene* s, const rt2_uniforms* u, rt2_shard sh, const void* rays,
                     bool device, long long* n) {
    const std::string w(who);
    if (!s || !u) {
        rt2h::set_error(w + ": bad argument (a scene and uniforms)");
        return -1;
    }
    if (u->width < 1 || u->height < 1 || u->width > 0x3fffffffu || u->height > 0x3fffffffu) {
        rt2h::set_error(w + ": bad argument (width and height must be in [1, 2^30))");
        return -1;
    }
    const int rows = rt2_shard_rows((int)u->height, sh);
    if (rows < 0) {
        rt2h::set_error(w + ": bad argument (bad shard)");
        return -1;
    }
    *n = (long long)rows * (long long)u->width;
    if (*n > 0 && (!rays || (device && (reinterpret_cast<uintptr_t>(rays) & 15)))) {
        rt2h::set_error(w + ": bad argument (rays must not be null" + (device ? ", and aligned to 16 B)" : ")"));
        return -1;
    }
    return 0;
}

// The argument checks of both path-camera entry points: camera_rays_args and the stream array.
int path_rays_args(const char* who, const rt2_scene* s, const rt2_uniforms* u, rt2_shard sh, const void* rng,
                   const void* rays, bool device, long long* n) {
    if (camera_rays_args(who, s, u, sh, rays, device, n) != 0) return -1;
    if (*n > 0 && (!rng || (device && (reinterpret_cast<uintptr_t>(rng) & 3)))) {
        rt2h::set_error(std::string(who) + ": bad argument (rng must not be null" +
                        (device ? ", and aligned to 4 B)" : ")"));
        return -1;
    }
    return 0;
}

// What CameraParams and PathRaysParams share: the view, the image and shard, the slab.
template <class P>
void camera_params(P& c, const rt2_uniforms* u, rt2_shard sh, long long n, rt2_ray* d_rays) {
    std::memset(&c, 0, sizeof(c));
    copy3(c.cam, u->cameraPos);
    copy3(c.vpRight, u->viewportRight);
    copy3(c.vpUp, u->viewportUp);
    copy3(c.vpFront, u->viewportFront);
    c.W = (int)u->width;
    c.H = (int)u->height;
    c.tile_rows = sh.tile_rows;
    c.rank = sh.rank;
    c.nranks = sh.nranks;
    c.n = n;
    c.out = d_rays;
}
}  // namespace

extern "C" int rt2_camera_rays(rt2_scene* s, const rt2_uniforms* u, rt2_shard sh, rt2_ray* d_rays, void* stream) {
    long long n = 0;
    if (camera_rays_args("rt2_camera_rays", s, u, sh, d_rays, true, &n) != 0) return -1;
    if (n == 0) return 0;
    HIPCHECK(hipSetDevice(s->device));
    CameraParams c;
    camera_params(c, u, sh, n, d_rays);
    hipLaunchKernelGGL(camera_rays_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, c);
    HIPCHECK(hipGetLastError());
    return 0;
}

extern "C" int rt2_camera_rays_host(rt2_scene* s, const rt2_uniforms* u, rt2_shard sh, rt2_ray* rays) {
    long long n = 0;
    if (camera_rays_args("rt2_camera_rays_host", s, u, sh, rays, false, &n) != 0) return -1;
    if (n == 0) return 0;
    if (staging_begin(s, (size_t)n, false, 0) != 0) return -1;
    hipStream_t st = s->host_stream;
    rt2_ray* d_rays = static_cast<rt2_ray*>(s->stage_rays.ptr);
    if (rt2_camera_rays(s, u, sh, d_rays, st) != 0) return -1;
    HIPCHECK(hipMemcpyAsync(rays, d_rays, (size_t)n * sizeof(rt2_ray), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    return 0;
}

extern "C" int rt2_path_rays(rt2_scene* s, const rt2_uniforms* u, rt2_shard sh, uint32_t frame_index, int reseed,
                             uint32_t* d_rng, rt2_ray* d_rays, void* stream) {
    long long n = 0;
    if (path_rays_args("rt2_path_rays", s, u, sh, d_rng, d_rays, true, &n) != 0) return -1;
    if (n == 0) return 0;
    HIPCHECK(hipSetDevice(s->device));
    PathRaysParams c;
    camera_params(c, u, sh, n, d_rays);
    copy3(c.pixR, u->pixelRight);
    copy3(c.pixU, u->pixelUp);
    copy3(c.defR, u->defocusDiskRight);
    copy3(c.defU, u->defocusDiskUp);
    c.frame = frame_index;
    c.reseed = reseed;
    c.rng = d_rng;
    hipLaunchKernelGGL(path_rays_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, c);
    HIPCHECK(hipGetLastError());
    return 0;
}

extern "C" int rt2_path_rays_host(rt2_scene* s, const rt2_uniforms* u, rt2_shard sh, uint32_t frame_index,
                                  int reseed, uint32_t* rng, rt2_ray* rays) {
    long long n = 0;
    if (path_rays_args("rt2_path_rays_host", s, u, sh, rng, rays, false, &n) != 0) return -1;
    if (n == 0) return 0;
    if (staging_begin(s, (size_t)n, true, 0) != 0) return -1;
    hipStream_t st = s->host_stream;
    rt2_ray* d_rays = static_cast<rt2_ray*>(s->stage_rays.ptr);
    uint32_t* d_rng = static_cast<uint32_t*>(s->stage_rng.ptr);
    if (!reseed) HIPCHECK(hipMemcpyAsync(d_rng, rng, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    if (rt2_path_rays(s, u, sh, frame_index, reseed, d_rng, d_rays, st) != 0) return -1;
    HIPCHECK(hipMemcpyAsync(rays, d_rays, (size_t)n * sizeof(rt2_ray), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(rng, d_rng, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    return 0;
}

// Not in rt2.h (diagnostics): counters of the last rt2_scene_stats call
// [1] segments, [2] groups, [3] groups with survivors, [4] exact iterations,
// [5] lane survivors (STATS variants only), and the variant last launched.
// Not in rt2.h (diagnostics): all kCounters counters of the last stats call.
extern "C" int rt2_scene_diag_ex(rt2_scene* s, unsigned long long* out, int n) {
    if (!s || !out || n < 0) return -1;
    std::memcpy(out, s->diag, sizeof(unsigned long long) * (size_t)std::min(n, kCounters));
    return std::min(n, kCounters);
}

// Not in rt2.h (test hook): the cost map of the last cost-ordered launch
// (shader clocks per pixel of the slab) into `out` (n entries); returns the
// pixels it describes (0 = no valid map), < 0 on error.
extern "C" long long rt2_scene_cost_map(rt2_scene* s, uint32_t* out, unsigned long long n) {
    if (!s) return -1;
    if (!s->cost.ptr || s->cost_npix == 0) return 0;
    if (out && n >= s->cost_npix) {
        HIPCHECK(hipSetDevice(s->device));
        HIPCHECK(hipDeviceSynchronize());
        HIPCHECK(hipMemcpy(out, s->cost.ptr, s->cost_npix * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    return (long long)s->cost_npix;
}

// Not in rt2.h (diagnostics): whether the scene's triangles admit sweep_plk,
// its A (max |a_i|) and how many triangles carry an always-pass record.
extern "C" int rt2_scene_plk_info(rt2_scene* s, int* ok, float* A, int* n_outside) {
    if (!s) return -1;
    if (ok) *ok = s->plk_ok;
    if (A) *A = s->plk_A;
    if (n_outside) *n_outside = s->plk_outside;
    return 0;
}

extern "C" int rt2_scene_diag(rt2_scene* s, unsigned long long* out8, int* last_variant) {
    if (!s || !out8) return -1;
    std::memcpy(out8, s->diag, 8 * sizeof(unsigned long long));
    if (last_variant) *last_variant = s->last_variant;
    return 0;
}

// Not in rt2.h (test hook): exhaustive reciprocal check over [lo, hi] bit patterns.
extern "C" int rt2_device_rcp_check(uint32_t lo, uint32_t hi, int variant, unsigned long long* mismatches,
                                    uint32_t* first_bad) {
    unsigned long long* d = nullptr;
    HIPCHECK(hipMalloc(&d, 16));
    HIPCHECK(hipMemset(d, 0, 8));
    uint32_t init = 0xffffffffu;
    HIPCHECK(hipMemcpy((char*)d + 8, &init, 4, hipMemcpyHostToDevice));
    const unsigned long long count = (unsigned long long)hi - lo + 1;
    hipLaunchKernelGGL(rcp_check_kernel, dim3(4096), dim3(256), 0, 0, lo, count, variant, d, (uint32_t*)((char*)d + 8));
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpy(mismatches, d, 8, hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(first_bad, (char*)d + 8, 4, hipMemcpyDeviceToHost));
    (void)hipFree(d);
    return 0;
}

// Not in rt2.h (test hook): div_mk (mode 0) or div64 (mode 1) against IEEE
// division on `count` random (n, d) pairs of the ranges the kernels use them on.
extern "C" int rt2_device_div_check(uint32_t seed, unsigned long long count, int mode,
                                    unsigned long long* mismatches, uint32_t* first_bad) {
    unsigned long long* d = nullptr;
    HIPCHECK(hipMalloc(&d, 16));
    HIPCHECK(hipMemset(d, 0, 8));
    uint32_t init = 0xffffffffu;
    HIPCHECK(hipMemcpy((char*)d + 8, &init, 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(div_check_kernel, dim3(8192), dim3(256), 0, 0, seed, count, mode, d,
                       (uint32_t*)((char*)d + 8));
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpy(mismatches, d, 8, hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(first_bad, (char*)d + 8, 4, hipMemcpyDeviceToHost));
    (void)hipFree(d);
    return 0;
}

// Not in rt2.h (test hook): device numerics self-test, host in/out arrays.
extern "C" int rt2_device_selftest(const float* in, int32_t n, float* out10) {
    float *din = nullptr, *dout = nullptr;
    HIPCHECK(hipMalloc(&din, (size_t)n * 4));
    HIPCHECK(hipMalloc(&dout, (size_t)n * 40));
    HIPCHECK(hipMemcpy(din, in, (size_t)n * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(selftest_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, din, n, dout);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpy(out10, dout, (size_t)n * 40, hipMemcpyDeviceToHost));
    (void)hipFree(din);
    (void)hipFree(dout);
    return 0;
}

// Not in rt2.h (test hook): one operation of DESIGN.md §Numerics (numerics_kernel's codes) on n rows of 9 input
// words, giving n rows of 4 output words; host arrays of binary32 bit patterns, one launch.
extern "C" int rt2_device_numerics(int32_t op, const uint32_t* in9, int32_t n, uint32_t* out4) {
    if (op < 0 || op > 28 || n < 0 || (n > 0 && (!in9 || !out4))) {
        rt2h::set_error("rt2_device_numerics: bad argument");
        return -1;
    }
    if (n == 0) return 0;
    uint32_t *din = nullptr, *dout = nullptr;
    HIPCHECK(hipMalloc(&din, (size_t)n * 36));
    HIPCHECK(hipMalloc(&dout, (size_t)n * 16));
    HIPCHECK(hipMemcpy(din, in9, (size_t)n * 36, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(numerics_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, op, din, n, dout);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpy(out4, dout, (size_t)n * 16, hipMemcpyDeviceToHost));
    (void)hipFree(din);
    (void)hipFree(dout);
    return 0;
}

// Not in rt2.h (test hook): copies one of the scene's derived device arrays to
// host memory: 0 = pre-transformed triangles (3 float4 each), 1 = the filter
// records in the 16x16x32 layout, 2 = their per-triangle tau, 3 = sweep_k16 records,
// 4 = their tau, 5 = the k5 form's per-triangle m.z residual bounds, 6 = the
// kthr records (threshold in the K-slots), 7 = the cluster table (rt2_cluster_table of rt2_cluster.h, the host's
// copy; n = 0 when the scene has no compact cluster), 8 = the table over the slot groups of the resident kernel's slot
// image, 9 = its slot_tri (int32 per triangle; empty for a scene without the image).  Returns the array's size in
// bytes (nothing copied when `host` is null or `bytes` is too small), < 0 on error.
extern "C" long long rt2_scene_export(rt2_scene* s, int what, void* host, unsigned long long bytes) {
    if (!s) return -1;
    const size_t n = (size_t)std::max(s->n_tris, 1), n16 = (size_t)(s->n_tris + 15) / 16 * 16,
                 n32 = (size_t)(s->n_tris + 31) / 32 * 32;
    const void* src = nullptr;
    size_t sz = 0;
    if ((what == 1 || what == 2) && ensure_mfma16(s) != 0) return -1;
    if (what == 7) {
        if (host && bytes >= sizeof(s->clusters)) std::memcpy(host, &s->clusters, sizeof(s->clusters));
        return (long long)sizeof(s->clusters);
    }
    if (what == 8) {
        if (host && bytes >= sizeof(s->slot_table)) std::memcpy(host, &s->slot_table, sizeof(s->slot_table));
        return (long long)sizeof(s->slot_table);
    }
    if (what == 9) {
        const size_t b = s->slot_tri.size() * sizeof(int32_t);
        if (host && b && bytes >= b) std::memcpy(host, s->slot_tri.data(), b);
        return (long long)b;
    }
    switch (what) {
    case 0: src = s->d_tri, sz = n * 3 * sizeof(float4); break;
    case 1: src = s->d_mfma, sz = n16 * kMfmaQ * 32 * sizeof(_Float16); break;
    case 2: src = s->d_mfma_tau, sz = n16 * sizeof(float); break;
    case 3: src = s->d_mfma_k16, sz = n32 * kK16Ops * 16 * sizeof(_Float16); break;
    case 4: src = s->d_mfma_k16_tau, sz = n32 * sizeof(float); break;
    case 5: src = s->d_mfma_k16_bnd, sz = n32 * sizeof(float2); break;
    case 6: src = s->d_mfma_kt, sz = n32 * kKtOps * 16 * sizeof(_Float16); break;
    default: return -1;
    }
    if (!src || s->n_tris == 0) return 0;
    if (host && bytes >= sz) {
        HIPCHECK(hipSetDevice(s->device));
        HIPCHECK(hipDeviceSynchronize());
        HIPCHECK(hipMemcpy(host, src, sz, hipMemcpyDeviceToHost));
    }
    return (long long)sz;
}

// A caller's table: contiguous ranges that cover the scene's ng groups (n = 0: no clusters)
static bool cluster_table_covers(const rt2_cluster_table* t, int ng) {
    bool ok = t->n >= 0 && t->n <= RT2_MAX_CLUSTERS && (t->n == 0 || ng <= kResGroups) && t->far_o >= 0.0f;
    int g = 0;
    for (int k = 0; ok && k < t->n; k++) {
        const int g1 = t->c[k].g1_flags & 0xffff;
        ok = t->c[k].g0 == g && g1 > g && (t->c[k].g1_flags & ~(0xffff | RT2_CLUSTER_COMPACT)) == 0;
        g = g1;
    }
    return ok && (t->n == 0 || g == ng);
}

// Not in rt2.h (test hook): replaces the scene's cluster table (rt2_cluster.h) by the caller's, for tests that
// need clusters the upload rule would not choose.  The ranges must be contiguous and cover the scene's groups (the
// kernel steps through the resident records by them); that every triangle lies inside its cluster's box is the
// caller's business: a box that leaves one out loses hits, nothing else.  n = 0 switches the clusters off.
// This index-order table also becomes the slot image's, with the identity order: 353 / 354 then sweep what the
// kernels on the index image sweep.
extern "C" int rt2_scene_set_clusters(rt2_scene* s, const rt2_cluster_table* t) {
    if (!s || !t || !s->d_mfma_kt) {
        rt2h::set_error("rt2_scene_set_clusters: bad argument (a scene with matrix-filter records)");
        return -1;
    }
    const int ng = (s->n_tris + 31) / 32;
    if (!cluster_table_covers(t, ng)) {
        rt2h::set_error("rt2_scene_set_clusters: the ranges must be contiguous and cover the scene's groups");
        return -1;
    }
    HIPCHECK(hipSetDevice(s->device));
    HIPCHECK(hipDeviceSynchronize());
    s->clusters = *t;
    const size_t kt_bytes = (size_t)ng * 32 * kKtOps * 16 * sizeof(_Float16);
    HIPCHECK(hipMemcpy(reinterpret_cast<char*>(s->d_mfma_kt) + kt_bytes, &s->clusters, sizeof(s->clusters),
                       hipMemcpyHostToDevice));
    if (s->d_slot) {
        std::iota(s->slot_tri.begin(), s->slot_tri.end(), 0);
        s->slot_table = *t;
        if (build_slot_image(s) != 0) return -1;
    }
    return 0;
}

// Not in rt2.h (test hook): installs an explicit slot order (a permutation of the scene's triangle indices) and
// its table over the slot groups, for a scene of at most kResGroups groups.  The table's rules are
// rt2_scene_set_clusters'; the index image and its table are not touched.
extern "C" int rt2_scene_set_slot_order(rt2_scene* s, const int32_t* slot_tri, const rt2_cluster_table* t) {
    if (!s || !slot_tri || !t || !s->d_slot) {
        rt2h::set_error("rt2_scene_set_slot_order: bad argument (a scene with a slot image)");
        return -1;
    }
    const int ng = (s->n_tris + 31) / 32;
    std::vector<char> seen((size_t)s->n_tris, 0);
    for (int k = 0; k < s->n_tris; k++) {
        if (slot_tri[k] < 0 || slot_tri[k] >= s->n_tris || seen[(size_t)slot_tri[k]]) {
            rt2h::set_error("rt2_scene_set_slot_order: slot_tri must be a permutation of the triangle indices");
            return -1;
        }
        seen[(size_t)slot_tri[k]] = 1;
    }
    if (!cluster_table_covers(t, ng)) {
        rt2h::set_error("rt2_scene_set_slot_order: the ranges must be contiguous and cover the scene's groups");
        return -1;
    }
    HIPCHECK(hipSetDevice(s->device));
    HIPCHECK(hipDeviceSynchronize());
    s->slot_tri.assign(slot_tri, slot_tri + s->n_tris);
    s->slot_table = *t;
    return build_slot_image(s);
}

// Not in rt2.h (test hook): the matrix filter's terms on the hardware
// (mfma_probe_kernel) for n_rays rays (a multiple of 64; 8 floats each: o.xyz,
// best, d.xyz, 0) against every triangle of the scene.  layout 0 = the
// 16x16x32 form, 1 = the 8-product k16 form, 2 = its 5-product form
// (sweep_k16: U, -V, X from the first K-half), 3 = the 5-product form with the
// threshold in the accumulator (U, -V, X, Y shifted by TT = -Tl'', TT in the
// -tn slot), 4 = layout 3 with the fragments built in registers by frag_pair,
// 5 = the threshold in the K-slots (render_mfma_k5r / render_mfma_k5t,
// frag_pair fragments: U, -V, X, Y, slot 3 zero), 6 = layout 5 with each
// ray's own W (MfmaSpec::kt_lane_w), 7 = layout 6's U, -V, X by the 16-row
// products of MfmaSpec::cluster_rows16 (kt_group16's operands; terms 3, 4 stay 0),
// 8 = the same by the 8-row products of MfmaSpec::cluster_rows8 (kt_group8's operands).
// Host outputs, sized by the caller: terms [n_rays][n_pad][5]
// (n_pad = triangles padded to 16 / 32), frags [n_rays][80] f16 bits (the LDS
// row of layouts 0..3: main slots 0..31 and Y slots 16..31; layouts 4, 5 also
// the register fragments the MFMA read: main K-half at 48..63, Y at 64..79),
// rinfo [n_rays][8], accept [n_rays][n_tris].
extern "C" int rt2_mfma_probe(rt2_scene* s, int layout, const float* rays, int32_t n_rays, float* terms,
                              uint16_t* frags, float* rinfo, uint8_t* accept) {
    if (!s || !rays || n_rays <= 0 || n_rays % 64 != 0 || !terms || !frags || !rinfo || !accept ||
        layout < 0 || layout > 8 || s->n_tris < 1 || !s->mfma_ok) {
        rt2h::set_error("rt2_mfma_probe: bad argument (n_rays a positive multiple of 64, a scene in the filter's "
                        "range)");
        return -1;
    }
    HIPCHECK(hipSetDevice(s->device));
    if (layout == 0 && ensure_mfma16(s) != 0) return -1;
    const int n_pad = layout >= 1 ? (s->n_tris + 31) / 32 * 32 : (s->n_tris + 15) / 16 * 16;
    const size_t nr = (size_t)n_rays;
    const size_t b_rays = nr * 8 * sizeof(float), b_terms = nr * n_pad * 5 * sizeof(float),
                 b_frags = nr * 80 * sizeof(uint16_t), b_info = nr * 8 * sizeof(float), b_acc = nr * s->n_tris;
    char* d = nullptr;
    HIPCHECK(hipMalloc(&d, b_rays + b_terms + b_frags + b_info + b_acc + 64));
    char* p0 = d;
    float4* d_rays = (float4*)p0;
    float* d_terms = (float*)(p0 += b_rays);
    _Float16* d_frags = (_Float16*)(p0 += b_terms);
    float* d_info = (float*)(p0 += b_frags);
    uint8_t* d_acc = (uint8_t*)(p0 += b_info);
    int rc = 0;
    auto run = [&]() -> int {
        HIPCHECK(hipMemcpy(d_rays, rays, b_rays, hipMemcpyHostToDevice));
        HIPCHECK(hipMemset(d_terms, 0, b_terms));
        RenderParams p;
        std::memset(&p, 0, sizeof(p));
        p.tri = s->d_tri;
        p.n_tris = s->n_tris;
        p.mfma_frag = s->d_mfma;
        p.mfma_tau = s->d_mfma_tau;
        p.mfma_A = s->mfma_A;
        p.mfma_k16_frag = s->d_mfma_k16;
        p.mfma_k16_tau = s->d_mfma_k16_tau;
        p.mfma_k16_bnd = s->d_mfma_k16_bnd;
        p.mfma_kt_frag = s->d_mfma_kt;
        const auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(n_rays / 64), dim3(64), 0, 0, p, d_rays, n_pad, d_terms, d_frags, d_info,
                               d_acc);
        };
        switch (layout) {
        case 0: launch(mfma_probe_kernel<0>); break;
        case 1: launch(mfma_probe_kernel<1>); break;
        case 2: launch(mfma_probe_kernel<2>); break;
        case 3: launch(mfma_probe_kernel<3>); break;
        case 4: launch(mfma_probe_kernel<4>); break;
        case 5: launch(mfma_probe_kernel<5>); break;
        case 6: launch(mfma_probe_kernel<6>); break;
        case 7: launch(mfma_probe_kernel<7>); break;
        default: launch(mfma_probe_kernel<8>); break;
        }
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipDeviceSynchronize());
        HIPCHECK(hipMemcpy(terms, d_terms, b_terms, hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(frags, d_frags, b_frags, hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(rinfo, d_info, b_info, hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(accept, d_acc, b_acc, hipMemcpyDeviceToHost));
        return 0;
    };
    rc = run();
    (void)hipFree(d);
    return rc;
}
