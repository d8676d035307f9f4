/*
 * rt2.h — C-ABI of the MI355X-native render path (drop-in for the reference's
 * GL compute dispatch of RayTracing/Assets/Shaders/compute.glsl).
 *
 * Every entry point below replaces one piece of the reference's GPU boundary
 * (SURVEY.md §8b).  POD layouts are byte-identical to the reference's host
 * structs so a caller can hand over the very vectors it used to pass to
 * glBufferData:
 *
 *   rt2_triangle  == RTXTriangle      RayTracing/Assets/headers/mesh.h:112-139   (80 B)
 *   rt2_material  == Material         RayTracing/Assets/headers/mesh.h:26-103    (96 B)
 *   rt2_node      == Node             RayTracing/Assets/headers/BVH.h:54-65      (48 B)
 *   rt2_uniforms  == GlobalUniforms   RayTracing/Assets/headers/camera.h:10-36   (192 B, std140)
 *
 * Status convention: 0 = ok, < 0 = error; rt2_last_error() returns a
 * thread-local message.  No C++ exception crosses this ABI.
 *
 * Two groups of functions:
 *   (1) device path  (rt2_scene_*, rt2_render*, rt2_resolve_*) — HIP on gfx950;
 *   (2) host surface (rt2_sd_*, rt2_camera_*, rt2_write_png) — the reference's
 *       OBJ/MTL loader, Cornell-box builders, BVH build, camera and PNG writer,
 *       restated in C++ behind the same ABI.
 */
#ifndef RT2_H
#define RT2_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT2_ABI_VERSION 4

/* Material types: mesh.h:16-22 == compute.glsl:7-13 */
enum {
    RT2_DIFFUSE = 0,
    RT2_SPECULAR = 1,
    RT2_LIGHT = 2,
    RT2_CHECKER = 3,
    RT2_GLASS = 4,
    RT2_TEXTURE = 5,
    RT2_GLASS_HIGHLIGHT = 6
};

typedef struct rt2_vec4 { float x, y, z, w; } rt2_vec4;
typedef struct rt2_vec2 { float x, y; } rt2_vec2;

/* RTXTriangle, mesh.h:112-139.  GLSL std430 `Triangle` (compute.glsl:46-56)
 * reads a/b/c at byte 0/16/32, the UVs at 48/56/64 and mtlIndex at 72. */
typedef struct rt2_triangle {
    rt2_vec4 a, b, c;
    rt2_vec2 aTex, bTex, cTex;
    int32_t materialIndex;
    float pad;
} rt2_triangle;

/* Material, mesh.h:26-103 == compute.glsl:17-37 */
typedef struct rt2_material {
    rt2_vec4 color;
    rt2_vec4 specularColor;
    rt2_vec4 emissionColor;
    int32_t textureIndex;
    float emissionStrength;
    float smoothness;
    float specularProbability;
    float checkerScale;
    float refractiveIndex;
    int32_t materialType;
    int32_t index;
    int32_t isEdgeHighlight;
    int32_t pad1, pad2, pad3;
} rt2_material;

/* Node + BoundingBox, BVH.h:11-65 == compute.glsl:58-73 */
typedef struct rt2_node {
    float bmin[3];
    float pad0;
    float bmax[3];
    float pad1;
    int32_t triangleIndex;
    int32_t triangleCount;
    int32_t childIndex;
    int32_t pad;
} rt2_node;

/* GlobalUniforms, camera.h:10-36 == compute.glsl:119-146 (std140) */
typedef struct rt2_uniforms {
    int32_t pad;
    int32_t numTextures;
    uint32_t width;
    uint32_t height;
    int32_t numSpheres;
    int32_t numTriangles;
    int32_t basicShading;
    int32_t basicShadingShadow;
    rt2_vec4 basicShadingLightPosition;
    int32_t environmentalLight;
    int32_t maxBounceCount;
    int32_t numRaysPerPixel;
    uint32_t frameIndex;
    rt2_vec4 cameraPos;
    rt2_vec4 viewportRight;
    rt2_vec4 viewportUp;
    rt2_vec4 viewportFront;
    rt2_vec4 pixelRight;
    rt2_vec4 pixelUp;
    rt2_vec4 defocusDiskRight;
    rt2_vec4 defocusDiskUp;
} rt2_uniforms;

/* Image-row shard: the rows y in [0, height) with
 *   (y / tile_rows) % nranks == rank
 * in increasing order form this rank's slab (SURVEY.md §8e, row-tile
 * interleave).  {1, 0, 1} is the whole image. */
typedef struct rt2_shard {
    int32_t tile_rows;
    int32_t rank;
    int32_t nranks;
} rt2_shard;

/* Work counters of the last render on a scene (SURVEY.md §8d units). */
typedef struct rt2_stats {
    uint64_t samples;   /* pixel-rays traced = pixels * R * F              */
    uint64_t segments;  /* closest-hit queries (bounces actually traced)     */
    uint64_t tests;     /* ray-triangle tests = segments * N (brute force);
                           leaf tests (BVH traversal)                        */
    uint64_t node_visits; /* BVH traversal: interior nodes popped (box pairs
                             tested); 0 for brute force                      */
} rt2_stats;

/* An 8-bit image as stb_image returns it: `channels` (1..4) interleaved
 * bytes per pixel, rows of width*channels bytes, row 0 first in memory. */
typedef struct rt2_image {
    int32_t width;
    int32_t height;
    int32_t channels;
    uint8_t* pixels;
} rt2_image;

const char* rt2_last_error(void);
int rt2_abi_version(void);

/* ------------------------------------------------------------------------
 * (1) Device path
 * ---------------------------------------------------------------------- */

typedef struct rt2_scene rt2_scene;

/* Replaces the three SSBO uploads (rayTracing.cpp:1323-1325, SSBO.cpp:3-10,
 * glBufferData GL_STATIC_DRAW: the arrays are copied, the caller keeps
 * ownership).  `nodes` may be NULL (brute-force traversal does not need it).
 * Materials with materialType TEXTURE sample the images given to
 * rt2_scene_set_textures (getTriangleTextureColor, compute.glsl:342-368);
 * until that call they read black, as compute.glsl:349-350 does for a
 * texture index outside numTextures. */
int rt2_scene_create(const rt2_triangle* tris, int32_t n_tris,
                     const rt2_material* mats, int32_t n_mats,
                     const rt2_node* nodes, int32_t n_nodes,
                     int32_t device, rt2_scene** out);
void rt2_scene_destroy(rt2_scene* scene);

/* Number of slab rows a shard owns for an image of `height` rows. */
int32_t rt2_shard_rows(int32_t height, rt2_shard shard);
/* Image row y of slab row `local_row` (inverse of the interleave). */
int32_t rt2_shard_row(int32_t local_row, rt2_shard shard);

/* Replaces `frame_count` consecutive glDispatchCompute calls of compute.glsl
 * (rayTracing.cpp:184-191, uniforms->frameIndex = frame_begin + i), restricted
 * to the shard's rows, with the per-frame rgba32f imageStore (compute.glsl:700)
 * folded into an accumulator instead of a texture:
 *
 *   d_accum[4*(slab_row*W + x) + c] += color_f[c]   for f = frame_begin ...
 *
 * in increasing frame order (so splitting the frames over several calls gives
 * bit-identical sums).  d_accum is DEVICE memory of rows*W*4 floats.
 * d_accum8 (nullable, device, rows*W*4 uint32) accumulates the per-frame GL
 * unorm8 quantisation of the same colours — the reference screenshot path
 * (rayTracing.cpp:217-238).  `stream` is a hipStream_t (NULL = default);
 * the call is asynchronous like glDispatchCompute.  uniforms->basicShading != 0
 * selects the one-ray preview (traceBasic, compute.glsl:565-645 and the
 * basicShading branch of main, :672-678): deterministic, no jitter, no
 * tonemap; numRaysPerPixel is then ignored. */
int rt2_render(rt2_scene* scene, const rt2_uniforms* uniforms,
               uint32_t frame_begin, uint32_t frame_count, rt2_shard shard,
               float* d_accum, uint32_t* d_accum8, void* stream);

/* Blocking convenience wrapper — the readback half of screenshot()
 * (glReadPixels, rayTracing.cpp:217): renders into device buffers the scene
 * keeps between calls (allocated on first use, freed by rt2_scene_destroy), on
 * a stream of its own, and copies the resolved mean image back to host memory;
 * it waits for that stream only.  out_rgba (nullable):
 * rows*W*4 floats, mean over the frames (alpha = 1), slab-row order, slab row
 * 0 = lowest image row (GL convention, row 0 = bottom).  out_rgb8 (nullable):
 * rows*W*3 bytes, the reference's 8-bit screenshot average
 * (rayTracing.cpp:248-250), NOT flipped. */
int rt2_render_host(rt2_scene* scene, const rt2_uniforms* uniforms,
                    uint32_t frame_begin, uint32_t frame_count, rt2_shard shard,
                    float* out_rgba, uint8_t* out_rgb8);

/* Device resolve: out[i] = accum[i] / frames (rgb), alpha = 1.  Async. */
int rt2_resolve_rgba32f(const float* d_accum, int64_t n_pixels, uint32_t frames,
                        float* d_out, void* stream);
/* Host resolve of the 8-bit reference path (rayTracing.cpp:248-250):
 * u8(min(255, float(sum)/frames)) per channel, rgba sums -> rgb bytes. */
int rt2_resolve_rgb8_reference(const uint32_t* accum8, int64_t n_pixels, uint32_t frames,
                               uint8_t* out_rgb);

/* ------------------------------------------------------------------------
 * (1a) Ray queries: the closest hit of a caller's rays
 *
 * hits[i] is the result of calculateRayCollision for ray i over the scene's
 * triangles as uploaded (indices are those of the `tris` array given to
 * rt2_scene_create), with rayTriangleIntersect (compute.glsl:302-340)
 * verbatim and the scan started at best = bound_i:
 *   - bound_i = tmax when 0 < tmax < 1e38f, otherwise 1e38f: zero, negative,
 *     NaN and infinite tmax mean unbounded, so a zero-filled field gives the
 *     reference behaviour.  A hit needs dst < bound_i (strict);
 *   - on a miss tri = -1 and dst = bound_i;
 *   - d need not be normalised; o and d may be any floats.  Non-finite
 *     components give what the reference arithmetic gives, a miss, and do not
 *     disturb the other rays of the call;
 *   - RT2_TRAVERSAL_BRUTE: exact distance ties go to the lowest index.
 *     RT2_TRAVERSAL_BVH: they resolve in the reference's visiting order
 *     (calculateRayCollisionBVH, compute.glsl:410-460, started at best =
 *     bound_i; needs `nodes` at rt2_scene_create).
 * rt2_trace_rays reads d_rays and writes d_hits in DEVICE memory (n records
 * each, d_rays aligned to 16 bytes and d_hits to 8, as any hipMalloc'ed array
 * is) and is asynchronous on `stream` like rt2_render; it is ordered against
 * the scene's other launches by the rule renders follow (a launch waits for
 * the scene's previous one on any stream).  n == 0 returns 0 and launches
 * nothing.  Bad arguments (a null scene, n < 0, a null or misaligned pointer
 * with n > 0, unknown flag bits, BVH traversal on a scene without nodes)
 * return < 0 before any device call.
 * rt2_scene_stats counts a query as segments += n; tests and node_visits as
 * for renders (brute force: segments * N; BVH: leaf tests and nodes popped).
 * flags: RT2_TRACE_AUTO lets the launcher choose the kernel (the matrix-core
 * filter for brute force wherever the scene is in its range);
 * RT2_TRACE_SCALAR forces the one-thread-per-ray kernel for brute force, for
 * A/B comparison and cross-checks.  Every choice gives the same bits.
 * rt2_trace_rays_host is the blocking form over host arrays (no alignment
 * requirement): its device staging buffers are kept by the scene between
 * calls and freed by rt2_scene_destroy, like rt2_render_host's.
 * ---------------------------------------------------------------------- */
typedef struct rt2_ray { float o[3]; float tmax; float d[3]; float pad; } rt2_ray;   /* 32 B */
typedef struct rt2_hit { float dst; int32_t tri; } rt2_hit;                          /*  8 B */
enum { RT2_TRACE_AUTO = 0, RT2_TRACE_SCALAR = 1 };

int rt2_trace_rays(rt2_scene* scene, const rt2_ray* d_rays, int64_t n, rt2_hit* d_hits, int flags, void* stream);
int rt2_trace_rays_host(rt2_scene* scene, const rt2_ray* rays, int64_t n, rt2_hit* hits, int flags);

/* ------------------------------------------------------------------------
 * (1a') Occlusion queries: is anything in front of a caller's ray?
 *
 * occluded[i] is 1 when rt2_trace_rays on the same scene, traversal and ray
 * would return tri >= 0, and 0 otherwise; no other byte value is written and
 * no byte outside [0, n) is written:
 *   - bound_i is as in (1a): tmax when 0 < tmax < 1e38f, otherwise 1e38f, so
 *     a zero-filled field means unbounded.  The comparison is strict;
 *   - RT2_TRAVERSAL_BRUTE: some triangle of the array as uploaded has
 *     rayTriangleIntersect (compute.glsl:302-340) hit with dst < bound_i;
 *   - RT2_TRAVERSAL_BVH: calculateRayCollisionBVH (compute.glsl:410-460)
 *     started at best = bound_i accepts some hit (needs `nodes` at
 *     rt2_scene_create).  The definition is the walk's, not the array scan's:
 *     on trees whose boxes do not enclose their triangles the two can differ;
 *   - the query stops at a ray's first accepted hit.  That is exact: until the
 *     first accept the closest-hit scan's best is still bound_i, and after it
 *     tri never returns to -1;
 *   - d need not be normalised; o and d may be any floats.  A ray with a
 *     non-finite component is unoccluded and does not disturb the other rays
 *     of the call.
 * rt2_occluded reads d_rays and writes d_occluded in DEVICE memory (n records
 * and n bytes; d_rays aligned to 16 bytes, d_occluded with no alignment
 * requirement) and is asynchronous on `stream`; its ordering against the
 * scene's other launches is rt2_trace_rays'.  n == 0 returns 0 and launches
 * nothing.  Bad arguments (a null scene, n < 0, a null pointer with n > 0, a
 * misaligned d_rays, unknown flag bits, BVH traversal on a scene without
 * nodes) return < 0 before any device call.
 * rt2_scene_stats counts a query as segments += n.  Brute force: tests is the
 * nominal segments * N, as for every brute-force launch, not the tests an
 * early exit left undone.  BVH: tests and node_visits count what the walk did
 * up to its exit.
 * flags: RT2_TRACE_AUTO and RT2_TRACE_SCALAR, with the meaning they have for
 * rt2_trace_rays.  Every choice gives the same bytes.
 * rt2_occluded_host is the blocking form over host arrays: its device staging
 * buffers are kept by the scene between calls and freed by rt2_scene_destroy.
 * ---------------------------------------------------------------------- */
int rt2_occluded(rt2_scene* scene, const rt2_ray* d_rays, int64_t n, uint8_t* d_occluded, int flags, void* stream);
int rt2_occluded_host(rt2_scene* scene, const rt2_ray* rays, int64_t n, uint8_t* occluded, int flags);

/* ------------------------------------------------------------------------
 * (1a'') Surface queries: what is at the closest hit of a caller's rays
 *
 * out[i] is the reference's HitInfo (compute.glsl:97-106) at ray i's closest
 * hit, plus the surface's base colour:
 *   - dst and tri are exactly what rt2_trace_rays returns for the same scene,
 *     traversal, flags and ray: the tmax rule of (1a), the strict comparison,
 *     the ties, the BVH visiting order and the treatment of non-finite rays.
 * On a hit:
 *   - mtl = tris[tri].materialIndex and mtl_type = mats[mtl].materialType;
 *   - normal = normalize(cross(b - a, c - a)), the value the renderer scatters
 *     about (compute.glsl:331): one bit pattern per triangle, whatever the
 *     ray.  rayTriangleIntersect culls back faces (det < 0 is no hit), so
 *     dot(normal, d) < 0 at every hit: the normal always faces the ray;
 *   - u, v are the barycentrics of rayTriangleIntersect (compute.glsl:
 *     322-337) with the test's own arithmetic, as getTriangleTextureColor
 *     recomputes them: inv = 1 / det, u = -U * inv, v = V * inv, the weights
 *     of b and c; the weight of a is 1 - u - v (HitInfo.baryCoord is
 *     (1 - u - v, u, v)).  u >= 0, v >= 0 and 1 - u - v >= 0 hold exactly in
 *     binary32 (the test accepted them).  The reference's own texture lookup
 *     pairs them otherwise, uv = aTex * u + bTex * v + cTex * (1 - u - v)
 *     (compute.glsl:342-347); albedo follows the reference there;
 *   - albedo is what traceBasic (compute.glsl:565-645) returns for this ray
 *     with maxBounceCount = 1 and basicShadingShadow = 0: material.color for
 *     DIFFUSE, SPECULAR and GLASS; the sampled texel for TEXTURE
 *     (getTriangleTextureColor at the ray's own o, d); 0 or 1 for CHECKER,
 *     evaluated at hitPoint - normal * 1e-4; normalizeColor(emissionColor)
 *     for LIGHT (divided by its largest component only when that exceeds 1);
 *     black for GLASS_HIGHLIGHT; magenta (1, 0, 1) for any other type.
 *     A ray query has no uniforms: the reference's numTextures is taken as
 *     the number of images given to rt2_scene_set_textures, at most 5 (the
 *     shader's units), so a textureIndex at or above it reads black.
 * On a miss tri = mtl = mtl_type = -1, dst = bound_i, and normal, u, albedo
 * and v are +0.0: there is no sky colour without uniforms.
 * rt2_surface_rays reads d_rays and writes d_out in DEVICE memory (n records
 * each, both aligned to 16 bytes, as any hipMalloc'ed array is), nothing
 * outside records [0, n), and is asynchronous on `stream`; its ordering
 * against the scene's other launches is rt2_trace_rays'.  n == 0 returns 0
 * and launches nothing.  Bad arguments (a null scene, n < 0, a null or
 * misaligned pointer with n > 0, unknown flag bits, BVH traversal on a scene
 * without nodes) return < 0 before any device call.  rt2_scene_stats counts
 * it as it counts rt2_trace_rays.
 * flags: RT2_TRACE_AUTO and RT2_TRACE_SCALAR, with the meaning they have for
 * rt2_trace_rays.  Every choice gives the same bytes.
 * rt2_surface_rays_host is the blocking form over host arrays (no alignment
 * requirement): its device staging buffers are kept by the scene between
 * calls and freed by rt2_scene_destroy.
 *
 * rt2_camera_rays writes the deterministic primary ray of every pixel of the
 * shard's slab, in slab-row order (rt2_shard_rows(height, shard) * width
 * records, DEVICE memory aligned to 16 bytes): o = cameraPos, d =
 * normalize(viewportFront + viewportRight * x + viewportUp * y) with x =
 * float(2 * px - width) / width and y likewise from the image row: main's
 * basicShading branch (compute.glsl:665-676), evaluated as the preview
 * evaluates it, so the bits are the preview's rays'.  tmax = 0 (unbounded)
 * and pad = 0.  The jittered rays of the path tracer are not offered.  One
 * small launch, asynchronous on `stream`; it reads nothing of the scene but
 * its device and does not count in rt2_scene_stats.  Bad arguments (a null
 * scene or uniforms, zero width or height, a bad shard, a null or misaligned
 * d_rays for a non-empty slab) return < 0 before any device call.
 * rt2_camera_rays_host is the blocking form into a host array.
 * ---------------------------------------------------------------------- */
typedef struct rt2_surface {          /* 48 B, three 16-B stores per ray */
    float dst; int32_t tri; int32_t mtl; int32_t mtl_type;
    float normal[3]; float u;
    float albedo[3]; float v;
} rt2_surface;

int rt2_surface_rays(rt2_scene* scene, const rt2_ray* d_rays, int64_t n, rt2_surface* d_out, int flags, void* stream);
int rt2_surface_rays_host(rt2_scene* scene, const rt2_ray* rays, int64_t n, rt2_surface* out, int flags);
int rt2_camera_rays(rt2_scene* scene, const rt2_uniforms* uniforms, rt2_shard shard, rt2_ray* d_rays, void* stream);
int rt2_camera_rays_host(rt2_scene* scene, const rt2_uniforms* uniforms, rt2_shard shard, rt2_ray* rays);

/* ------------------------------------------------------------------------
 * (1a''') Preview shading queries: traceBasic for a caller's rays
 *
 * out[i].rgb is what the reference's preview shader traceBasic (compute.glsl:
 * 565-645) returns for Ray(o_i, d_i) over the scene as uploaded, with
 * insideGlass = false at the start, evaluated exactly as the preview render
 * (rt2_render with basicShading != 0) evaluates it: up to max_bounce segments
 * through mirrors, glass and the pass-through highlight type; a colour from
 * diffuse, checker, texture, light and sky; with `shadow` set, one shadow ray
 * from a diffuse, checker or texture end towards `light`.  No RNG.
 *   - d is used as given and is not normalised (rt2_camera_rays gives the
 *     preview's own normalised directions);
 *   - out[i].segments is the number of closest-hit searches the ray cost, the
 *     bounces plus the shadow ray: what the preview render adds to the scene's
 *     segment counter per pixel and frame;
 *   - rt2_ray.tmax is NOT used, unlike in every other query: each segment of
 *     traceBasic is unbounded, so the output does not depend on the field;
 *   - numTextures follows the rule of rt2_surface_rays: the number of images
 *     given to rt2_scene_set_textures, at most 5;
 *   - RT2_TRAVERSAL_BRUTE and _BVH have the closest-hit queries' meaning, for
 *     the bounce segments and for the shadow ray alike;
 *   - o and d may be any floats.  A non-finite component gives that ray what
 *     the preview's arithmetic gives and does not disturb the other rays.
 * rt2_shade_rays reads d_rays and writes d_out in DEVICE memory (n records
 * each, both aligned to 16 bytes), nothing outside records [0, n), and is
 * asynchronous on `stream`; its ordering against the scene's other launches is
 * rt2_trace_rays'.  n == 0 returns 0 and launches nothing.  Bad arguments (a
 * null scene or opts, n < 0, a null or misaligned pointer with n > 0, non-zero
 * pad, max_bounce outside 1 .. 256, unknown flag bits, BVH traversal on a
 * scene without nodes) return < 0 before any device call.
 * rt2_scene_stats: segments grows by the sum of out[i].segments.  Brute force:
 * tests is the nominal segments * N.  BVH: tests and node_visits count what
 * the walks did, the shadow rays' included (leaf tests and nodes popped).
 * flags: RT2_TRACE_AUTO and RT2_TRACE_SCALAR, with the meaning they have for
 * rt2_trace_rays.  Every choice gives the same bytes.
 * rt2_shade_rays_host is the blocking form over host arrays (no alignment
 * requirement): its device staging buffers are kept by the scene between
 * calls and freed by rt2_scene_destroy.
 * ---------------------------------------------------------------------- */
typedef struct rt2_shade_opts {   /* 32 B */
    float   light[3];    /* basicShadingLightPosition.xyz */
    int32_t shadow;      /* basicShadingShadow: 0 = none, non-zero = shadow ray */
    int32_t max_bounce;  /* maxBounceCount, 1 .. 256 */
    int32_t pad[3];      /* must be 0 */
} rt2_shade_opts;
typedef struct rt2_shaded { float rgb[3]; int32_t segments; } rt2_shaded;   /* 16 B, one store */

int rt2_shade_rays(rt2_scene* scene, const rt2_ray* d_rays, int64_t n, const rt2_shade_opts* opts,
                   rt2_shaded* d_out, int flags, void* stream);
int rt2_shade_rays_host(rt2_scene* scene, const rt2_ray* rays, int64_t n, const rt2_shade_opts* opts,
                        rt2_shaded* out, int flags);

/* ------------------------------------------------------------------------
 * (1a'''') Radiance queries: the path tracer's trace() for a caller's rays
 *
 * out[i].rgb is what the reference's Monte-Carlo path tracer trace()
 * (compute.glsl:472-563) returns for Ray(o_i, d_i, insideGlass = false) with
 * rngState = rng[i] over the scene as uploaded, maxBounceCount and
 * environmentalLight taken from opts, evaluated exactly as rt2_render
 * evaluates it: the scatter on diffuse, texture, specular, checker and glass,
 * the return on a light, magenta for every other type (GLASS_HIGHLIGHT
 * included), the isEdgeHighlight pass-through after the first bounce, the
 * roulette, and the sky on a miss when environmental_light is set.  It is the
 * value the render adds to colorCumulative (:692): linear, before the mean
 * over numRaysPerPixel, the tonemap and the sRGB encoding.
 *   - on return rng[i] holds the stream's state after the path's last draw:
 *     what `seed` holds after trace(rayJittered, seed), so a caller can go on
 *     drawing from it;
 *   - out[i].segments is the number of closest-hit searches: the bounces
 *     traced;
 *   - d is used as given and is not normalised;
 *   - rt2_ray.tmax is NOT used, as in rt2_shade_rays: every segment of trace
 *     is unbounded;
 *   - numTextures follows the rule of rt2_surface_rays;
 *   - RT2_TRAVERSAL_BRUTE and _BVH have the closest-hit queries' meaning;
 *   - o and d may be any floats.  A non-finite component gives that ray what
 *     the render's arithmetic gives and does not disturb the other rays.
 * rt2_radiance_rays reads d_rays, reads and writes d_rng and writes d_out in
 * DEVICE memory (n records each; rays and records aligned to 16 bytes, rng to
 * 4), nothing outside records [0, n), and is asynchronous on `stream`; its
 * ordering against the scene's other launches is rt2_trace_rays'.  n == 0
 * returns 0 and launches nothing.  Bad arguments (a null scene or opts, n < 0,
 * a null or misaligned pointer with n > 0, non-zero pad, max_bounce outside
 * 1 .. 256, unknown flag bits, BVH traversal on a scene without nodes) return
 * < 0 before any device call.
 * rt2_scene_stats: segments grows by the sum of out[i].segments.  Brute force:
 * tests is the nominal segments * N.  BVH: tests and node_visits count what
 * the walks did.
 * flags: RT2_TRACE_AUTO and RT2_TRACE_SCALAR, with the meaning they have for
 * rt2_trace_rays.  Every choice gives the same bytes.
 * rt2_radiance_rays_host is the blocking form over host arrays (no alignment
 * requirement; rng is copied in and out): its device staging buffers are kept
 * by the scene between calls and freed by rt2_scene_destroy.
 *
 * rt2_path_rays is the path tracer's camera: for every pixel of the shard's
 * slab, in slab-row order (rt2_shard_rows(height, shard) * width records), it
 * sets rng[i] = x + y * width + frame_index * 968824447u (compute.glsl:668,
 * 32-bit) when reseed != 0 and uses rng[i] as found otherwise, then executes
 * compute.glsl:686-690 as the render does: one draw for the defocus-disk
 * angle (with the pinned cos and sin), two jitter draws, o = cameraPos +
 * defocusDiskRight * cos + defocusDiskUp * sin, d = normalize(endPointJittered
 * - o), tmax = 0 and pad = 0; rng[i] is left at the state after those three
 * draws.  Alternating rt2_path_rays (reseed on the first sample only) and
 * rt2_radiance_rays numRaysPerPixel times reproduces the render's per-pixel
 * sample sequence exactly.  One small launch, asynchronous on `stream`; it
 * reads nothing of the scene but its device and does not count in
 * rt2_scene_stats.  Bad arguments are rt2_camera_rays' and a null or
 * misaligned d_rng for a non-empty slab.  rt2_path_rays_host is the blocking
 * form over host arrays.
 * ---------------------------------------------------------------------- */
typedef struct rt2_path_opts {   /* 16 B */
    int32_t max_bounce;           /* maxBounceCount, 1 .. 256 */
    int32_t environmental_light;  /* environmentalLight: 0 = black sky */
    int32_t pad[2];               /* must be 0 */
} rt2_path_opts;
typedef struct rt2_radiance { float rgb[3]; int32_t segments; } rt2_radiance;   /* 16 B, one store */

int rt2_radiance_rays(rt2_scene* scene, const rt2_ray* d_rays, int64_t n, const rt2_path_opts* opts,
                      uint32_t* d_rng, rt2_radiance* d_out, int flags, void* stream);
int rt2_radiance_rays_host(rt2_scene* scene, const rt2_ray* rays, int64_t n, const rt2_path_opts* opts,
                           uint32_t* rng, rt2_radiance* out, int flags);
int rt2_path_rays(rt2_scene* scene, const rt2_uniforms* uniforms, rt2_shard shard, uint32_t frame_index, int reseed,
                  uint32_t* d_rng, rt2_ray* d_rays, void* stream);
int rt2_path_rays_host(rt2_scene* scene, const rt2_uniforms* uniforms, rt2_shard shard, uint32_t frame_index,
                       int reseed, uint32_t* rng, rt2_ray* rays);

/* ------------------------------------------------------------------------
 * (1a-6) Linear renders: rt2_render's paths, HDR sums and second moments
 *
 * rt2_render_linear is rt2_render with another sink: the same pixels, frames,
 * seeds, draws and trace() calls on the same kernels' schedule, but what it
 * accumulates is the frame's linear mean, before aces1 and srgb1, and
 * (optionally) the mean of the samples' squares.  For every pixel p of the
 * shard's slab (slab-row order, as rt2_render) and every frame f = frame_begin
 * + i, in increasing i:
 *   - seed = x + y * width + f * 968824447u, and for sample s = 0 .. R-1 (R =
 *     numRaysPerPixel) the jittered ray and v_s = trace(ray, seed) exactly as
 *     in rt2_render: the same draws in the same order;
 *   - from c = q = (0,0,0), per channel and in sample order, c = c + v_s and
 *     q = q + v_s * v_s: the product is rounded to binary32, then the sum (no
 *     fused multiply-add);
 *   - m = c / (float)R and m2 = q / (float)R (IEEE division, the render's own);
 *   - d_sum[4*p + ch] += m[ch] and, when d_sumsq is not NULL,
 *     d_sumsq[4*p + ch] += m2[ch] (ch = 0, 1, 2); the fourth float of both
 *     records is written 0.0f, as rt2_render writes its accumulator's.
 * Frames are added in increasing order, so splitting them over several calls
 * gives identical bits; rt2_scene_set_frame_split, _set_cost_order,
 * _set_variant and _set_traversal change nothing in the result.
 * d_sum and d_sumsq are DEVICE memory of rows * width * 4 floats, aligned to
 * 16 bytes.  The call is asynchronous on `stream` and ordered against the
 * scene's other launches as renders are.  rt2_scene_stats counts it exactly as
 * it counts rt2_render (samples, segments, tests, node_visits);
 * uniforms->numTextures is used as rt2_render uses it; maxBounceCount <= 0
 * adds sums of 0, as the render's trace() returns 0.
 * The kernel is the linear twin of the variant rt2_render would launch for the
 * same call (the same selection, the same rt2_scene_set_variant rules applied
 * to the id the caller set): rt2_scene_diag reports the variant's id + 1000
 * (1136 for the automatic 0) and rt2_variant_name gives the parent's name with
 * "/lin" appended.  A forced variant without a twin (experiment builds) falls
 * back to the automatic choice.  A twin's id is not accepted by
 * rt2_scene_set_variant.
 * Bad arguments return < 0 before any device call: a null scene, uniforms or
 * d_sum; d_sum or d_sumsq not aligned to 16 bytes; numRaysPerPixel < 1; zero
 * width or height; a bad shard; basicShading != 0 (the preview has no
 * tonemap: rt2_render already gives its linear value).  frame_count == 0 or
 * an empty slab returns 0 and launches nothing.
 *
 * rt2_render_linear_host is the blocking form, like rt2_render_host: it
 * renders into device buffers the scene keeps (freed by rt2_scene_destroy) on
 * the scene's own stream and returns out_mean[4*p + ch] = sum / frames and,
 * when out_meansq is not NULL, out_meansq[4*p + ch] = sumsq / frames
 * (rt2_resolve_rgba32f's division, alpha = 1, slab-row order; host arrays of
 * rows * width * 4 floats, no alignment requirement).
 *
 * rt2_resolve_tonemap is the device resolve from a linear sum to the render's
 * display value: out[4*i + ch] = srgb1(aces1(d_linear_sum[4*i + ch] / frames))
 * with the render's pinned aces1 and srgb1, alpha = 1.  For a one-frame linear
 * sum (frames = 1) this is bit for bit the pixel rt2_render adds to its
 * accumulator for that frame.  Asynchronous; in place (d_out == d_linear_sum)
 * is allowed.  Bad arguments as rt2_resolve_rgba32f (a null pointer,
 * n_pixels < 0, frames == 0).
 * A sum no render produces (a denoiser's output, say) gets what the formula
 * gives in binary32, x = sum / frames, aces1(x) = clamp((x (2.51 x + 0.03)) /
 * (x (2.43 x + 0.59) + 0.14), 0, 1) with a clamp that ignores a NaN operand:
 *   - NaN, +inf and -inf give 0 (the quotient is NaN, and clamp(NaN) = 0);
 *   - x up to 1.1643e19, where x (2.51 x + 0.03) overflows, gives 1 (1e6 does),
 *     and so does x up to 1.1834e19, where inf / finite = inf clamps to 1;
 *     from there on both products overflow, inf / inf = NaN, and the result is
 *     0 — as for |x| beyond it on the negative side;
 *   - a negative x follows the rational, whose denominator never vanishes:
 *     -0.01195 < x <= -0 gives 0, below that the value is positive again and
 *     reaches 1 at x = -0.2418 (x = -5 gives 1).
 * A caller who wants another answer for such values clamps them first.
 * (tests/test_gpu_numerics.py, tests/test_numerics_cases.py.)
 * ---------------------------------------------------------------------- */
int rt2_render_linear(rt2_scene* scene, const rt2_uniforms* uniforms, uint32_t frame_begin, uint32_t frame_count,
                      rt2_shard shard, float* d_sum, float* d_sumsq, void* stream);
int rt2_render_linear_host(rt2_scene* scene, const rt2_uniforms* uniforms, uint32_t frame_begin,
                           uint32_t frame_count, rt2_shard shard, float* out_mean, float* out_meansq);
int rt2_resolve_tonemap(const float* d_linear_sum, int64_t n_pixels, uint32_t frames, float* d_out, void* stream);

/* ------------------------------------------------------------------------
 * (1b) Multi-GPU: row-tile shards + one RCCL gather
 *
 * The reference renders on one GPU and reads the framebuffer back with
 * glReadPixels inside screenshot() (rayTracing.cpp:124-283, :217).  With N
 * ranks (one process per GPU), rank r renders the rows of rt2_shard
 * {tile_rows, r, N} and ONE ncclGather (RCCL over xGMI) brings the resolved
 * slabs to the root, which un-interleaves them: bit-identical to one GPU.
 *
 * Failure contract (raytracing2-fork_amd/csrc/device/rt2_comm_protocol.h):
 * every rank issues the same collectives in the same order.  A rank-local
 * failure (arguments, a shard that does not match the communicator, device
 * memory, a failed render) is decided by an agreement step — a 2-int
 * ncclAllReduce(max) read back on the host — before any gather, so every
 * rank returns < 0 and no gather is issued.  A rank that cannot take part in
 * an agreement (its communicator was aborted, the agreement's own copy or
 * allreduce fails) aborts and returns; its peers wait for it at most
 * RT2_COMM_TIMEOUT_S seconds (default 600; every host wait on a collective is
 * a poll of the stream and ncclCommGetAsyncError with that deadline), then
 * abort their communicator and return < 0.  An aborted owned communicator is
 * unusable: destroy it.  A wrapped communicator is never aborted here (its
 * owner must abort it); the handle only refuses further use.
 * RT2_FAULT_AT=<site>[@rank] injects a failure (tests only; sites
 * gather.prepare, gather.issue, check, render, agree.copy).
 * ---------------------------------------------------------------------- */
#define RT2_COMM_ID_BYTES 128 /* sizeof(ncclUniqueId) */
typedef struct rt2_comm rt2_comm;

/* ncclGetUniqueId: called once (by the root); the bytes travel to the other
 * ranks by any channel (a file, a socket, an MPI broadcast). */
int rt2_comm_unique_id(uint8_t* id /* RT2_COMM_ID_BYTES */);
/* ncclCommInitRank on `device` (blocks until all nranks have joined). */
int rt2_comm_init(const uint8_t* id, int32_t nranks, int32_t rank, int32_t device, rt2_comm** out);
/* Uses a caller-owned ncclComm_t (not destroyed by rt2_comm_destroy). */
int rt2_comm_wrap(void* nccl_comm, int32_t device, rt2_comm** out);
void rt2_comm_destroy(rt2_comm* comm);
int rt2_comm_size(rt2_comm* comm, int32_t* nranks, int32_t* rank);
/* ncclCommGetAsyncError: < 0 (with rt2_last_error) if a collective failed. */
int rt2_comm_check(rt2_comm* comm);

/* Gathers every rank's slab — rt2_shard_rows(height, shard) rows of `width`
 * 16-byte pixels (an rgba32f image or the uint32x4 8-bit sums), device memory —
 * to `root` with one ncclGather and un-interleaves it there into d_image
 * (height*width pixels, device; ignored on other ranks).  shard.rank/nranks
 * must be the communicator's.  The host first waits for the work already
 * queued on `stream` (this rank's render: no peer is involved, so no deadline
 * applies; bounded at 20 x RT2_COMM_TIMEOUT_S, and twice its duration is added
 * to the deadlines that follow), then the ranks agree that each of them can
 * take part (one agreement step on the communicator's own stream, which could
 * not start on a device still busy with the render); the gather and the
 * un-interleave are then asynchronous on `stream`.  A local failure (a root without d_image, a
 * shard that does not match, no device memory) makes every rank return < 0
 * with nothing issued.  Once the gather is queued, a peer that fails inside
 * it (ncclCommAbort does not release ranks already in the collective) leaves
 * `stream` waiting: wait for it with rt2_comm_wait, not an unbounded
 * hipStreamSynchronize. */
int rt2_gather_slabs(rt2_comm* comm, const void* d_slab, int32_t width, int32_t height, rt2_shard shard,
                     int32_t root, void* d_image, void* stream);
/* The host waits for `stream` (e.g. rt2_gather_slabs' gather) under the
 * RT2_COMM_TIMEOUT_S deadline, polling ncclCommGetAsyncError: 0 when it has
 * drained; on a timeout, an RCCL error or a stream error the communicator is
 * aborted as above and < 0 returned (replaces the caller's
 * hipStreamSynchronize / cudaStreamSynchronize after the collective).  When
 * the last rt2_gather_slabs of this communicator was queued on `stream`, the
 * work queued before that gather (already waited for by rt2_gather_slabs) is
 * excluded from the deadline in the same way. */
int rt2_comm_wait(rt2_comm* comm, void* stream);
/* The root's un-interleave alone: d_gathered = [nranks][max_rows][width]
 * 16-byte pixels (rank-major slabs, padded to max_rows rows) -> d_image
 * [height][width] for the tile layout {tile_rows, -, nranks}.  Async. */
int rt2_unshard_slabs(const void* d_gathered, int32_t max_rows, int32_t width, int32_t height, rt2_shard layout,
                      void* d_image, void* stream);
/* rt2_render_host across ranks: every rank renders its shard, the resolved
 * slabs (and, if out_rgb8, the 8-bit sums) are gathered to `root`, which
 * receives the whole image in out_rgba (height*width*4 floats) / out_rgb8
 * (height*width*3 bytes, not flipped); other ranks' output pointers are
 * ignored.  Blocking; every rank must call it.  The 8-bit sums are accumulated
 * and gathered when ANY rank passes out_rgb8 (so ranks may pass different
 * pointers), and the ranks agree before the gather that every one of them
 * rendered (two agreement steps): a rank-local failure makes every rank
 * return < 0 ("a peer rank failed") instead of leaving peers blocked in the
 * gather.  The host waits for the gathers under the RT2_COMM_TIMEOUT_S
 * deadline before the root copies the image out. */
int rt2_render_host_gather(rt2_scene* scene, const rt2_uniforms* uniforms, uint32_t frame_begin,
                           uint32_t frame_count, rt2_shard shard, rt2_comm* comm, int32_t root,
                           float* out_rgba, uint8_t* out_rgb8);

/* Counters of the renders issued on this scene since the last reset
 * (synchronises the scene's device). */
int rt2_scene_stats(rt2_scene* scene, rt2_stats* out, int reset);

/* Kernel-variant control for experiments: 0 = auto.  Returns the variant the
 * next render will use for this scene. */
int rt2_scene_set_variant(rt2_scene* scene, int variant);

/* Closest-hit algorithm.  BRUTE (default): every triangle in array order, the
 * north-star kernel.  BVH: the reference's own traversal of the node array
 * (calculateRayCollisionBVH, compute.glsl:410-460; needs `nodes` at
 * rt2_scene_create) — identical to BRUTE except on exact distance ties, where
 * it resolves in the reference's visiting order. */
enum { RT2_TRAVERSAL_BRUTE = 0, RT2_TRAVERSAL_BVH = 1 };
int rt2_scene_set_traversal(rt2_scene* scene, int traversal);

/* Work-item shape for frame_count > 1 (default 1): the render hands out
 * (frame, pixel) items frame-major and adds the frames in order afterwards,
 * instead of one whole pixel (all frames) per item — a shorter tail at the end
 * of each launch.  Results are bit-identical either way; costs
 * frame_count * pixels * 16 B of device scratch per scene. */
int rt2_scene_set_frame_split(rt2_scene* scene, int enable);

/* Work-item order (default 0 = raster order): when enabled, each render
 * records a per-pixel cost map of the scene's slab (item time in shader
 * clocks) and the next render of the same slab hands out runs of 64
 * neighbouring pixels most-expensive-first (a GPU counting sort), so the last
 * items of a launch are cheap ones — the reference's progressive renders of
 * one view repeat the same per-pixel costs.  Measured: −7 % time on config E
 * (heavy-tailed mirror paths), neutral to −2 % elsewhere.  Results are
 * bit-identical in any order.  Renders of one scene are always ordered among
 * themselves (a render waits for the scene's previous one on any stream). */
int rt2_scene_set_cost_order(rt2_scene* scene, int enable);

/* Replaces binding the loader's textures to units 0..4 (rayTracing.cpp:
 * 1315-1320; Texture2D(path), textureClass.cpp:55-104): the images are copied
 * to HBM as RGBA8 with GL's unpack of GL_RED/GL_RG/GL_RGB/GL_RGBA bytes
 * (4-byte row alignment, GL_UNPACK_ALIGNMENT's default) and the 1-channel
 * swizzle (r, r, r, 1).  TEXTURE materials then sample texture
 * `textureIndex` with GL_LINEAR + GL_REPEAT (getTriangleTextureColor,
 * compute.glsl:342-368): black when textureIndex is outside [0,
 * uniforms->numTextures), magenta for an index >= 5 (the shader binds five
 * samplers), black for an index with no image here (an unbound unit).
 * n = 0 removes the textures. */
int rt2_scene_set_textures(rt2_scene* scene, const rt2_image* images, int32_t n);

/* ------------------------------------------------------------------------
 * (2) Host surface
 * ---------------------------------------------------------------------- */

/* Scene data under construction: the reference's rtxTriangles, bvhTriangles,
 * materials, texture list and BVH nodes (rayTracing.cpp:1256-1293). */
typedef struct rt2_scene_data rt2_scene_data;

rt2_scene_data* rt2_sd_create(void);
void rt2_sd_destroy(rt2_scene_data* sd);

/* getTrianglesData_ (mesh.h:279-613): first *.obj of the folder, every *.mtl
 * of the folder, every file of <folder>/textures decoded as a texture (in
 * directory order, flipped vertically on load, like Texture2D(path)).
 * Appends. */
int rt2_sd_load_obj_folder(rt2_scene_data* sd, const char* folder);
/* Decoded texture i of the scene data (pixels owned by sd) or < 0. */
int rt2_sd_texture(const rt2_scene_data* sd, int32_t i, rt2_image* out_view);

/* stbi_set_flip_vertically_on_load(flip); stbi_load(path, &w, &h, &n, 0)
 * (external/stb/stb_image.h v2.30 as Texture2D uses it), restated: PNG (all
 * depths/colour types, tRNS, interlace) and sequential-Huffman JPEG.  The
 * pixels are malloc'ed; release them with rt2_image_free. */
int rt2_image_load(const char* path, int32_t flip_vertically, rt2_image* out);
void rt2_image_free(rt2_image* image);
/* Appends one material; returns its index or < 0. */
int32_t rt2_sd_add_material(rt2_scene_data* sd, const rt2_material* m);
/* Appends one triangle (and its BVH triangle) as a builder would. */
int rt2_sd_add_triangle(rt2_scene_data* sd, const float a[3], const float b[3], const float c[3],
                        int32_t material_index);

/* Appends n complete triangle records (rtxTriangles.push_back). */
int rt2_sd_add_triangles(rt2_scene_data* sd, const rt2_triangle* tris, int32_t n);

/* Scene builders of rayTracing.cpp. */
int rt2_sd_add_cornell_box(rt2_scene_data* sd, float light_size, float pad, int32_t light_mtl,
                           int32_t light_enabled);                           /* :453-547 */
int rt2_sd_add_mirror_cornell_box(rt2_scene_data* sd, float light_size, float pad,
                                  int32_t light_mtl, int32_t mirror_mtl);    /* :569-664 */
int rt2_sd_add_side_lit_cornell_box(rt2_scene_data* sd, float light_size, float pad,
                                    int32_t light_mtl, int32_t wall_mtl, int32_t rotate); /* :690-847 */
int rt2_sd_add_sky_light_plane(rt2_scene_data* sd, int32_t light_mtl);       /* :388-432 */
int rt2_sd_add_cube(rt2_scene_data* sd, const float center[3], const float size[3],
                    const float rotation[3], int32_t mtl);                   /* :867-923 */
int rt2_sd_create_classic_cornell_box(rt2_scene_data* sd, float room, int32_t red, int32_t green,
                                      int32_t white, int32_t light);         /* :949-1041 */
int rt2_sd_create_diverse_cornell_box(rt2_scene_data* sd, float room, int32_t red, int32_t green,
                                      int32_t white, int32_t light, int32_t glass, int32_t mirror,
                                      int32_t checker, int32_t metal);       /* :1071-1118 */

/* BVH(bvhTriangles, rtxTriangles) (BVH.h:145-221): builds the node array and
 * reorders the triangles in place, exactly as the reference does. */
int rt2_sd_build_bvh(rt2_scene_data* sd);

int32_t rt2_sd_num_triangles(const rt2_scene_data* sd);
int32_t rt2_sd_num_materials(const rt2_scene_data* sd);
int32_t rt2_sd_num_nodes(const rt2_scene_data* sd);
int32_t rt2_sd_num_textures(const rt2_scene_data* sd);
const rt2_triangle* rt2_sd_triangles(const rt2_scene_data* sd);
const rt2_material* rt2_sd_materials(const rt2_scene_data* sd);
const rt2_node* rt2_sd_nodes(const rt2_scene_data* sd);
/* BVHTriangle min/max/center (mesh.h:141-154), 9 floats per triangle. */
int rt2_sd_bvh_triangles(const rt2_scene_data* sd, float* out9);
/* Texture file name i (directory order, mesh.h:305-318) or NULL. */
const char* rt2_sd_texture_name(const rt2_scene_data* sd, int32_t i);

/* Material helpers of mesh.h:47-102 (fields the reference leaves
 * uninitialised are zero here). */
void rt2_material_default(rt2_material* m);
void rt2_material_make_diffuse(rt2_material* m, float r, float g, float b);
void rt2_material_make_light(rt2_material* m, float r, float g, float b, float strength);
void rt2_material_make_specular(rt2_material* m, float r, float g, float b,
                                float sr, float sg, float sb, float smooth, float prob);
void rt2_material_make_checker(rt2_material* m, float scale);
void rt2_material_make_glass(rt2_material* m, float r, float g, float b, float ior);

/* Camera(...) + updateUniforms (camera.h:99-192): fills the eight camera
 * vec4s of `u` (other fields untouched). */
typedef struct rt2_camera {
    int32_t width, height;
    float position[3];
    float hfov, pitch, yaw;
    float focus_distance, defocus_angle, zoom;
} rt2_camera;
/* Reference defaults (rayTracing.cpp:82-89) for a width x height screen. */
void rt2_camera_default(rt2_camera* cam, int32_t width, int32_t height);
int rt2_camera_uniforms(const rt2_camera* cam, rt2_uniforms* u);
/* Offline-render uniforms (rayTracing.cpp:146-153 + :1386-1400). */
void rt2_uniforms_offline(rt2_uniforms* u, int32_t width, int32_t height, int32_t max_bounce,
                          int32_t rays_per_pixel, int32_t num_triangles, int32_t num_textures);

/* stbi_write_png surface (rayTracing.cpp:264): 8-bit, comps 1..4. */
int rt2_write_png(const char* path, int32_t w, int32_t h, int32_t comps, const uint8_t* data,
                  int32_t stride_bytes);

#ifdef __cplusplus
}
#endif

#endif /* RT2_H */
