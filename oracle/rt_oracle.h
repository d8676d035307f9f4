/*
 * rt_oracle.h — TEST INFRASTRUCTURE ONLY (see rt_oracle.c).  CPU restatement of
 * RayTracing/Assets/Shaders/compute.glsl.  Struct layouts mirror the
 * reference's host structs directly (not the product header), so the oracle
 * stays independent of the code it checks.
 */
#ifndef RT_ORACLE_H
#define RT_ORACLE_H

#include <stdint.h>

/* RTXTriangle, mesh.h:112-139 (80 B) */
typedef struct {
    float a[4], b[4], c[4];
    float aTex[2], bTex[2], cTex[2];
    int32_t materialIndex;
    float pad;
} oracle_triangle;

/* Material, mesh.h:26-103 (96 B) */
typedef struct {
    float color[4], specularColor[4], emissionColor[4];
    int32_t textureIndex;
    float emissionStrength, smoothness, specularProbability, checkerScale, refractiveIndex;
    int32_t materialType, index, isEdgeHighlight, pad1, pad2, pad3;
} oracle_material;

/* Node, BVH.h:54-65 (48 B) */
typedef struct {
    float bmin[3], pad0, bmax[3], pad1;
    int32_t triangleIndex, triangleCount, childIndex, pad;
} oracle_node;

/* GlobalUniforms, camera.h:10-36 (192 B) */
typedef struct {
    int32_t pad, numTextures;
    uint32_t width, height;
    int32_t numSpheres, numTriangles, basicShading, basicShadingShadow;
    float basicShadingLightPosition[4];
    int32_t environmentalLight, maxBounceCount, numRaysPerPixel;
    uint32_t frameIndex;
    float cameraPos[4], viewportRight[4], viewportUp[4], viewportFront[4];
    float pixelRight[4], pixelUp[4], defocusDiskRight[4], defocusDiskUp[4];
} oracle_uniforms;

#ifdef __cplusplus
extern "C" {
#endif

/* Renders frames [frame_begin, frame_begin+frame_count) of the listed image
 * rows (row 0 = bottom, as gl_GlobalInvocationID.y).  out_accum (nullable):
 * n_rows*W*4 floats, per-pixel SUM over frames in frame order (alpha = frame
 * count).  out_acc8 (nullable): n_rows*W*4 uint32 sums of the per-frame GL
 * unorm8 quantisation.  mode 0 = brute force, 1 = BVH (needs nodes). */
int oracle_render(const oracle_triangle* tris, int32_t n_tris, const oracle_material* mats, int32_t n_mats,
                  const oracle_node* nodes, int32_t n_nodes, const oracle_uniforms* u, uint32_t frame_begin,
                  uint32_t frame_count, const int32_t* rows, int32_t n_rows, int32_t mode, int32_t threads,
                  float* out_accum, uint32_t* out_acc8, uint64_t* out_segments, uint64_t* out_tests);

/* Same, over an arbitrary pixel list px = n_px (x, y) pairs; outputs are
 * n_px*4 in list order (bounded CPU samples of large configs). */
int oracle_render_pixels(const oracle_triangle* tris, int32_t n_tris, const oracle_material* mats, int32_t n_mats,
                         const oracle_node* nodes, int32_t n_nodes, const oracle_uniforms* u, uint32_t frame_begin,
                         uint32_t frame_count, const int32_t* px, int64_t n_px, int32_t mode, int32_t threads,
                         float* out_accum, uint32_t* out_acc8, uint64_t* out_segments, uint64_t* out_tests);

/* The closest hit of n rays (o, d: n * 3 floats), each scan started at
 * r.dst = bound[i]: mode 0 = the array scan, 1 = the BVH walk over `nodes`.
 * A miss keeps dst = bound[i] and tri = -1.  out_tests / out_visits
 * (nullable): per-ray leaf triangle tests and interior nodes popped. */
int oracle_closest_hits(const oracle_triangle* tris, int32_t n_tris, const oracle_node* nodes, int32_t n_nodes,
                        const float* o, const float* d, const float* bound, int64_t n, int32_t mode, float* out_dst,
                        int32_t* out_tri, uint64_t* out_tests, uint64_t* out_visits);

/* Textures for TEXTURE materials (global to the library): n stb-layout
 * images, whn = (width, height, channels) triples.  n = 0 clears. */
int oracle_set_textures(const int32_t* whn, const uint8_t* const* pixels, int32_t n);

uint32_t oracle_pcg_next(uint32_t* state, float* out);
int oracle_ray_triangle(const float o[3], const float d[3], const oracle_triangle* t, float* dst);
void oracle_sky(const float d[3], float out[3]);
float oracle_tonemap_srgb(float x);
float oracle_pinned(int which, float x);

/* One operation of DESIGN.md §Numerics on n rows, by this file's own dot, sky,
 * aces1 and the rest: in9 = n rows of 9 words, out4 = n rows of 4 words, all
 * binary32 bit patterns (NaN payloads, zero signs and RNG states kept).
 * Vectors take words 0-2 and 3-5, a trailing scalar word 6.  op:
 *    0 a/b   1 1/a   2 sqrt(a)   3 fma(a,b,c)   4 a*b   5 a+b   6 a-b
 *    7 fminf(a,b)   8 fmaxf(a,b)   9 clampf(x,lo,hi)
 *   10 dot   11 cross   12 length   13 normalize   14 reflect(I,N)
 *   15 refract_(I,N,eta): xyz + isRefracted   16 mixs(x,y,a)
 *   17 smoothstep(e0,e1,x)
 *   18 exp   19 log   20 acos   21 cos   22 sin   23 pow(a,b)   (rt2pm_*)
 *   24 aces1   25 srgb1   26 sky(dir)
 *   27 rnd(state): value, new state   28 rnd_dir(state): xyz + new state
 * The product's test hook rt2_device_numerics takes the same codes. */
int oracle_numerics(int32_t op, const uint32_t* in9, int64_t n, uint32_t* out4);

#ifdef __cplusplus
}
#endif

#endif
