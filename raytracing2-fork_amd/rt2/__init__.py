"""rt2 — Python mirror of the reference's render-path surface over the rt2 C-ABI.

The reference drives its renderer from C++ (RayTracing/src/rayTracing.cpp):
getTrianglesData_ -> material appends -> a Cornell builder -> BVH -> Camera ->
SSBO/UBO upload -> glDispatchCompute per frame -> readback/accumulate -> PNG.
This module exposes the same steps, with the same names and argument meaning,
over ``librt2.so`` (include/rt2.h):

    sd = SceneData()                          # rtxTriangles/bvhTriangles/materials
    sd.load_obj_folder(path)                  # getTrianglesData_   mesh.h:279
    red = sd.add_material(Material.diffuse((1, 0, 0)))
    sd.add_cornell_box(0.17, 0.3, light, True)  # addCornellBox    rayTracing.cpp:453
    sd.build_bvh()                            # BVH(bvh, rtx)       BVH.h:150
    u = offline_uniforms(W, H, bounces, rays, sd.num_triangles)
    scene = Scene(sd, device=0)               # SSBO uploads        rayTracing.cpp:1323
    img = scene.render_host(u, 0, frames)     # dispatch x frames + resolve

The render itself runs only on the HIP path: if librt2.so is missing or no
GPU is present the calls raise — there is no CPU fallback in this package.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# RT2_LIB=exp selects the experiment build (make EXPERIMENTS=1: the product
# kernels plus the A/B variants of DESIGN.md "Tried and measured").
LIB_PATH = os.path.join(_HERE, "librt2_exp.so" if os.environ.get("RT2_LIB") == "exp" else "librt2.so")

DIFFUSE, SPECULAR, LIGHT, CHECKER, GLASS, TEXTURE, GLASS_HIGHLIGHT = range(7)


class Vec4(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float), ("w", C.c_float)]


class Vec2(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float)]


class Triangle(C.Structure):  # RTXTriangle, mesh.h:112-139
    _fields_ = [("a", Vec4), ("b", Vec4), ("c", Vec4), ("aTex", Vec2), ("bTex", Vec2), ("cTex", Vec2),
                ("materialIndex", C.c_int32), ("pad", C.c_float)]


class Material(C.Structure):  # Material, mesh.h:26-103
    _fields_ = [("color", Vec4), ("specularColor", Vec4), ("emissionColor", Vec4),
                ("textureIndex", C.c_int32), ("emissionStrength", C.c_float), ("smoothness", C.c_float),
                ("specularProbability", C.c_float), ("checkerScale", C.c_float), ("refractiveIndex", C.c_float),
                ("materialType", C.c_int32), ("index", C.c_int32), ("isEdgeHighlight", C.c_int32),
                ("pad1", C.c_int32), ("pad2", C.c_int32), ("pad3", C.c_int32)]

    @staticmethod
    def default() -> "Material":
        m = Material()
        lib().rt2_material_default(C.byref(m))
        return m

    @staticmethod
    def diffuse(col) -> "Material":  # makeDiffusive, mesh.h:49-53
        m = Material.default()
        lib().rt2_material_make_diffuse(C.byref(m), *map(float, col))
        return m

    @staticmethod
    def light(col, strength: float) -> "Material":  # makeLight, mesh.h:72-77
        m = Material.default()
        lib().rt2_material_make_light(C.byref(m), *map(float, col), float(strength))
        return m

    @staticmethod
    def specular(col, spec_col, smooth: float, prob: float) -> "Material":  # makeSpecular, mesh.h:63-70
        m = Material.default()
        lib().rt2_material_make_specular(C.byref(m), *map(float, col), *map(float, spec_col), float(smooth),
                                         float(prob))
        return m

    @staticmethod
    def texture(index: int, col=(1.0, 1.0, 1.0)) -> "Material":  # map_Kd in an MTL, mesh.h:430-450
        m = Material.diffuse(col)
        m.materialType = 5
        m.textureIndex = int(index)
        return m

    @staticmethod
    def checker(scale: float) -> "Material":  # makeChecker, mesh.h:79-83
        m = Material.default()
        lib().rt2_material_make_checker(C.byref(m), float(scale))
        return m

    @staticmethod
    def glass(col, ior: float) -> "Material":  # makeGlass, mesh.h:85-90
        m = Material.default()
        lib().rt2_material_make_glass(C.byref(m), *map(float, col), float(ior))
        return m


class Node(C.Structure):  # Node, BVH.h:54-65
    _fields_ = [("bmin", C.c_float * 3), ("pad0", C.c_float), ("bmax", C.c_float * 3), ("pad1", C.c_float),
                ("triangleIndex", C.c_int32), ("triangleCount", C.c_int32), ("childIndex", C.c_int32),
                ("pad", C.c_int32)]


class Uniforms(C.Structure):  # GlobalUniforms, camera.h:10-36
    _fields_ = [("pad", C.c_int32), ("numTextures", C.c_int32), ("width", C.c_uint32), ("height", C.c_uint32),
                ("numSpheres", C.c_int32), ("numTriangles", C.c_int32), ("basicShading", C.c_int32),
                ("basicShadingShadow", C.c_int32), ("basicShadingLightPosition", Vec4),
                ("environmentalLight", C.c_int32), ("maxBounceCount", C.c_int32), ("numRaysPerPixel", C.c_int32),
                ("frameIndex", C.c_uint32), ("cameraPos", Vec4), ("viewportRight", Vec4), ("viewportUp", Vec4),
                ("viewportFront", Vec4), ("pixelRight", Vec4), ("pixelUp", Vec4), ("defocusDiskRight", Vec4),
                ("defocusDiskUp", Vec4)]


class Shard(C.Structure):
    _fields_ = [("tile_rows", C.c_int32), ("rank", C.c_int32), ("nranks", C.c_int32)]


ABI_VERSION = 4  # include/rt2.h RT2_ABI_VERSION
COMM_ID_BYTES = 128  # RT2_COMM_ID_BYTES


class Image(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("channels", C.c_int32),
                ("pixels", C.POINTER(C.c_uint8))]


class Stats(C.Structure):
    _fields_ = [("samples", C.c_uint64), ("segments", C.c_uint64), ("tests", C.c_uint64),
                ("node_visits", C.c_uint64)]


class ShadeOpts(C.Structure):  # rt2_shade_opts
    _fields_ = [("light", C.c_float * 3), ("shadow", C.c_int32), ("max_bounce", C.c_int32), ("pad", C.c_int32 * 3)]


class PathOpts(C.Structure):  # rt2_path_opts
    _fields_ = [("max_bounce", C.c_int32), ("environmental_light", C.c_int32), ("pad", C.c_int32 * 2)]


class CameraDesc(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("position", C.c_float * 3), ("hfov", C.c_float),
                ("pitch", C.c_float), ("yaw", C.c_float), ("focus_distance", C.c_float),
                ("defocus_angle", C.c_float), ("zoom", C.c_float)]


assert C.sizeof(Triangle) == 80 and C.sizeof(Material) == 96
assert C.sizeof(Node) == 48 and C.sizeof(Uniforms) == 192 and C.sizeof(ShadeOpts) == 32

TRI_DTYPE = np.dtype([("a", "<f4", 4), ("b", "<f4", 4), ("c", "<f4", 4), ("aTex", "<f4", 2), ("bTex", "<f4", 2),
                      ("cTex", "<f4", 2), ("materialIndex", "<i4"), ("pad", "<f4")])
MAT_DTYPE = np.dtype([("color", "<f4", 4), ("specularColor", "<f4", 4), ("emissionColor", "<f4", 4),
                      ("textureIndex", "<i4"), ("emissionStrength", "<f4"), ("smoothness", "<f4"),
                      ("specularProbability", "<f4"), ("checkerScale", "<f4"), ("refractiveIndex", "<f4"),
                      ("materialType", "<i4"), ("index", "<i4"), ("isEdgeHighlight", "<i4"), ("pad1", "<i4"),
                      ("pad2", "<i4"), ("pad3", "<i4")])
NODE_DTYPE = np.dtype([("bmin", "<f4", 3), ("pad0", "<f4"), ("bmax", "<f4", 3), ("pad1", "<f4"),
                       ("triangleIndex", "<i4"), ("triangleCount", "<i4"), ("childIndex", "<i4"), ("pad", "<i4")])
assert TRI_DTYPE.itemsize == 80 and MAT_DTYPE.itemsize == 96 and NODE_DTYPE.itemsize == 48
# rt2_ray / rt2_hit (ray queries); tmax: 0 (or anything outside (0, 1e38)) = unbounded
RAY_DTYPE = np.dtype([("o", "<f4", 3), ("tmax", "<f4"), ("d", "<f4", 3), ("pad", "<f4")])
HIT_DTYPE = np.dtype([("dst", "<f4"), ("tri", "<i4")])
assert RAY_DTYPE.itemsize == 32 and HIT_DTYPE.itemsize == 8
# rt2_surface (surface queries): the hit record of rt2_trace_rays, the material, the unit normal, the
# barycentrics of b and c, and the base colour; a miss has tri = mtl = mtl_type = -1 and zeros
SURFACE_DTYPE = np.dtype([("dst", "<f4"), ("tri", "<i4"), ("mtl", "<i4"), ("mtl_type", "<i4"), ("normal", "<f4", 3),
                          ("u", "<f4"), ("albedo", "<f4", 3), ("v", "<f4")])
assert SURFACE_DTYPE.itemsize == 48
TRACE_AUTO, TRACE_SCALAR = 0, 1  # RT2_TRACE_AUTO, RT2_TRACE_SCALAR
# rt2_cluster / rt2_cluster_table (include/rt2_cluster.h): the resident kernel's clusters of triangle groups
MAX_CLUSTERS, CLUSTER_COMPACT = 13, 0x10000
CLUSTER_DTYPE = np.dtype([("lo", "<f4", 3), ("g0", "<i4"), ("hi", "<f4", 3), ("g1_flags", "<i4")])
CLUSTER_TABLE_DTYPE = np.dtype([("far_o", "<f4"), ("n", "<i4"), ("pad_abs", "<f4"), ("reserved", "<i4", 5),
                                ("c", CLUSTER_DTYPE, MAX_CLUSTERS)])
assert CLUSTER_DTYPE.itemsize == 32 and CLUSTER_TABLE_DTYPE.itemsize == 32 + 32 * MAX_CLUSTERS
QUERY_RES, QUERY_RES_L2, QUERY_SCALAR, QUERY_BVH = -2, -3, -4, -5  # Scene.last_kernel after a query
OCCLUDED_RES, OCCLUDED_RES_L2, OCCLUDED_SCALAR, OCCLUDED_BVH = -6, -7, -8, -9  # ... after an occlusion query
SURFACE_RES, SURFACE_RES_L2, SURFACE_SCALAR, SURFACE_BVH = -10, -11, -12, -13  # ... after a surface query
SHADE_RES, SHADE_RES_L2, SHADE_SCALAR, SHADE_BVH = -14, -15, -16, -17  # ... after a preview shading query
# rt2_shaded (preview shading queries): traceBasic's colour and the closest-hit searches the ray cost
SHADED_DTYPE = np.dtype([("rgb", "<f4", 3), ("segments", "<i4")])
assert SHADED_DTYPE.itemsize == 16
RADIANCE_RES, RADIANCE_RES_L2, RADIANCE_SCALAR, RADIANCE_BVH = -18, -19, -20, -21  # ... after a radiance query
LINEAR_TWIN = 1000  # ... after a linear render: the variant's id + LINEAR_TWIN (1136 for the automatic 0)
# rt2_radiance (radiance queries): trace()'s linear colour and the closest-hit searches the path cost
RADIANCE_DTYPE = np.dtype([("rgb", "<f4", 3), ("segments", "<i4")])
assert RADIANCE_DTYPE.itemsize == 16 and C.sizeof(PathOpts) == 16

# Every symbol include/rt2.h declares (tests check the library exports them all).
EXPORTED = [
    "rt2_last_error", "rt2_abi_version", "rt2_scene_create", "rt2_scene_destroy", "rt2_shard_rows",
    "rt2_shard_row", "rt2_render", "rt2_render_host", "rt2_resolve_rgba32f", "rt2_resolve_rgb8_reference",
    "rt2_scene_stats", "rt2_scene_set_variant", "rt2_scene_set_traversal", "rt2_scene_set_frame_split", "rt2_scene_set_cost_order", "rt2_sd_create", "rt2_sd_destroy", "rt2_sd_load_obj_folder",
    "rt2_sd_add_material", "rt2_sd_add_triangle", "rt2_sd_add_triangles", "rt2_sd_add_cornell_box", "rt2_sd_add_mirror_cornell_box",
    "rt2_sd_add_side_lit_cornell_box", "rt2_sd_add_sky_light_plane", "rt2_sd_add_cube",
    "rt2_sd_create_classic_cornell_box", "rt2_sd_create_diverse_cornell_box", "rt2_sd_build_bvh",
    "rt2_sd_num_triangles", "rt2_sd_num_materials", "rt2_sd_num_nodes", "rt2_sd_num_textures",
    "rt2_sd_triangles", "rt2_sd_materials", "rt2_sd_nodes", "rt2_sd_bvh_triangles", "rt2_sd_texture_name",
    "rt2_material_default", "rt2_material_make_diffuse", "rt2_material_make_light", "rt2_material_make_specular",
    "rt2_material_make_checker", "rt2_material_make_glass", "rt2_camera_default", "rt2_camera_uniforms",
    "rt2_uniforms_offline", "rt2_write_png", "rt2_image_load", "rt2_image_free", "rt2_sd_texture",
    "rt2_scene_set_textures", "rt2_comm_unique_id", "rt2_comm_init", "rt2_comm_wrap", "rt2_comm_destroy",
    "rt2_comm_size", "rt2_comm_check", "rt2_gather_slabs", "rt2_unshard_slabs", "rt2_render_host_gather",
    "rt2_comm_wait", "rt2_trace_rays", "rt2_trace_rays_host", "rt2_occluded", "rt2_occluded_host",
    "rt2_surface_rays", "rt2_surface_rays_host", "rt2_camera_rays", "rt2_camera_rays_host",
    "rt2_shade_rays", "rt2_shade_rays_host",
    "rt2_radiance_rays", "rt2_radiance_rays_host", "rt2_path_rays", "rt2_path_rays_host",
    "rt2_render_linear", "rt2_render_linear_host", "rt2_resolve_tonemap",
]

_lib: Optional[C.CDLL] = None


class RT2Error(RuntimeError):
    pass


def lib() -> C.CDLL:
    """Load librt2.so (raises if it was not built: no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RT2Error(f"{LIB_PATH} is missing: build it with `make -C raytracing2-fork_amd` "
                       "(or __graft_entry__.build()); the render path has no CPU fallback")
    # One HIP runtime per process.  torch ships its own libamdhip64 (SONAME
    # libamdhip64.so.7, but its libs NEED the file name "libamdhip64.so"): if
    # librt2 loaded /opt/rocm's runtime first, importing torch afterwards would
    # bring a second runtime and the two would fight over the device.  Loading
    # torch first makes librt2's NEEDED libamdhip64.so.7 bind to torch's copy,
    # so torch tensors and rt2 kernels share one runtime (and one context).
    if os.environ.get("RT2_NO_TORCH", "0") != "1":
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    L = C.CDLL(LIB_PATH)
    P, I32, U32, I64, F = C.c_void_p, C.c_int32, C.c_uint32, C.c_int64, C.c_float
    sig = {
        "rt2_last_error": (C.c_char_p, []),
        "rt2_abi_version": (C.c_int, []),
        "rt2_scene_create": (C.c_int, [P, I32, P, I32, P, I32, I32, C.POINTER(P)]),
        "rt2_scene_destroy": (None, [P]),
        "rt2_shard_rows": (I32, [I32, Shard]),
        "rt2_shard_row": (I32, [I32, Shard]),
        "rt2_render": (C.c_int, [P, C.POINTER(Uniforms), U32, U32, Shard, P, P, P]),
        "rt2_render_host": (C.c_int, [P, C.POINTER(Uniforms), U32, U32, Shard, P, P]),
        "rt2_trace_rays": (C.c_int, [P, P, I64, P, C.c_int, P]),
        "rt2_trace_rays_host": (C.c_int, [P, P, I64, P, C.c_int]),
        "rt2_occluded": (C.c_int, [P, P, I64, P, C.c_int, P]),
        "rt2_occluded_host": (C.c_int, [P, P, I64, P, C.c_int]),
        "rt2_surface_rays": (C.c_int, [P, P, I64, P, C.c_int, P]),
        "rt2_surface_rays_host": (C.c_int, [P, P, I64, P, C.c_int]),
        "rt2_shade_rays": (C.c_int, [P, P, I64, C.POINTER(ShadeOpts), P, C.c_int, P]),
        "rt2_shade_rays_host": (C.c_int, [P, P, I64, C.POINTER(ShadeOpts), P, C.c_int]),
        "rt2_radiance_rays": (C.c_int, [P, P, I64, C.POINTER(PathOpts), P, P, C.c_int, P]),
        "rt2_radiance_rays_host": (C.c_int, [P, P, I64, C.POINTER(PathOpts), P, P, C.c_int]),
        "rt2_path_rays": (C.c_int, [P, C.POINTER(Uniforms), Shard, U32, C.c_int, P, P, P]),
        "rt2_path_rays_host": (C.c_int, [P, C.POINTER(Uniforms), Shard, U32, C.c_int, P, P]),
        "rt2_camera_rays": (C.c_int, [P, C.POINTER(Uniforms), Shard, P, P]),
        "rt2_camera_rays_host": (C.c_int, [P, C.POINTER(Uniforms), Shard, P]),
        "rt2_render_linear": (C.c_int, [P, C.POINTER(Uniforms), U32, U32, Shard, P, P, P]),
        "rt2_render_linear_host": (C.c_int, [P, C.POINTER(Uniforms), U32, U32, Shard, P, P]),
        "rt2_resolve_tonemap": (C.c_int, [P, I64, U32, P, P]),
        "rt2_resolve_rgba32f": (C.c_int, [P, I64, U32, P, P]),
        "rt2_resolve_rgb8_reference": (C.c_int, [P, I64, U32, P]),
        "rt2_scene_stats": (C.c_int, [P, C.POINTER(Stats), C.c_int]),
        "rt2_scene_set_variant": (C.c_int, [P, C.c_int]),
        "rt2_scene_set_traversal": (C.c_int, [P, C.c_int]),
        "rt2_scene_set_frame_split": (C.c_int, [P, C.c_int]),
        "rt2_scene_set_cost_order": (C.c_int, [P, C.c_int]),
        "rt2_scene_set_textures": (C.c_int, [P, C.POINTER(Image), I32]),
        "rt2_image_load": (C.c_int, [C.c_char_p, I32, C.POINTER(Image)]),
        "rt2_image_free": (None, [C.POINTER(Image)]),
        "rt2_sd_texture": (C.c_int, [P, I32, C.POINTER(Image)]),
        "rt2_sd_create": (P, []),
        "rt2_sd_destroy": (None, [P]),
        "rt2_sd_load_obj_folder": (C.c_int, [P, C.c_char_p]),
        "rt2_sd_add_material": (I32, [P, C.POINTER(Material)]),
        "rt2_sd_add_triangle": (C.c_int, [P, P, P, P, I32]),
        "rt2_sd_add_triangles": (C.c_int, [P, P, I32]),
        "rt2_sd_add_cornell_box": (C.c_int, [P, F, F, I32, I32]),
        "rt2_sd_add_mirror_cornell_box": (C.c_int, [P, F, F, I32, I32]),
        "rt2_sd_add_side_lit_cornell_box": (C.c_int, [P, F, F, I32, I32, I32]),
        "rt2_sd_add_sky_light_plane": (C.c_int, [P, I32]),
        "rt2_sd_add_cube": (C.c_int, [P, P, P, P, I32]),
        "rt2_sd_create_classic_cornell_box": (C.c_int, [P, F, I32, I32, I32, I32]),
        "rt2_sd_create_diverse_cornell_box": (C.c_int, [P, F, I32, I32, I32, I32, I32, I32, I32, I32]),
        "rt2_sd_build_bvh": (C.c_int, [P]),
        "rt2_sd_num_triangles": (I32, [P]),
        "rt2_sd_num_materials": (I32, [P]),
        "rt2_sd_num_nodes": (I32, [P]),
        "rt2_sd_num_textures": (I32, [P]),
        "rt2_sd_triangles": (P, [P]),
        "rt2_sd_materials": (P, [P]),
        "rt2_sd_nodes": (P, [P]),
        "rt2_sd_bvh_triangles": (C.c_int, [P, P]),
        "rt2_sd_texture_name": (C.c_char_p, [P, I32]),
        "rt2_material_default": (None, [C.POINTER(Material)]),
        "rt2_material_make_diffuse": (None, [C.POINTER(Material), F, F, F]),
        "rt2_material_make_light": (None, [C.POINTER(Material), F, F, F, F]),
        "rt2_material_make_specular": (None, [C.POINTER(Material), F, F, F, F, F, F, F, F]),
        "rt2_material_make_checker": (None, [C.POINTER(Material), F]),
        "rt2_material_make_glass": (None, [C.POINTER(Material), F, F, F, F]),
        "rt2_camera_default": (None, [C.POINTER(CameraDesc), I32, I32]),
        "rt2_camera_uniforms": (C.c_int, [C.POINTER(CameraDesc), C.POINTER(Uniforms)]),
        "rt2_uniforms_offline": (None, [C.POINTER(Uniforms), I32, I32, I32, I32, I32, I32]),
        "rt2_write_png": (C.c_int, [C.c_char_p, I32, I32, I32, P, I32]),
        "rt2_comm_unique_id": (C.c_int, [P]),
        "rt2_comm_init": (C.c_int, [P, I32, I32, I32, C.POINTER(P)]),
        "rt2_comm_wrap": (C.c_int, [P, I32, C.POINTER(P)]),
        "rt2_comm_destroy": (None, [P]),
        "rt2_comm_size": (C.c_int, [P, C.POINTER(I32), C.POINTER(I32)]),
        "rt2_comm_check": (C.c_int, [P]),
        "rt2_comm_wait": (C.c_int, [P, P]),
        "rt2_gather_slabs": (C.c_int, [P, P, I32, I32, Shard, I32, P, P]),
        "rt2_unshard_slabs": (C.c_int, [P, I32, I32, I32, Shard, P, P]),
        "rt2_render_host_gather": (C.c_int, [P, C.POINTER(Uniforms), U32, U32, Shard, P, I32, P, P]),
        "rt2_device_selftest": (C.c_int, [P, I32, P]),
        "rt2_device_numerics": (C.c_int, [I32, P, I32, P]),
        "rt2_device_rcp_check": (C.c_int, [U32, U32, C.c_int, C.POINTER(C.c_ulonglong), C.POINTER(U32)]),
        "rt2_device_div_check": (C.c_int, [U32, C.c_ulonglong, C.c_int, C.POINTER(C.c_ulonglong), C.POINTER(U32)]),
        "rt2_variant_name": (C.c_char_p, [C.c_int]),
        "rt2_scene_diag": (C.c_int, [P, C.POINTER(C.c_ulonglong), C.POINTER(C.c_int)]),
        "rt2_scene_plk_info": (C.c_int, [P, C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_int)]),
        "rt2_scene_export": (C.c_longlong, [P, C.c_int, P, C.c_ulonglong]),
        "rt2_mfma_probe": (C.c_int, [P, C.c_int, P, I32, P, P, P, P]),
        "rt2_cluster_table_build": (C.c_int, [P, I32, P]),
        "rt2_cluster_need": (C.c_int, [P, P, I64, P]),
        "rt2_scene_set_clusters": (C.c_int, [P, P]),
        "rt2_cluster_order_build": (C.c_int, [P, I32, P, P]),
        "rt2_scene_set_slot_order": (C.c_int, [P, P, P]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    if L.rt2_abi_version() != ABI_VERSION:
        raise RT2Error(f"librt2.so ABI {L.rt2_abi_version()} != {ABI_VERSION}: rebuild (make -C raytracing2-fork_amd)")
    _lib = L
    return L


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise RT2Error(f"{what}: {lib().rt2_last_error().decode()}")


def _f3(v) -> C.Array:
    return (C.c_float * 3)(*map(float, v))


def _ptr(x: int):
    """A nullable address (a device array, a stream) as a ctypes argument."""
    return C.c_void_p(x) if x else None


def _pack_rays(who: str, origins, directions, tmax=None) -> np.ndarray:
    """The RAY_DTYPE array of a blocking ray query: origins and directions
    (n, 3), tmax None (0: unbounded), a scalar or (n,)."""
    o = np.asarray(origins, dtype=np.float32).reshape(-1, 3)
    d = np.asarray(directions, dtype=np.float32).reshape(-1, 3)
    if len(o) != len(d):
        raise RT2Error(f"{who}: {len(o)} origins for {len(d)} directions")
    rays = np.zeros(len(o), dtype=RAY_DTYPE)
    rays["o"], rays["d"] = o, d
    if tmax is not None:
        rays["tmax"] = np.asarray(tmax, dtype=np.float32)
    return rays


class SceneData:
    """The reference's host scene arrays (rayTracing.cpp:1256-1293)."""

    def __init__(self):
        self._p = lib().rt2_sd_create()
        if not self._p:
            raise RT2Error("rt2_sd_create failed")

    def __del__(self):
        if getattr(self, "_p", None) and _lib is not None:
            try:
                _lib.rt2_sd_destroy(self._p)
            except Exception:  # interpreter shutdown
                pass
            self._p = None

    def load_obj_folder(self, folder: str) -> None:  # getTrianglesData_, mesh.h:279-613
        _check(lib().rt2_sd_load_obj_folder(self._p, folder.encode()), f"load {folder}")

    def add_material(self, m: Material) -> int:
        i = lib().rt2_sd_add_material(self._p, C.byref(m))
        if i < 0:
            _check(-1, "add_material")
        return i

    def add_triangle(self, a, b, c, material_index: int) -> None:
        _check(lib().rt2_sd_add_triangle(self._p, _f3(a), _f3(b), _f3(c), int(material_index)), "add_triangle")

    def add_triangles(self, tris: np.ndarray) -> None:
        tris = np.ascontiguousarray(tris, dtype=TRI_DTYPE)
        _check(lib().rt2_sd_add_triangles(self._p, tris.ctypes.data, len(tris)), "add_triangles")

    def add_cornell_box(self, light_size, pad, light_mtl, light_enabled=True):  # rayTracing.cpp:453
        _check(lib().rt2_sd_add_cornell_box(self._p, light_size, pad, light_mtl, int(bool(light_enabled))),
               "addCornellBox")

    def add_mirror_cornell_box(self, light_size, pad, light_mtl, mirror_mtl):  # :569
        _check(lib().rt2_sd_add_mirror_cornell_box(self._p, light_size, pad, light_mtl, mirror_mtl),
               "addMirrorCornellBox")

    def add_side_lit_cornell_box(self, light_size, pad, light_mtl, wall_mtl, rotate=False):  # :690
        _check(lib().rt2_sd_add_side_lit_cornell_box(self._p, light_size, pad, light_mtl, wall_mtl, int(rotate)),
               "addSideLitCornellBox")

    def add_sky_light_plane(self, light_mtl):  # :388
        _check(lib().rt2_sd_add_sky_light_plane(self._p, light_mtl), "addSkyLightPlane")

    def add_cube(self, center, size, rotation, mtl):  # :867
        _check(lib().rt2_sd_add_cube(self._p, _f3(center), _f3(size), _f3(rotation), mtl), "addCube")

    def create_classic_cornell_box(self, room, red, green, white, light):  # :949
        _check(lib().rt2_sd_create_classic_cornell_box(self._p, room, red, green, white, light),
               "createClassicCornellBox")

    def create_diverse_cornell_box(self, room, red, green, white, light, glass, mirror, checker, metal):  # :1071
        _check(lib().rt2_sd_create_diverse_cornell_box(self._p, room, red, green, white, light, glass, mirror,
                                                       checker, metal), "createDiverseCornellBox")

    def build_bvh(self) -> None:  # BVH.h:150-163
        _check(lib().rt2_sd_build_bvh(self._p), "BVH")

    @property
    def num_triangles(self) -> int:
        return lib().rt2_sd_num_triangles(self._p)

    @property
    def num_materials(self) -> int:
        return lib().rt2_sd_num_materials(self._p)

    @property
    def num_nodes(self) -> int:
        return lib().rt2_sd_num_nodes(self._p)

    @property
    def texture_names(self) -> list:
        return [lib().rt2_sd_texture_name(self._p, i).decode() for i in range(lib().rt2_sd_num_textures(self._p))]

    def texture(self, i: int) -> np.ndarray:
        """Decoded texture i as (height, width, channels) uint8, row 0 first (flipped on load)."""
        im = Image()
        _check(lib().rt2_sd_texture(self._p, i, C.byref(im)), "rt2_sd_texture")
        return _image_array(im)

    def textures(self) -> list:
        return [self.texture(i) for i in range(lib().rt2_sd_num_textures(self._p))]

    def _view(self, ptr, n, dtype) -> np.ndarray:
        if n == 0:
            return np.zeros(0, dtype=dtype)
        buf = (C.c_char * (n * dtype.itemsize)).from_address(ptr)
        return np.frombuffer(buf, dtype=dtype).copy()

    def triangles(self) -> np.ndarray:
        return self._view(lib().rt2_sd_triangles(self._p), self.num_triangles, TRI_DTYPE)

    def materials(self) -> np.ndarray:
        return self._view(lib().rt2_sd_materials(self._p), self.num_materials, MAT_DTYPE)

    def nodes(self) -> np.ndarray:
        return self._view(lib().rt2_sd_nodes(self._p), self.num_nodes, NODE_DTYPE)

    def bvh_triangles(self) -> np.ndarray:
        out = np.zeros((self.num_triangles, 9), dtype=np.float32)
        _check(lib().rt2_sd_bvh_triangles(self._p, out.ctypes.data), "bvh_triangles")
        return out


def default_camera(width: int, height: int) -> CameraDesc:
    cam = CameraDesc()
    lib().rt2_camera_default(C.byref(cam), width, height)
    return cam


def camera_uniforms(cam: CameraDesc, u: Optional[Uniforms] = None) -> Uniforms:
    u = u or Uniforms()
    _check(lib().rt2_camera_uniforms(C.byref(cam), C.byref(u)), "camera")
    return u


def _image_array(im: Image) -> np.ndarray:
    n = im.width * im.height * im.channels
    buf = (C.c_uint8 * n).from_address(C.addressof(im.pixels.contents))
    return np.frombuffer(buf, dtype=np.uint8).copy().reshape(im.height, im.width, im.channels)


def load_image(path: str, flip_vertically: bool = True) -> np.ndarray:
    """rt2_image_load: stbi_load(path, ..., 0) as Texture2D uses it -> (h, w, channels) uint8."""
    im = Image()
    _check(lib().rt2_image_load(path.encode(), int(bool(flip_vertically)), C.byref(im)), "rt2_image_load")
    try:
        return _image_array(im)
    finally:
        lib().rt2_image_free(C.byref(im))


def offline_uniforms(width, height, max_bounce, rays_per_pixel, num_triangles, num_textures=0) -> Uniforms:
    """screenshot() settings (rayTracing.cpp:146-153) + main()'s per-frame fields."""
    u = Uniforms()
    lib().rt2_uniforms_offline(C.byref(u), width, height, max_bounce, rays_per_pixel, num_triangles, num_textures)
    return u


def shade_opts(light=(0.0, 0.0, 0.0), shadow: bool = False, max_bounce: int = 1) -> ShadeOpts:
    """rt2_shade_opts: the preview's light position, shadow switch and bounce limit."""
    o = ShadeOpts()
    o.light[:] = [float(x) for x in light]
    o.shadow, o.max_bounce = int(bool(shadow)), int(max_bounce)
    return o


def path_opts(max_bounce: int = 8, environmental_light: bool = True) -> PathOpts:
    """rt2_path_opts: the path tracer's bounce limit and sky switch."""
    o = PathOpts()
    o.max_bounce, o.environmental_light = int(max_bounce), int(bool(environmental_light))
    return o


def shard(tile_rows=1, rank=0, nranks=1) -> Shard:
    return Shard(tile_rows, rank, nranks)


def shard_rows(height: int, sh: Shard) -> int:
    return lib().rt2_shard_rows(height, sh)


def shard_row_ids(height: int, sh: Shard) -> np.ndarray:
    n = shard_rows(height, sh)
    return np.array([lib().rt2_shard_row(i, sh) for i in range(n)], dtype=np.int32)


class Comm:
    """RCCL communicator of the multi-GPU C-ABI (rt2_comm_*): one per rank/GPU."""

    @staticmethod
    def unique_id() -> bytes:
        buf = (C.c_uint8 * COMM_ID_BYTES)()
        _check(lib().rt2_comm_unique_id(buf), "rt2_comm_unique_id")
        return bytes(buf)

    def __init__(self, uid: bytes, nranks: int, rank: int, device: int = 0):
        if len(uid) != COMM_ID_BYTES:
            raise RT2Error(f"communicator id must be {COMM_ID_BYTES} bytes")
        buf = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(uid)
        p = C.c_void_p()
        _check(lib().rt2_comm_init(buf, nranks, rank, device, C.byref(p)), "rt2_comm_init")
        self._p = p
        self.nranks, self.rank, self.device = nranks, rank, device

    def close(self):
        if getattr(self, "_p", None) and _lib is not None:
            _lib.rt2_comm_destroy(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass

    def check(self) -> None:
        _check(lib().rt2_comm_check(self._p), "rt2_comm_check")

    def gather_slabs(self, slab_ptr: int, width: int, height: int, sh: Shard, root: int, image_ptr: int,
                     stream: int = 0) -> None:
        _check(lib().rt2_gather_slabs(self._p, C.c_void_p(slab_ptr), width, height, sh, root,
                                      _ptr(image_ptr), _ptr(stream)), "rt2_gather_slabs")

    def wait(self, stream: int = 0) -> None:
        """rt2_comm_wait: the stream drained under the RT2_COMM_TIMEOUT_S deadline."""
        _check(lib().rt2_comm_wait(self._p, _ptr(stream)), "rt2_comm_wait")


def unshard_slabs(gathered_ptr: int, max_rows: int, width: int, height: int, layout: Shard, image_ptr: int,
                  stream: int = 0) -> None:
    """Root-side un-interleave of [nranks][max_rows][width] 16-byte pixels (rt2_unshard_slabs)."""
    _check(lib().rt2_unshard_slabs(C.c_void_p(gathered_ptr), max_rows, width, height, layout, C.c_void_p(image_ptr),
                                   _ptr(stream)), "rt2_unshard_slabs")


class Scene:
    """Device-resident scene: the SSBO uploads of rayTracing.cpp:1323-1325."""

    def __init__(self, sd: Optional[SceneData] = None, device: int = 0, triangles=None, materials=None,
                 nodes=None):
        if sd is not None:
            triangles, materials, nodes = sd.triangles(), sd.materials(), sd.nodes()
        triangles = np.ascontiguousarray(triangles, dtype=TRI_DTYPE)
        materials = np.ascontiguousarray(materials, dtype=MAT_DTYPE)
        nodes = None if nodes is None or len(nodes) == 0 else np.ascontiguousarray(nodes, dtype=NODE_DTYPE)
        self.n_tris = len(triangles)
        self.device = device
        p = C.c_void_p()
        _check(lib().rt2_scene_create(triangles.ctypes.data, len(triangles), materials.ctypes.data, len(materials),
                                      None if nodes is None else nodes.ctypes.data,
                                      0 if nodes is None else len(nodes), device, C.byref(p)), "rt2_scene_create")
        self._p = p

    def close(self):
        if getattr(self, "_p", None) and _lib is not None:
            _lib.rt2_scene_destroy(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass

    def set_variant(self, v: int) -> int:
        """Forces kernel variant v (0 = automatic); raises if v is not in this build."""
        r = lib().rt2_scene_set_variant(self._p, v)
        if r < 0:
            _check(r, "set_variant")
        return r

    def set_traversal(self, traversal: str) -> None:
        """"brute" (north-star kernel) or "bvh" (compute.glsl:410-460 on the uploaded nodes)."""
        _check(lib().rt2_scene_set_traversal(self._p, {"brute": 0, "bvh": 1}[traversal]), "set_traversal")

    def set_frame_split(self, enable: bool) -> None:
        """(frame, pixel) work items for multi-frame renders (rt2_scene_set_frame_split)."""
        _check(lib().rt2_scene_set_frame_split(self._p, int(bool(enable))), "set_frame_split")

    def set_cost_order(self, enable: bool) -> None:
        """Most-expensive-first pixel order from the previous render (rt2_scene_set_cost_order)."""
        _check(lib().rt2_scene_set_cost_order(self._p, int(bool(enable))), "set_cost_order")

    def set_textures(self, images) -> None:
        """Uploads textures (list of (h, w, channels) uint8 arrays, stb layout) — the
        reference's texture units 0..4 (rt2_scene_set_textures)."""
        arrs = [np.ascontiguousarray(a, dtype=np.uint8) for a in images]
        arrs = [a if a.ndim == 3 else a[..., None] for a in arrs]
        ims = (Image * max(len(arrs), 1))()
        for i, a in enumerate(arrs):
            ims[i].width, ims[i].height, ims[i].channels = a.shape[1], a.shape[0], a.shape[2]
            ims[i].pixels = a.ctypes.data_as(C.POINTER(C.c_uint8))
        _check(lib().rt2_scene_set_textures(self._p, ims, len(arrs)), "rt2_scene_set_textures")

    def render(self, u: Uniforms, frame_begin: int, frame_count: int, sh: Shard, accum_ptr: int,
               accum8_ptr: int = 0, stream: int = 0) -> None:
        """Asynchronous device render into caller-owned device accumulators (rt2_render)."""
        _check(lib().rt2_render(self._p, C.byref(u), frame_begin, frame_count, sh, C.c_void_p(accum_ptr),
                                _ptr(accum8_ptr), _ptr(stream)), "rt2_render")

    def render_host(self, u: Uniforms, frame_begin: int, frame_count: int, sh: Optional[Shard] = None,
                    rgb8: bool = False):
        """Blocking render; returns the mean rgba32f slab (rows, W, 4) [and the 8-bit reference average]."""
        sh = sh or shard()
        rows = shard_rows(u.height, sh)
        out = np.zeros((rows, u.width, 4), dtype=np.float32)
        out8 = np.zeros((rows, u.width, 3), dtype=np.uint8) if rgb8 else None
        _check(lib().rt2_render_host(self._p, C.byref(u), frame_begin, frame_count, sh, out.ctypes.data,
                                     None if out8 is None else out8.ctypes.data), "rt2_render_host")
        return (out, out8) if rgb8 else out

    def render_linear(self, u: Uniforms, frame_begin: int, frame_count: int, sh: Shard, sum_ptr: int,
                      sumsq_ptr: int = 0, stream: int = 0) -> None:
        """Asynchronous linear render (rt2_render_linear): render()'s paths on the chosen kernel's linear twin
        (last_kernel() = the variant's id + LINEAR_TWIN), the frames' linear means added to the device array at
        sum_ptr and, with sumsq_ptr, the means of the samples' squares to that one ((rows, W, 4) float32 each,
        aligned to 16 bytes, .w written 0)."""
        _check(lib().rt2_render_linear(self._p, C.byref(u), frame_begin, frame_count, sh, C.c_void_p(sum_ptr),
                                       _ptr(sumsq_ptr), _ptr(stream)), "rt2_render_linear")

    def render_linear_host(self, u: Uniforms, frame_begin: int, frame_count: int, sh: Optional[Shard] = None,
                           moments: bool = False):
        """Blocking linear render (rt2_render_linear_host): the (rows, W, 4) float32 mean over the frames of the
        per-frame linear means (alpha = 1) — render_host's image before the tonemap and the sRGB encoding — or,
        with moments, the pair (mean, meansq) with the mean of the samples' squares beside it."""
        sh = sh or shard()
        rows = max(shard_rows(u.height, sh), 0)  # a bad shard: the library says so
        mean = np.zeros((rows, u.width, 4), dtype=np.float32)
        meansq = np.zeros((rows, u.width, 4), dtype=np.float32) if moments else None
        _check(lib().rt2_render_linear_host(self._p, C.byref(u), frame_begin, frame_count, sh, mean.ctypes.data,
                                            None if meansq is None else meansq.ctypes.data),
               "rt2_render_linear_host")
        return (mean, meansq) if moments else mean

    def render_host_gather(self, u: Uniforms, frame_begin: int, frame_count: int, sh: Shard, comm: "Comm",
                           root: int = 0, rgb8: bool = False):
        """rt2_render_host_gather: this rank's shard, gathered to `root`; returns the
        whole (H, W, 4) mean image [and the 8-bit average] on the root, None elsewhere."""
        is_root = comm.rank == root
        out = np.zeros((u.height, u.width, 4), dtype=np.float32) if is_root else None
        out8 = np.zeros((u.height, u.width, 3), dtype=np.uint8) if (is_root and rgb8) else None
        _check(lib().rt2_render_host_gather(self._p, C.byref(u), frame_begin, frame_count, sh, comm._p, root,
                                            None if out is None else out.ctypes.data,
                                            None if out8 is None else out8.ctypes.data), "rt2_render_host_gather")
        if not is_root:
            return None
        return (out, out8) if rgb8 else out

    def trace_rays(self, origins, directions, tmax=None, flags: int = 0):
        """Closest hit of n rays (rt2_trace_rays_host, blocking): origins and
        directions (n, 3), tmax None (unbounded), a scalar or (n,).  Returns
        (dst float32[n], tri int32[n]); a miss has tri = -1 and dst = the ray's
        bound.  Indices are those of the triangle array the scene was made of."""
        rays = _pack_rays("trace_rays", origins, directions, tmax)
        hits = np.zeros(len(rays), dtype=HIT_DTYPE)
        _check(lib().rt2_trace_rays_host(self._p, rays.ctypes.data, len(rays), hits.ctypes.data, int(flags)),
               "rt2_trace_rays_host")
        return hits["dst"].copy(), hits["tri"].copy()

    def trace_rays_device(self, rays_ptr: int, n: int, hits_ptr: int, flags: int = 0, stream: int = 0) -> None:
        """Asynchronous query over device arrays of n rt2_ray / rt2_hit records (rt2_trace_rays)."""
        _check(lib().rt2_trace_rays(self._p, _ptr(rays_ptr), int(n), _ptr(hits_ptr), int(flags), _ptr(stream)),
               "rt2_trace_rays")

    def occluded(self, origins, directions, tmax=None, flags: int = 0) -> np.ndarray:
        """Whether anything lies in front of each of n rays before its bound
        (rt2_occluded_host, blocking): the arguments of trace_rays; returns
        bool[n], equal to trace_rays(...)[1] >= 0 without the closest hit being
        found (a ray stops at its first accepted hit)."""
        rays = _pack_rays("occluded", origins, directions, tmax)
        out = np.full(len(rays), 0xAA, dtype=np.uint8)
        _check(lib().rt2_occluded_host(self._p, rays.ctypes.data, len(rays), out.ctypes.data, int(flags)),
               "rt2_occluded_host")
        if (out > 1).any():
            raise RT2Error("rt2_occluded_host wrote a byte other than 0 or 1")
        return out.astype(bool)

    def occluded_device(self, rays_ptr: int, n: int, out_ptr: int, flags: int = 0, stream: int = 0) -> None:
        """Asynchronous occlusion query over a device array of n rt2_ray records into n bytes (rt2_occluded)."""
        _check(lib().rt2_occluded(self._p, _ptr(rays_ptr), int(n), _ptr(out_ptr), int(flags), _ptr(stream)),
               "rt2_occluded")

    def surface(self, origins, directions, tmax=None, flags: int = 0) -> np.ndarray:
        """What is at the closest hit of n rays (rt2_surface_rays_host, blocking):
        the arguments of trace_rays; returns a SURFACE_DTYPE array of n records.
        dst and tri are trace_rays' result; on a hit mtl and mtl_type are the
        triangle's material index and type, normal the triangle's unit normal
        (it faces the ray), u and v the barycentric weights of b and c, albedo
        the surface's base colour (traceBasic with one bounce and no shadow).
        A miss has tri = mtl = mtl_type = -1, dst = the ray's bound and zeros."""
        rays = _pack_rays("surface", origins, directions, tmax)
        out = np.zeros(len(rays), dtype=SURFACE_DTYPE)
        _check(lib().rt2_surface_rays_host(self._p, rays.ctypes.data, len(rays), out.ctypes.data, int(flags)),
               "rt2_surface_rays_host")
        return out

    def surface_device(self, rays_ptr: int, n: int, out_ptr: int, flags: int = 0, stream: int = 0) -> None:
        """Asynchronous surface query over device arrays of n rt2_ray / rt2_surface records (rt2_surface_rays)."""
        _check(lib().rt2_surface_rays(self._p, _ptr(rays_ptr), int(n), _ptr(out_ptr), int(flags), _ptr(stream)),
               "rt2_surface_rays")

    def camera_rays(self, u: Uniforms, sh: Optional[Shard] = None) -> np.ndarray:
        """The deterministic primary ray of every pixel of the shard's slab
        (rt2_camera_rays_host, blocking): a RAY_DTYPE array of rows * width
        records in slab-row order, the preview's rays bit for bit."""
        sh = sh or shard()
        rows = shard_rows(u.height, sh)
        rays = np.zeros(max(rows, 0) * u.width, dtype=RAY_DTYPE)
        _check(lib().rt2_camera_rays_host(self._p, C.byref(u), sh, rays.ctypes.data), "rt2_camera_rays_host")
        return rays

    def camera_rays_device(self, u: Uniforms, sh: Shard, rays_ptr: int, stream: int = 0) -> None:
        """Asynchronous: the slab's primary rays into a device array of rt2_ray records (rt2_camera_rays)."""
        _check(lib().rt2_camera_rays(self._p, C.byref(u), sh, _ptr(rays_ptr), _ptr(stream)), "rt2_camera_rays")

    def feature_buffers(self, u: Uniforms, sh: Optional[Shard] = None, flags: int = 0) -> dict:
        """First-hit feature buffers of a view, for a denoiser, picking or
        masks: the slab's camera rays are written into a device buffer and
        their surface records follow on the same stream.  Returns slab-shaped
        arrays: depth [rows, W] (1e38 where nothing is hit), tri, mtl and
        mtl_type [rows, W] (-1 where nothing is hit), normal and albedo
        [rows, W, 3], uv [rows, W, 2].  u.numTextures is not consulted: a
        surface query takes the number of images given to set_textures."""
        import torch

        sh = sh or shard()
        rows = shard_rows(u.height, sh)
        if rows < 0:
            raise RT2Error("feature_buffers: bad shard")
        W = int(u.width)
        n = rows * W
        rec = np.zeros(n, dtype=SURFACE_DTYPE)
        if n:
            dev = torch.device("cuda", self.device)
            with torch.cuda.device(dev):
                rays = torch.empty(n * RAY_DTYPE.itemsize, dtype=torch.uint8, device=dev)
                out = torch.empty(n * SURFACE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
                stream = torch.cuda.current_stream(dev).cuda_stream
                self.camera_rays_device(u, sh, rays.data_ptr(), stream)
                self.surface_device(rays.data_ptr(), n, out.data_ptr(), flags, stream)
                rec = out.cpu().numpy().view(SURFACE_DTYPE)  # the copy waits for the stream
        shape = (rows, W)
        return {"depth": rec["dst"].reshape(shape).copy(), "tri": rec["tri"].reshape(shape).copy(),
                "mtl": rec["mtl"].reshape(shape).copy(), "mtl_type": rec["mtl_type"].reshape(shape).copy(),
                "normal": rec["normal"].reshape(shape + (3,)).copy(),
                "albedo": rec["albedo"].reshape(shape + (3,)).copy(),
                "uv": np.stack([rec["u"], rec["v"]], -1).reshape(shape + (2,))}

    def shade_rays(self, origins, directions, light=(0.0, 0.0, 0.0), shadow: bool = False, max_bounce: int = 1,
                   flags: int = 0) -> np.ndarray:
        """The preview shader's colour of n rays (rt2_shade_rays_host, blocking):
        origins and directions (n, 3), used as given; `light`, `shadow` and
        `max_bounce` are the uniforms' basicShadingLightPosition,
        basicShadingShadow and maxBounceCount.  Returns a SHADED_DTYPE array:
        rgb is what traceBasic returns for the ray, segments the closest-hit
        searches it cost (bounces plus the shadow ray).  Every segment is
        unbounded: there is no tmax."""
        rays = _pack_rays("shade_rays", origins, directions)
        out = np.zeros(len(rays), dtype=SHADED_DTYPE)
        opts = shade_opts(light, shadow, max_bounce)
        _check(lib().rt2_shade_rays_host(self._p, rays.ctypes.data, len(rays), C.byref(opts), out.ctypes.data,
                                         int(flags)), "rt2_shade_rays_host")
        return out

    def shade_rays_device(self, rays_ptr: int, n: int, out_ptr: int, light=(0.0, 0.0, 0.0), shadow: bool = False,
                          max_bounce: int = 1, flags: int = 0, stream: int = 0) -> None:
        """Asynchronous shading query over device arrays of n rt2_ray / rt2_shaded records (rt2_shade_rays)."""
        opts = shade_opts(light, shadow, max_bounce)
        _check(lib().rt2_shade_rays(self._p, _ptr(rays_ptr), int(n), C.byref(opts), _ptr(out_ptr), int(flags),
                                    _ptr(stream)), "rt2_shade_rays")

    def preview(self, u: Uniforms, sh: Optional[Shard] = None, flags: int = 0) -> np.ndarray:
        """The preview image of a view through the shading query: the slab's
        camera rays are written into a device buffer and shaded on the same
        stream with the uniforms' basicShadingLightPosition,
        basicShadingShadow and maxBounceCount.  Returns (rows, W, 4) float32
        with alpha 1: the bits of render_host(u with basicShading = 1, 0, 1),
        when u.numTextures is the number of images given to set_textures (at
        most 5), which is what a ray query takes."""
        import torch

        sh = sh or shard()
        rows = shard_rows(u.height, sh)
        if rows < 0:
            raise RT2Error("preview: bad shard")
        W = int(u.width)
        n = rows * W
        img = np.ones((rows, W, 4), dtype=np.float32)
        if n:
            lp = u.basicShadingLightPosition
            dev = torch.device("cuda", self.device)
            with torch.cuda.device(dev):
                rays = torch.empty(n * RAY_DTYPE.itemsize, dtype=torch.uint8, device=dev)
                out = torch.empty(n * SHADED_DTYPE.itemsize, dtype=torch.uint8, device=dev)
                stream = torch.cuda.current_stream(dev).cuda_stream
                self.camera_rays_device(u, sh, rays.data_ptr(), stream)
                self.shade_rays_device(rays.data_ptr(), n, out.data_ptr(), (lp.x, lp.y, lp.z),
                                       bool(u.basicShadingShadow), int(u.maxBounceCount), flags, stream)
                rec = out.cpu().numpy().view(SHADED_DTYPE)  # the copy waits for the stream
            img[..., :3] = rec["rgb"].reshape(rows, W, 3)
        return img

    def radiance(self, origins, directions, rng, max_bounce: int = 8, environmental_light: bool = True,
                 flags: int = 0):
        """The path tracer's radiance along n rays (rt2_radiance_rays_host,
        blocking): origins and directions (n, 3), used as given; rng (n,)
        uint32, one random stream per ray.  Returns (records, rng_out): a
        RADIANCE_DTYPE array (rgb is what trace() returns for the ray, linear;
        segments the closest-hit searches the path cost) and the streams'
        states after the paths' last draws.  The caller's rng array is not
        modified.  Every segment is unbounded: there is no tmax."""
        rays = _pack_rays("radiance", origins, directions)
        state = np.array(rng, dtype=np.uint32).reshape(-1)  # a copy
        if len(rays) != len(state):
            raise RT2Error(f"radiance: {len(rays)} rays for {len(state)} rng states")
        out = np.zeros(len(rays), dtype=RADIANCE_DTYPE)
        opts = path_opts(max_bounce, environmental_light)
        _check(lib().rt2_radiance_rays_host(self._p, rays.ctypes.data, len(rays), C.byref(opts), state.ctypes.data,
                                            out.ctypes.data, int(flags)), "rt2_radiance_rays_host")
        return out, state

    def radiance_device(self, rays_ptr: int, n: int, rng_ptr: int, out_ptr: int, max_bounce: int = 8,
                        environmental_light: bool = True, flags: int = 0, stream: int = 0) -> None:
        """Asynchronous radiance query over device arrays of n rt2_ray records, uint32 stream states (read and
        written) and rt2_radiance records (rt2_radiance_rays)."""
        opts = path_opts(max_bounce, environmental_light)
        _check(lib().rt2_radiance_rays(self._p, _ptr(rays_ptr), int(n), C.byref(opts), _ptr(rng_ptr), _ptr(out_ptr),
                                       int(flags), _ptr(stream)), "rt2_radiance_rays")

    def path_rays(self, u: Uniforms, frame_index: int, sh: Optional[Shard] = None, rng=None):
        """The path tracer's jittered camera rays of the slab's pixels
        (rt2_path_rays_host, blocking).  rng=None seeds every pixel's stream
        for `frame_index` as the render does; otherwise rng (one uint32 per
        slab pixel) is the streams' states, used as found.  Returns (rays,
        rng): a RAY_DTYPE array in slab-row order and the states after the
        three draws of each ray.  The caller's rng array is not modified."""
        sh = sh or shard()
        rows = shard_rows(u.height, sh)
        if rows < 0:
            raise RT2Error("path_rays: bad shard")
        n = rows * int(u.width)
        rays = np.zeros(n, dtype=RAY_DTYPE)
        if rng is None:
            state = np.zeros(n, dtype=np.uint32)
        else:
            state = np.array(rng, dtype=np.uint32).reshape(-1)
            if len(state) != n:
                raise RT2Error(f"path_rays: {len(state)} rng states for {n} pixels")
        _check(lib().rt2_path_rays_host(self._p, C.byref(u), sh, int(frame_index) & 0xFFFFFFFF, int(rng is None),
                                        state.ctypes.data if n else None, rays.ctypes.data if n else None),
               "rt2_path_rays_host")
        return rays, state

    def path_rays_device(self, u: Uniforms, frame_index: int, sh: Shard, reseed: bool, rng_ptr: int, rays_ptr: int,
                         stream: int = 0) -> None:
        """Asynchronous: the slab's path-tracer camera rays into a device array of rt2_ray records, the streams'
        states in a device array of uint32 (rt2_path_rays)."""
        _check(lib().rt2_path_rays(self._p, C.byref(u), sh, int(frame_index) & 0xFFFFFFFF, int(bool(reseed)),
                                   _ptr(rng_ptr), _ptr(rays_ptr), _ptr(stream)), "rt2_path_rays")

    def radiance_image(self, u: Uniforms, frame_index: int, sh: Optional[Shard] = None, flags: int = 0):
        """The linear (HDR) image of one frame of a view: the mean over
        u.numRaysPerPixel samples of trace(), before the tonemap and the sRGB
        encoding that render_host applies.  path_rays_device and
        radiance_device are chained on one stream over device buffers, one
        random stream per pixel seeded for `frame_index`; the samples are added
        in order on the device and divided by numRaysPerPixel in binary32 on
        the host.  Returns ((rows, W, 3) float32, (rows, W) int64 segment
        counts).  u.numTextures is not consulted: a ray query takes the number
        of images given to set_textures.  render_linear_host is the fast form
        of the same image (one launch of the render's own kernel, with
        u.numTextures as the render uses it)."""
        import torch

        sh = sh or shard()
        rows = shard_rows(u.height, sh)
        if rows < 0:
            raise RT2Error("radiance_image: bad shard")
        W, R = int(u.width), int(u.numRaysPerPixel)
        n = rows * W
        total = np.zeros((n, 3), dtype=np.float32)
        segs = np.zeros(n, dtype=np.int64)
        if n and R > 0:
            dev = torch.device("cuda", self.device)
            with torch.cuda.device(dev):
                rays = torch.empty(n * RAY_DTYPE.itemsize, dtype=torch.uint8, device=dev)
                rng = torch.empty(n, dtype=torch.int32, device=dev)
                out = torch.empty(n * RADIANCE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
                acc = torch.zeros((n, 3), dtype=torch.float32, device=dev)
                cnt = torch.zeros(n, dtype=torch.int64, device=dev)
                stream = torch.cuda.current_stream(dev).cuda_stream
                for k in range(R):
                    self.path_rays_device(u, frame_index, sh, k == 0, rng.data_ptr(), rays.data_ptr(), stream)
                    self.radiance_device(rays.data_ptr(), n, rng.data_ptr(), out.data_ptr(), int(u.maxBounceCount),
                                         bool(u.environmentalLight), flags, stream)
                    acc += out.view(torch.float32).view(n, 4)[:, :3]
                    cnt += out.view(torch.int32).view(n, 4)[:, 3]
                total = acc.cpu().numpy()  # the copy waits for the stream
                segs = cnt.cpu().numpy()
        img = total / np.float32(max(R, 1))
        return img.reshape(rows, W, 3), segs.reshape(rows, W)

    def last_kernel(self) -> int:
        """What the scene launched last (rt2_scene_diag): a render's variant id (-1: the traceBasic preview; a linear
        render's: the id + LINEAR_TWIN), or
        after a query QUERY_RES (trace_rays_k5r, every group resident), QUERY_RES_L2 (its L2 continuation),
        QUERY_SCALAR or QUERY_BVH (trace_rays_scalar); after an occlusion query OCCLUDED_RES, OCCLUDED_RES_L2
        (occluded_k5r), OCCLUDED_SCALAR or OCCLUDED_BVH (occluded_scalar); after a surface query SURFACE_RES,
        SURFACE_RES_L2 (surface_k5r), SURFACE_SCALAR or SURFACE_BVH (surface_scalar); after a preview shading query
        SHADE_RES, SHADE_RES_L2 (shade_rays_k5r), SHADE_SCALAR or SHADE_BVH (shade_rays_scalar); after a radiance
        query RADIANCE_RES, RADIANCE_RES_L2 (radiance_rays_k5r), RADIANCE_SCALAR or RADIANCE_BVH
        (radiance_rays_scalar)."""
        c, v = (C.c_ulonglong * 8)(), C.c_int(-1)
        if lib().rt2_scene_diag(self._p, c, C.byref(v)) != 0:
            raise RT2Error("rt2_scene_diag failed")
        return v.value

    def export(self, what: int, dtype) -> np.ndarray:
        """A derived device array of the scene (rt2_scene_export, test hook): 0 =
        pre-transformed triangles, 1/2 = render_mfma records/tau, 3/4 = sweep_k16 records/tau,
        5 = the k5 form's per-triangle m.z residual bounds (float32 pairs), 6 = the kthr records (threshold in
        the K-slots), 7 = the cluster table (one CLUSTER_TABLE_DTYPE record), 8 = the slot table of the resident
        kernel's slot image (one CLUSTER_TABLE_DTYPE record), 9 = its slot_tri (int32 per triangle)."""
        n = lib().rt2_scene_export(self._p, what, None, 0)
        if n < 0:
            raise RT2Error("rt2_scene_export: bad argument")
        out = np.zeros(n // np.dtype(dtype).itemsize, dtype=dtype)
        if n and lib().rt2_scene_export(self._p, what, out.ctypes.data, n) != n:
            raise RT2Error("rt2_scene_export failed")
        return out

    def cluster_table(self) -> np.ndarray:
        """The scene's cluster table (rt2_scene_export selector 7): one CLUSTER_TABLE_DTYPE record."""
        return self.export(7, CLUSTER_TABLE_DTYPE)[0]

    def set_cluster_table(self, table) -> None:
        """Replaces the scene's cluster table (rt2_scene_set_clusters, test hook)."""
        t = np.zeros(1, dtype=CLUSTER_TABLE_DTYPE)
        t[0] = table
        _check(lib().rt2_scene_set_clusters(self._p, t.ctypes.data), "rt2_scene_set_clusters")

    def slot_table(self) -> np.ndarray:
        """The table over the slot groups of the resident kernel's slot image (rt2_scene_export selector 8)."""
        return self.export(8, CLUSTER_TABLE_DTYPE)[0]

    def slot_tri(self) -> np.ndarray:
        """The slot order (rt2_scene_export selector 9): slot s holds triangle slot_tri[s]."""
        return self.export(9, np.int32)

    def set_slot_order(self, slot_tri, table) -> None:
        """Installs an explicit slot order and its table (rt2_scene_set_slot_order, test hook)."""
        st = np.ascontiguousarray(slot_tri, dtype=np.int32)
        if len(st) != self.n_tris:
            raise RT2Error("set_slot_order: one slot per triangle")
        t = np.zeros(1, dtype=CLUSTER_TABLE_DTYPE)
        t[0] = table
        _check(lib().rt2_scene_set_slot_order(self._p, st.ctypes.data, t.ctypes.data), "rt2_scene_set_slot_order")

    def mfma_probe(self, layout: int, rays: np.ndarray):
        """The matrix filter's terms on the device (rt2_mfma_probe, test hook):
        rays (n, 8) float32 {o, best, d, 0}, n a multiple of 64; layout 0 =
        16x16x32 (render_mfma), 1 = k16, 2 = its 5-product form (k5), 3 = k5 with the threshold in the
        accumulator (cthr: U, -V, X, Y shifted by TT, TT in slot 3), 4 = layout 3 with the fragments built in
        registers (frag_pair: the operand path of the shipping kernels), 5 = the threshold in the K-slots (kthr:
        U, -V, X, Y; slot 3 zero; frag_pair fragments), 6 = layout 5 with each ray's own W, 7 = layout 6's U, -V, X
        by the 16-row products of MfmaSpec::cluster_rows16 (slots 3, 4 zero), 8 = the same by the 8-row products of
        MfmaSpec::cluster_rows8.  Returns (terms [n, n_pad, 5], frags [n, 48] float16
        (layouts 4, 5: [n, 80], the register fragments at 48..63 and 64..79), rinfo [n, 8], accept [n, n_tris]
        bool)."""
        rays = np.ascontiguousarray(rays, dtype=np.float32)
        n = rays.shape[0]
        g = 32 if layout >= 1 else 16
        n_pad = -(-self.n_tris // g) * g
        terms = np.zeros((n, n_pad, 5), dtype=np.float32)
        frags = np.zeros((n, 80), dtype=np.uint16)
        rinfo = np.zeros((n, 8), dtype=np.float32)
        acc = np.zeros((n, self.n_tris), dtype=np.uint8)
        _check(lib().rt2_mfma_probe(self._p, layout, rays.ctypes.data, n, terms.ctypes.data, frags.ctypes.data,
                                    rinfo.ctypes.data, acc.ctypes.data), "rt2_mfma_probe")
        frags = frags.view(np.float16)
        return terms, (frags if layout >= 4 else np.ascontiguousarray(frags[:, :48])), rinfo, acc.astype(bool)

    def cost_map(self) -> np.ndarray | None:
        """The per-pixel cost map of the last cost-ordered launch (test hook
        rt2_scene_cost_map; shader clocks), or None when there is none."""
        fn = lib().rt2_scene_cost_map
        fn.restype = C.c_longlong
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_ulonglong]
        n = fn(self._p, None, 0)
        if n <= 0:
            return None
        out = np.zeros(n, dtype=np.uint32)
        if fn(self._p, out.ctypes.data, n) != n:
            raise RT2Error("rt2_scene_cost_map failed")
        return out

    def stats(self, reset: bool = False) -> Stats:
        s = Stats()
        _check(lib().rt2_scene_stats(self._p, C.byref(s), int(reset)), "stats")
        return s


def cluster_table(triangles: np.ndarray) -> np.ndarray:
    """The cluster table rt2_scene_create derives for a triangle list
    (rt2_cluster_table_build, host only): one CLUSTER_TABLE_DTYPE record; n = 0
    when no cluster is compact."""
    triangles = np.ascontiguousarray(triangles, dtype=TRI_DTYPE)
    t = np.zeros(1, dtype=CLUSTER_TABLE_DTYPE)
    if lib().rt2_cluster_table_build(triangles.ctypes.data, len(triangles), t.ctypes.data) < 0:
        raise RT2Error(f"rt2_cluster_table_build: {lib().rt2_last_error().decode()}")
    return t[0]


def cluster_order(triangles: np.ndarray):
    """The slot order rt2_scene_create derives for a triangle list of at most 38
    groups (rt2_cluster_order_build, host only): (slot_tri int32 [n], the table
    over the slot groups).  The identity with rt2_cluster_table_build's table
    where the rule's own order does not project cheaper."""
    triangles = np.ascontiguousarray(triangles, dtype=TRI_DTYPE)
    st = np.zeros(len(triangles), dtype=np.int32)
    t = np.zeros(1, dtype=CLUSTER_TABLE_DTYPE)
    if lib().rt2_cluster_order_build(triangles.ctypes.data, len(triangles), st.ctypes.data, t.ctypes.data) < 0:
        raise RT2Error(f"rt2_cluster_order_build: {lib().rt2_last_error().decode()}")
    return st, t[0]


def cluster_need(table, o: np.ndarray, d: np.ndarray) -> np.ndarray:
    """Bit k of element i: ray i (origin o[i], direction d[i]) needs cluster k
    of `table`, by the arithmetic the kernel runs (rt2_cluster_need, host only)."""
    t = np.zeros(1, dtype=CLUSTER_TABLE_DTYPE)
    t[0] = table
    rays = np.zeros(len(o), dtype=RAY_DTYPE)
    rays["o"], rays["d"] = o, d
    bits = np.zeros(len(rays), dtype=np.uint32)
    _check(lib().rt2_cluster_need(t.ctypes.data, rays.ctypes.data, len(rays), bits.ctypes.data), "rt2_cluster_need")
    return bits


def has_variant(v: int) -> bool:
    """Whether kernel variant v is compiled into the loaded library (experiment
    variants need make EXPERIMENTS=1 and RT2_LIB=exp)."""
    return v == 0 or lib().rt2_variant_name(v) is not None


def resolve_rgba32f(accum_ptr: int, n_pixels: int, frames: int, out_ptr: int, stream: int = 0) -> None:
    _check(lib().rt2_resolve_rgba32f(C.c_void_p(accum_ptr), n_pixels, frames, C.c_void_p(out_ptr),
                                     _ptr(stream)), "resolve")


def resolve_tonemap(sum_ptr: int, n_pixels: int, frames: int, out_ptr: int, stream: int = 0) -> None:
    """Device resolve of a linear sum (Scene.render_linear) to the render's display value: srgb1(aces1(sum /
    frames)) per channel, alpha = 1 (rt2_resolve_tonemap); asynchronous."""
    _check(lib().rt2_resolve_tonemap(_ptr(sum_ptr), n_pixels, frames, _ptr(out_ptr), _ptr(stream)),
           "rt2_resolve_tonemap")


def resolve_rgb8_reference(acc8: np.ndarray, frames: int) -> np.ndarray:
    acc8 = np.ascontiguousarray(acc8, dtype=np.uint32)
    n = acc8.size // 4
    out = np.zeros(acc8.shape[:-1] + (3,), dtype=np.uint8)
    _check(lib().rt2_resolve_rgb8_reference(acc8.ctypes.data, n, frames, out.ctypes.data), "resolve_rgb8")
    return out


def write_png(path: str, img: np.ndarray) -> None:
    img = np.ascontiguousarray(img, dtype=np.uint8)
    h, w = img.shape[:2]
    comps = 1 if img.ndim == 2 else img.shape[2]
    _check(lib().rt2_write_png(path.encode(), w, h, comps, img.ctypes.data, w * comps), "write_png")


def device_selftest(x: np.ndarray) -> np.ndarray:
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = np.zeros((len(x), 10), dtype=np.float32)
    _check(lib().rt2_device_selftest(x.ctypes.data, len(x), out.ctypes.data), "device_selftest")
    return out


# rt2_device_numerics (test hook): the operation codes of numerics_kernel, which oracle_numerics shares.  Operands
# are words of a 9-word row (vectors in words 0-2 and 3-5, a trailing scalar in word 6), results words of a 4-word
# row (refract_: xyz + its flag; rnd: value, new state; rnd_dir: xyz + new state).
NUMERICS_OPS = {name: code for code, name in enumerate((
    "div", "rcp", "sqrt", "fma", "mul", "add", "sub", "fmin", "fmax", "clamp", "dot", "cross", "length",
    "normalize", "reflect", "refract", "mix", "smoothstep", "exp", "log", "acos", "cos", "sin", "pow", "aces1",
    "srgb1", "sky", "rnd", "rnd_dir"))}


def device_numerics(op, rows: np.ndarray) -> np.ndarray:
    """One operation of DESIGN.md §Numerics on the device, by the functions the kernels call: rows is (n, 9) uint32
    bit patterns (fewer columns are padded with zeros), the result (n, 4) uint32; one launch."""
    code = NUMERICS_OPS[op] if isinstance(op, str) else int(op)
    rows = np.asarray(rows, dtype=np.uint32)
    assert rows.ndim == 2 and rows.shape[1] <= 9
    full = np.zeros((len(rows), 9), np.uint32)
    full[:, :rows.shape[1]] = rows
    out = np.zeros((len(rows), 4), np.uint32)
    _check(lib().rt2_device_numerics(code, full.ctypes.data, len(full), out.ctypes.data), "device_numerics")
    return out


from .scenes import (REF_DATA_ENV, build_config_scene, config_spec, generate_torus_obj,  # noqa: E402,F401
                     CONFIGS)
