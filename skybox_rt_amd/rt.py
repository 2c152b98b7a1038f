"""ctypes binding of include/vx_rt.h (librtapp.so): the RT regression app.

    scene = Scene.load("tekkaman.cgltrace")
    r = Renderer(scene)
    r.configure(1024, 1024, shadows=True)
    r.render()
    fb = r.framebuffer()          # uint32 ARGB8888 [H, W], row 0 = NDC y=-1
    stats = r.stats()

All work runs through the native library and the HIP driver; there is no
fallback.  Errors raise RtError with the library's message.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib

RT_RENDER_SHADOWS = 0x1
RT_RENDER_PATH = 0x8
RT_RENDER_FLAT = 0x10
RT_RENDER_RASTER = 0x20
RT_RENDER_BVH2 = 0x40
PT_SEED = 0x5EED
RT_RENDER_INSTRUMENTED = 0x100
RT_RENDER_COMPACT = 0x200
RT_RENDER_COUNTERS = 0x400
RT_RENDER_HOST_SETUP = 0x800
RT_RENDER_BVH_WALK = 0x2000
RT_SCENE_OM_LAYERS = 0x1
# rt_renderer_export_records arrays: name -> (id, dtype, words per record)
RECORDS = {"prims": (0, np.int32, 32), "bbox": (1, np.uint32, 2), "vis": (2, np.uint32, 4),
           "vnodes": (3, np.uint32, 16), "vtris": (4, np.int32, 16), "vlayers": (5, np.int32, 16),
           "vgeom": (6, np.int32, 16), "order": (7, np.uint32, 1), "ptris": (8, np.float32, 12),
           "geom": (9, np.float32, 12), "bidx": (10, np.uint32, 2), "blist": (11, np.uint32, 4),
           "cdesc": (14, np.uint32, 4), "cdesc_host": (15, np.uint32, 4),
           "sidx": (12, np.uint32, 2), "slist": (13, np.float32, 12),
           "oidx": (16, np.uint32, 2), "olist": (17, np.uint32, 1),
           "bglayer": (18, np.uint32, 2), "bglayer_host": (19, np.uint32, 2),
           "btidx": (20, np.uint32, 2), "btrim": (21, np.uint32, 4),
           "btidx_host": (22, np.uint32, 2), "btrim_host": (23, np.uint32, 4)}
RT_BVH_STACK4_UNUSED = 0xFFFFFFFF
RT_BVH_BUILD_HOST = 2
CLEAR_COLOR = 0xFF000000               # draw3d/main.cpp:47
DEFAULT_LIGHT = (0.0, 60.0, 80.0)      # clip (x, y, w), SURVEY.md 8(d) config 3
TILE = 32                              # RASTER_TILE_LOGSIZE = 5


class SceneInfo(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in (
        "num_drawcalls", "num_prims", "num_geometry", "num_layer", "num_textures",
        "bvh_nodes", "bvh_tris", "bvh_leaves", "bvh_depth", "bvh4_nodes", "bvh4_depth",
        "bvh4_stack", "bvh4_f16")] + [
        ("parse_ms", C.c_double), ("bvh_ms", C.c_double)]


class BvhBuildStats(C.Structure):
    _fields_ = [("nodes", C.c_uint32), ("depth", C.c_uint32), ("launches", C.c_uint32),
                ("stack4", C.c_uint32), ("build_ms", C.c_double), ("kernel_ms", C.c_double),
                ("nodes4", C.c_uint32), ("depth4", C.c_uint32), ("method", C.c_uint32),
                ("pad", C.c_uint32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "pad"}


class SetupStats(C.Structure):
    _fields_ = [("device", C.c_uint32), ("launches", C.c_uint32), ("heavy_tiles", C.c_uint32),
                ("blist_blocks", C.c_uint32), ("setup_ms", C.c_double), ("configure_ms", C.c_double),
                ("blist_entries", C.c_uint64), ("blist_max", C.c_uint32), ("slist_on", C.c_uint32),
                ("slist_entries", C.c_uint64), ("path_queue", C.c_uint32), ("slist_built", C.c_uint32),
                ("slist_stale", C.c_uint32), ("lane_grid", C.c_uint32),
                ("bg_first_chunk", C.c_uint32), ("tier_groups", C.c_uint32),
                ("btrim_entries", C.c_uint64), ("btrim_blocks", C.c_uint32), ("fused_chunk", C.c_uint32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "pad"}


class LightInfo(C.Structure):
    _fields_ = [("light", C.c_float * 3), ("slist_on", C.c_uint32), ("slist_entries", C.c_uint64)]


RT_MAX_LIGHTS = 16
RT_MAX_PATH_LIGHTS = 8
# rt_aov_t (vx_rt.h): one visibility record per framebuffer pixel
AOV_DTYPE = np.dtype([("pid", "<i4"), ("depth_flags", "<u4"), ("t", "<f4"), ("light_mask", "<u4")])
# a denoise guide record (vx_rt.h rt_denoise_guide_t): normal = signed bytes x | y << 8 | z << 16
DENOISE_GUIDE_DTYPE = np.dtype([("pid", "<i4"), ("depth_flags", "<u4"), ("normal", "<u4"), ("reserved", "<u4")])
DENOISE_PASSES, DENOISE_DEPTH_SHIFT, DENOISE_COLOR_SHIFT = 2, 2, 3   # vx_rt.h RT_DENOISE_DEFAULT_*
RT_AOV_DEPTH_MASK = 0xFFFFFF
RT_AOV_GEOM = 0x01000000
RT_AOV_SHADOW_RAY = 0x02000000
# ambient occlusion (vx_rt.h rt_ao_params_t, RT_AO_GREY / RT_AO_MODULATE)
AO_SEED = PT_SEED
AO_MODES = {"grey": 0, "modulate": 1}


class AoParams(C.Structure):
    _fields_ = [("radius", C.c_float), ("seed", C.c_uint32)]


# soft shadows (vx_rt.h rt_soft_params_t, RT_SOFT_DEFAULT_SEED, RT_SOFT_LIT / RT_SOFT_GREY)
RT_SOFT_DEFAULT_SEED = 0x5EED
RT_SOFT_MAX_SAMPLES = 1024
SOFT_MODES = {"lit": 0, "grey": 1}


class SoftParams(C.Structure):
    _fields_ = [("radii", C.POINTER(C.c_float)), ("n", C.c_uint32), ("seed", C.c_uint32)]


# caller-supplied rays (vx_rt.h rt_ray_t / rt_hit_t / rt_query_buffers_t, RT_QUERY_*)
RAY_DTYPE = np.dtype([("o", "<f4", 3), ("tmin", "<f4"), ("d", "<f4", 3), ("tmax", "<f4")])
HIT_DTYPE = np.dtype([("pid", "<i4"), ("t", "<f4")])
QUERY_MODES = {"closest": 0, "any": 1}
RT_QUERY_SKIP, RT_QUERY_PERM = 0x1, 0x2
RT_QUERY_MISS_KEY = 0xFFFFFFFF


class QueryBuffers(C.Structure):
    _fields_ = [("rays", C.c_void_p), ("hits", C.c_void_p), ("skip", C.c_void_p), ("perm", C.c_void_p),
                ("keys", C.c_void_p), ("capacity", C.c_uint64), ("box", C.c_float * 6)]


class RenderParams(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("flags", C.c_uint32),
                ("light", C.c_float * 3), ("clear_color", C.c_uint32),
                ("shard_index", C.c_uint32), ("shard_count", C.c_uint32),
                ("bounces", C.c_uint32), ("seed", C.c_uint32), ("tile_logsize", C.c_uint32)]


class Stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in (
        "primary_rays", "shadow_rays", "geometry_hits", "occluded", "node_visits",
        "tri_tests", "layer_tests", "shaded", "texel_bytes", "tasks")] + [
        ("kernel_ms", C.c_double), ("grid", C.c_uint32), ("block", C.c_uint32),
        ("num_tasks", C.c_uint32), ("local_tiles", C.c_uint32), ("bounce_rays", C.c_uint64),
        ("rect_tests", C.c_uint64), ("edge_tests", C.c_uint64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class RtError(RuntimeError):
    pass


_h = None


def lib():
    global _h
    if _h is None:
        h = _lib.load("librtapp.so")
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        sig = {
            "rt_scene_load": [C.c_char_p, C.POINTER(vp)],
            "rt_scene_load_ex": [C.c_char_p, u32, u32, u32, C.POINTER(vp)],
            "rt_scene_om_split": [vp, C.POINTER(u32), C.POINTER(u32)],
            "rt_scene_setup_olists": [vp, u32, u32, vp, vp, C.POINTER(u64), C.POINTER(u64)],
            "rt_scene_free": [vp],
            "rt_scene_info": [vp, C.POINTER(SceneInfo)],
            "rt_scene_export_prims": [vp, vp, u64],
            "rt_scene_export_bvh": [vp, vp, vp],
            "rt_scene_export_bvh4": [vp, vp],
            "rt_renderer_build_bvh": [vp, C.POINTER(BvhBuildStats)],
            "rt_renderer_build_bvh_ex": [vp, u32, C.POINTER(BvhBuildStats)],
            "rt_renderer_bvh_stats": [vp, C.POINTER(BvhBuildStats)],
            "rt_renderer_export_bvh": [vp, vp, vp, C.POINTER(u32), C.POINTER(u32)],
            "rt_renderer_export_bvh4": [vp, vp, C.POINTER(u32)],
            "rt_renderer_export_bvh4h": [vp, vp, C.POINTER(u32)],
            "rt_renderer_export_vis_tree": [vp, vp, C.POINTER(u32), vp, C.POINTER(u32)],
            "rt_renderer_create": [vp, C.c_char_p, C.POINTER(vp)],
            "rt_renderer_free": [vp],
            "rt_renderer_configure": [vp, C.POINTER(RenderParams)],
            "rt_render_start": [vp],
            "rt_render_wait": [vp],
            "rt_render": [vp],
            "rt_render_stats": [vp, C.POINTER(Stats)],
            "rt_render_kernel_ms": [vp, C.POINTER(C.c_double)],
            "rt_render_run_totals": [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64),
                                     C.POINTER(C.c_uint64)],
            "rt_render_set_timing": [vp, C.c_int],
            "rt_read_framebuffer": [vp, vp, u64],
            "rt_read_framebuffer_prev": [vp, vp, u64],
            "rt_read_depthbuffer": [vp, vp, u64],
            "rt_launch_rows": [vp, vp, u64, C.POINTER(u64)],
            "rt_scene_setup_prims": [vp, u32, u32, vp, u64],
            "rt_scene_setup_vis": [vp, u32, u32, vp, u64],
            "rt_scene_bg_layers": [vp, u32, u32, vp, u32, vp, u64, C.POINTER(u64)],
            "rt_scene_block_trim": [vp, u32, u32, u32, u32, vp, vp, vp, vp, C.POINTER(u64), C.POINTER(u64)],
            "rt_scene_vis_tree": [vp, u32, u32, C.c_float, vp, C.POINTER(u32), vp, C.POINTER(u32),
                                  C.POINTER(u32)],
            "rt_framebuffer_device": [vp, C.POINTER(vp), C.POINTER(u64)],
            "rt_device_stream": [vp, C.POINTER(vp)],
            "rt_device_caps": [vp, C.POINTER(u64)],
            "rt_render_gather": [vp, vp, vp],
            "rt_renderer_setup_stats": [vp, C.POINTER(SetupStats)],
            "rt_renderer_set_light": [vp, C.POINTER(C.c_float)],
            "rt_renderer_set_list_policy": [vp, u32],
            "rt_renderer_export_records": [vp, u32, vp, u64, C.POINTER(u64)],
            "rt_renderer_accum_begin": [vp],
            "rt_renderer_accum_reset": [vp],
            "rt_render_accumulate_start": [vp, u32],
            "rt_render_accumulate": [vp, u32],
            "rt_renderer_accum_samples": [vp, C.POINTER(u32)],
            "rt_read_accum": [vp, vp, u64],
            "rt_renderer_set_lights": [vp, vp, u32],
            "rt_renderer_set_path_lights": [vp, vp, u32],
            "rt_renderer_lights_info": [vp, C.POINTER(LightInfo), u32, C.POINTER(u32)],
            "rt_renderer_export_light_lists": [vp, u32, u32, vp, u64, C.POINTER(u64)],
            "rt_render_aov_start": [vp],
            "rt_render_aov": [vp],
            "rt_read_aov": [vp, vp, u64],
            "rt_relight_capture_start": [vp],
            "rt_relight_capture": [vp],
            "rt_render_relight_start": [vp, vp, u32],
            "rt_render_relight": [vp, vp, u32],
            "rt_read_relight_base": [vp, vp, u64],
            "rt_denoise_capture_start": [vp],
            "rt_denoise_capture": [vp],
            "rt_render_denoise_start": [vp, vp],
            "rt_render_denoise": [vp, vp],
            "rt_read_denoise_guide": [vp, vp, vp, u64],
            "rt_write_accum": [vp, vp, u64, u32],
            "rt_renderer_ao_begin": [vp, C.POINTER(AoParams)],
            "rt_renderer_ao_reset": [vp],
            "rt_render_ao_start": [vp, u32],
            "rt_render_ao": [vp, u32],
            "rt_renderer_ao_samples": [vp, C.POINTER(u32)],
            "rt_read_ao": [vp, vp, u64],
            "rt_render_ao_resolve_start": [vp, u32, vp, u32],
            "rt_render_ao_resolve": [vp, u32, vp, u32],
            "rt_renderer_soft_begin": [vp, C.POINTER(SoftParams)],
            "rt_renderer_soft_reset": [vp],
            "rt_render_soft_start": [vp, u32],
            "rt_render_soft": [vp, u32],
            "rt_renderer_soft_samples": [vp, C.POINTER(u32)],
            "rt_read_soft": [vp, vp, u64],
            "rt_render_soft_resolve_start": [vp, u32, vp, u32],
            "rt_render_soft_resolve": [vp, u32, vp, u32],
            "rt_query_reserve": [vp, u64],
            "rt_query_buffers": [vp, C.POINTER(QueryBuffers)],
            "rt_query_write_rays": [vp, vp, u64, u64],
            "rt_query_write_skip": [vp, vp, u64, u64],
            "rt_query_write_perm": [vp, vp, u64, u64],
            "rt_query_trace_start": [vp, u64, u32, u32],
            "rt_query_trace": [vp, u64, u32, u32],
            "rt_query_keys_start": [vp, u64],
            "rt_query_keys": [vp, u64],
            "rt_query_read_hits": [vp, vp, u64, u64],
            "rt_query_read_keys": [vp, vp, u64, u64],
        }
        for name, argtypes in sig.items():
            fn = getattr(h, name)
            fn.argtypes = argtypes
            fn.restype = C.c_int
        h.rt_accum_resolve.argtypes = [C.POINTER(u32), u32]
        h.rt_accum_resolve.restype = u32
        h.rt_lights_resolve.argtypes = [u32, u32, u32]
        h.rt_lights_resolve.restype = u32
        h.rt_path_lights_resolve.argtypes = [C.POINTER(u32), u32, u32]
        h.rt_path_lights_resolve.restype = u32
        h.rt_aov_relight.argtypes = [u32, u32, u32]
        h.rt_aov_relight.restype = u32
        h.rt_relight_resolve.argtypes = [u32, u32, u32, vp, u32]
        h.rt_relight_resolve.restype = u32
        h.rt_ao_resolve.argtypes = [u32, u32, u32]
        h.rt_ao_resolve.restype = u32
        h.rt_soft_resolve.argtypes = [u32, u32, vp, u32, vp, u32]
        h.rt_soft_resolve.restype = u32
        h.rt_query_key.argtypes = [vp, C.POINTER(C.c_float)]
        h.rt_query_key.restype = u32
        h.rt_last_error.restype = C.c_char_p
        h.rt_last_error.argtypes = []
        _h = h
    return _h


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise RtError(f"{what} failed ({rc}): {lib().rt_last_error().decode(errors='replace')}")


class Scene:
    def __init__(self, handle):
        self._h = handle

    @classmethod
    def load(cls, path: str, om_layers: bool = False) -> "Scene":
        """om_layers=True (RT_SCENE_OM_LAYERS): a scene the RT path cannot
        trace as a whole (blending, stencil, colour masks, layers after
        geometry) is split at the first such drawcall; its plain and shadow
        frames trace the drawcalls before it and fold the rest -- the ordered
        tail -- over them through the output merger (kernels/rt_om_kernel.hip)."""
        h = C.c_void_p()
        if om_layers:
            _check(lib().rt_scene_load_ex(str(path).encode(), 0, 0xFFFFFFFF, RT_SCENE_OM_LAYERS,
                                          C.byref(h)), f"rt_scene_load_ex({path})")
        else:
            _check(lib().rt_scene_load(str(path).encode(), C.byref(h)), f"rt_scene_load({path})")
        return cls(h)

    def om_split(self):
        """(first drawcall of the ordered tail, tail primitives); the drawcall
        count and 0 when the tail is empty or the scene was loaded without om_layers."""
        k, n = C.c_uint32(), C.c_uint32()
        _check(lib().rt_scene_om_split(self._h, C.byref(k), C.byref(n)), "rt_scene_om_split")
        return k.value, n.value

    def setup_olists(self, width: int, height: int):
        """The ordered tail's per-block lists at width x height (one shard):
        (idx uint32[blocks, 2] = first entry, count per 8x8 block in bidx's
        numbering; ent uint32[entries] = primitive indices, ascending per block)."""
        ne, nb = C.c_uint64(), C.c_uint64()
        _check(lib().rt_scene_setup_olists(self._h, width, height, None, None, C.byref(ne), C.byref(nb)),
               "rt_scene_setup_olists")
        idx = np.zeros((max(nb.value, 1), 2), np.uint32)
        ent = np.zeros(max(ne.value, 1), np.uint32)
        _check(lib().rt_scene_setup_olists(self._h, width, height, idx.ctypes.data, ent.ctypes.data,
                                           C.byref(ne), C.byref(nb)), "rt_scene_setup_olists")
        return idx[:nb.value], ent[:ne.value]

    def info(self) -> dict:
        i = SceneInfo()
        _check(lib().rt_scene_info(self._h, C.byref(i)), "rt_scene_info")
        return {n: getattr(i, n) for n, _ in i._fields_ if n not in ("pad", "pad8")}

    def prims(self) -> np.ndarray:
        n = self.info()["num_prims"]
        out = np.zeros((max(n, 1), 3, 10), np.float32)
        _check(lib().rt_scene_export_prims(self._h, out.ctypes.data, n), "rt_scene_export_prims")
        return out[:n]

    def bvh(self):
        info = self.info()
        nodes = np.zeros((max(info["bvh_nodes"], 1), 16), np.float32)
        tris = np.zeros((max(info["bvh_tris"], 1), 12), np.float32)
        _check(lib().rt_scene_export_bvh(self._h, nodes.ctypes.data, tris.ctypes.data),
               "rt_scene_export_bvh")
        return nodes[:info["bvh_nodes"]], tris[:info["bvh_tris"]]

    def bvh4(self):
        """The 4-wide BVH nodes (float32[N4, 32], rt_node4_t); leaves index bvh()'s tris."""
        n = self.info()["bvh4_nodes"]
        nodes4 = np.zeros((max(n, 1), 32), np.float32)
        _check(lib().rt_scene_export_bvh4(self._h, nodes4.ctypes.data), "rt_scene_export_bvh4")
        return nodes4[:n]

    def setup_prims(self, width: int, height: int) -> np.ndarray:
        """rt_prim_t shading records (int32[P, 32]) at width x height."""
        n = self.info()["num_prims"]
        out = np.zeros((max(n, 1), 32), np.int32)
        _check(lib().rt_scene_setup_prims(self._h, width, height, out.ctypes.data, n),
               "rt_scene_setup_prims")
        return out[:n]

    def bg_layers(self, width: int, height: int, order=None, first_chunk: int = 0) -> np.ndarray:
        """The background-layer table (uint32[chunks - first_chunk, 2]: pid + 1 of the one
        screen layer over the chunk's 8x8 block -- 0xffffffff none, 0 mixed or off the image --
        and its drawcall) of a width x height frame, computed on the host; `order`: the 32x32
        tiles' work order (default row-major), 16 chunks a tile."""
        tiles = ((width + 31) // 32) * ((height + 31) // 32)
        o = None if order is None else np.ascontiguousarray(order, np.uint32)
        assert o is None or o.size == tiles
        out = np.zeros((tiles * 16, 2), np.uint32)
        n = C.c_uint64()
        _check(lib().rt_scene_bg_layers(self._h, width, height, None if o is None else o.ctypes.data,
                                        first_chunk, out.ctypes.data, tiles * 16, C.byref(n)),
               "rt_scene_bg_layers")
        return out[:n.value]

    def block_trim(self, width: int, height: int, shard_index: int = 0, shard_count: int = 1):
        """The per-block candidate lists of a width x height frame (one shard) and the same lists
        trimmed to the entries whose primitive wins a pixel of the block, computed on the host:
        (bidx uint32[blocks, 2], blist uint32[entries + 3, 4], btidx, btrim) -- btidx keeps bidx's
        first entry beside the kept count, btrim the kept entries at the front of each list's slots."""
        ne, nb = C.c_uint64(), C.c_uint64()
        _check(lib().rt_scene_block_trim(self._h, width, height, shard_index, shard_count, None, None, None, None,
                                         C.byref(ne), C.byref(nb)), "rt_scene_block_trim")
        bidx, btidx = (np.zeros((max(nb.value, 1), 2), np.uint32) for _ in range(2))
        blist, btrim = (np.zeros((ne.value + 3, 4), np.uint32) for _ in range(2))
        _check(lib().rt_scene_block_trim(self._h, width, height, shard_index, shard_count, bidx.ctypes.data,
                                         blist.ctypes.data, btidx.ctypes.data, btrim.ctypes.data, C.byref(ne),
                                         C.byref(nb)), "rt_scene_block_trim")
        return bidx[:nb.value], blist, btidx[:nb.value], btrim

    def setup_vis(self, width: int, height: int) -> np.ndarray:
        """Primary-visibility records (uint32[P, 3]: covered-pixel rectangle
        x0|x1<<16, y0|y1<<16 inclusive, depth-word lower bound) at width x height."""
        n = self.info()["num_prims"]
        out = np.zeros((max(n, 1), 3), np.uint32)
        _check(lib().rt_scene_setup_vis(self._h, width, height, out.ctypes.data, n),
               "rt_scene_setup_vis")
        return out[:n]

    def vis_tree(self, width: int, height: int, depth_scale: float = 0.0):
        """The primary rays' screen-space BVH4 at width x height: (refs
        int32[N, 4], leaf_pids int32[M], worst-case stack)."""
        nn, nl, st = C.c_uint32(), C.c_uint32(), C.c_uint32()
        _check(lib().rt_scene_vis_tree(self._h, width, height, depth_scale, None, C.byref(nn), None,
                                       C.byref(nl), C.byref(st)), "rt_scene_vis_tree")
        refs = np.zeros((max(nn.value, 1), 4), np.int32)
        pids = np.zeros(max(nl.value, 1), np.int32)
        _check(lib().rt_scene_vis_tree(self._h, width, height, depth_scale, refs.ctypes.data,
                                       C.byref(nn), pids.ctypes.data, C.byref(nl), C.byref(st)),
               "rt_scene_vis_tree")
        return refs[:nn.value], pids[:nl.value], st.value

    def close(self) -> None:
        if self._h:
            lib().rt_scene_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Renderer:
    """One vortex device running the RT kernel for one scene."""

    def __init__(self, scene: Scene, kernel_dir: str = None):
        self.scene = scene
        h = C.c_void_p()
        _check(lib().rt_renderer_create(scene._h, kernel_dir.encode() if kernel_dir else None,
                                        C.byref(h)), "rt_renderer_create")
        self._h = h
        self.params = None
        self._query_keep = []   # the tensors whose queued copies trace_rays() / query_keys() started
        # the tree rt_renderer_create built: on the device (binned SAH, the
        # host build's arrays) unless env RT_BVH=host
        st = self.bvh_stats()
        self.gpu_bvh = st["method"] != RT_BVH_BUILD_HOST
        self.gpu_bvh4 = self.gpu_bvh and st["stack4"] != RT_BVH_STACK4_UNUSED

    def configure(self, width: int, height: int, shadows: bool = True, light=DEFAULT_LIGHT,
                  clear_color: int = CLEAR_COLOR, shard_index: int = 0, shard_count: int = 1,
                  instrumented: bool = False, path: bool = False, bounces: int = 4,
                  seed: int = PT_SEED, flat: bool = False, raster: bool = False,
                  bvh_width: int = 0, compact: bool = False, counters: bool = True,
                  host_setup: bool = False, bvh_walk: bool = False) -> None:
        """path=True: diffuse path trace (pt_kernel; `bounces` segments per
        path, RNG `seed`) instead of primary + shadow rays.  flat=True: the
        flat triangle list without BVH (BASELINE config 2).  raster=True:
        the draw3d raster pipeline (any scene; depth/stencil/blend).
        bvh_width: 2 = traverse the binary BVH, 0 = the default (the 4-wide
        BVH unless env RT_BVH_WIDTH=2).  compact=True: the shard layout
        (tile order, as for shard_count > 1) for a single shard too.
        counters=False: no per-workgroup counter rows (the timed product
        configuration; stats() then has the task count and kernel time only).
        host_setup=True: build the per-resolution records with the host loops
        instead of on the device (kernels/rt_setup.hip).  bvh_walk=True: no
        per-block / light-space lists -- primary visibility by the BVH4 packet
        walk, shadow rays by the BVH (BASELINE config 3's full BVH traversal;
        primary+shadow frames run the rt_bvh image)."""
        p = RenderParams()
        p.width, p.height = width, height
        p.flags = ((RT_RENDER_SHADOWS if shadows else 0) | (RT_RENDER_INSTRUMENTED if instrumented else 0)
                   | (RT_RENDER_PATH if path else 0) | (RT_RENDER_FLAT if flat else 0)
                   | (RT_RENDER_RASTER if raster else 0) | (RT_RENDER_BVH2 if bvh_width == 2 else 0)
                   | (RT_RENDER_COMPACT if compact else 0) | (RT_RENDER_COUNTERS if counters else 0)
                   | (RT_RENDER_HOST_SETUP if host_setup else 0) | (RT_RENDER_BVH_WALK if bvh_walk else 0))
        p.bounces, p.seed = bounces, seed
        p.light[:] = [float(np.float32(x)) for x in light]
        p.clear_color = clear_color
        p.shard_index, p.shard_count = shard_index, shard_count
        _check(lib().rt_renderer_configure(self._h, C.byref(p)), "rt_renderer_configure")
        self.params = p
        self.bvh4 = (bvh_width != 2 and os.environ.get("RT_BVH_WIDTH", "4") != "2"
                     and (not self.gpu_bvh or self.gpu_bvh4))
        # BVH4 node steps read 64-B binary16 nodes (rt_node4h_t) when the scene has them
        self.bvh4_f16 = self.bvh4 and (self.gpu_bvh or bool(self.scene.info()["bvh4_f16"]))

    def set_light(self, light) -> None:
        """Move the point light (clip x, y, w) of the current configuration,
        queued behind the frames already started (rt_renderer_set_light: no
        host wait).  When the configuration uses light-space shadow lists
        they are rebuilt on the device -- at once, or (the default policy,
        set_list_policy) once the light has stayed for a few frames, the
        frames before tracing their shadow rays by the BVH packet walk."""
        arr = (C.c_float * 3)(*[float(np.float32(x)) for x in light])
        _check(lib().rt_renderer_set_light(self._h, arr), "rt_renderer_set_light")
        self.params.light[:] = [float(np.float32(x)) for x in light]

    # several lights (vx_rt.h rt_renderer_set_lights; images rt_lights / rt_lights_stats)
    def set_lights(self, lights) -> None:
        """Light the configured primary + shadow frame by 1..16 point lights
        (clip x, y, w each): the frames after it are, per pixel and channel,
        the rounded mean of the single-light frames, traced in one launch --
        primary visibility and shading once, every shadow ray against each
        light on that light's own shadow lists.  Builds the lists at once and
        waits for the device.  set_light() and configure() return to one light."""
        arr = np.ascontiguousarray(np.asarray(lights, np.float32).reshape(-1, 3))
        _check(lib().rt_renderer_set_lights(self._h, arr.ctypes.data, arr.shape[0]), "rt_renderer_set_lights")
        self.params.light[:] = [float(x) for x in arr[0]]

    # several lights on a path frame (vx_rt.h rt_renderer_set_path_lights; images pt_lights / pt_lights_accum)
    def set_path_lights(self, lights) -> None:
        """Light the configured path-traced frame by 1..8 point lights (clip x,
        y, w each): render() / start() frames and accumulate() samples after it
        are, per pixel and channel, the rounded mean of the single-light path
        frames of the same seed, traced in one launch -- every bounce ray once,
        one shadow ray per light at each vertex.  Builds a set of shadow lists
        per light and waits for the device; starts accumulated records over.
        set_light() and configure() return to one light."""
        arr = np.ascontiguousarray(np.asarray(lights, np.float32).reshape(-1, 3))
        _check(lib().rt_renderer_set_path_lights(self._h, arr.ctypes.data, arr.shape[0]),
               "rt_renderer_set_path_lights")
        self.params.light[:] = [float(x) for x in arr[0]]

    def lights_info(self) -> list:
        """The lights in use: per light {light, slist_on, slist_entries}."""
        out = (LightInfo * RT_MAX_LIGHTS)()
        n = C.c_uint32()
        _check(lib().rt_renderer_lights_info(self._h, out, RT_MAX_LIGHTS, C.byref(n)), "rt_renderer_lights_info")
        return [{"light": tuple(out[i].light), "slist_on": out[i].slist_on,
                 "slist_entries": out[i].slist_entries} for i in range(n.value)]

    def light_records(self, i: int, name: str) -> np.ndarray:
        """Light i's shadow-list array ("sidx" or "slist"), as records() gives
        the single light's."""
        which, dt, words = RECORDS[name]
        n = C.c_uint64()
        _check(lib().rt_renderer_export_light_lists(self._h, int(i), which, None, 0, C.byref(n)),
               f"rt_renderer_export_light_lists({i}, {name})")
        out = np.zeros(max(n.value // 4, 1), dt)
        _check(lib().rt_renderer_export_light_lists(self._h, int(i), which, out.ctypes.data, out.nbytes,
                                                    C.byref(n)), f"rt_renderer_export_light_lists({i}, {name})")
        return out[:n.value // 4].reshape(-1, words)

    def set_list_policy(self, defer_frames: int) -> None:
        """0: set_light queues the new light's shadow lists at once; n > 0:
        before the (n + 1)-th frame with that light (rt_renderer_set_list_policy)."""
        _check(lib().rt_renderer_set_list_policy(self._h, int(defer_frames)),
               "rt_renderer_set_list_policy")

    def setup_stats(self) -> dict:
        """How the last configure built its records (device / host, launches,
        heavy tiles, setup and configure wall ms)."""
        st = SetupStats()
        _check(lib().rt_renderer_setup_stats(self._h, C.byref(st)), "rt_renderer_setup_stats")
        return st.as_dict()

    def records(self, name: str) -> np.ndarray:
        """One per-resolution record array of the current configuration
        (RECORDS: prims, bbox, vis, vnodes, vtris, vlayers, vgeom, order,
        ptris, geom, bidx, blist -- the per-block candidate lists, blist with
        its 3 padding entries; btidx, btrim -- the same lists trimmed to their
        winners, which the frames scan, and btidx_host, btrim_host, their host
        restatement; oidx, olist -- the ordered tail's per-block
        lists, olist with its 2 padding entries), as [count, words]."""
        which, dt, words = RECORDS[name]
        n = C.c_uint64()
        _check(lib().rt_renderer_export_records(self._h, which, None, 0, C.byref(n)),
               f"rt_renderer_export_records({name})")
        out = np.zeros(max(n.value // 4, 1), dt)
        _check(lib().rt_renderer_export_records(self._h, which, out.ctypes.data, out.nbytes, C.byref(n)),
               f"rt_renderer_export_records({name})")
        return out[:n.value // 4].reshape(-1, words)

    def bvh_stats(self) -> dict:
        """How the current tree was built (method: 0 LBVH, 1 SAH on the
        device, 2 the host build; nodes, depth, stack4, build_ms, ...)."""
        st = BvhBuildStats()
        _check(lib().rt_renderer_bvh_stats(self._h, C.byref(st)), "rt_renderer_bvh_stats")
        return st.as_dict()

    def build_bvh(self, method: str = "lbvh") -> dict:
        """Build the BVH on the device and trace over it from now on; returns
        the build statistics.  method "lbvh": Morton codes + radix tree
        (kernels/bvh_build.hip); "sah": the host builder's binned-SAH tree
        restated on the device (kernels/bvh_sah.hip), equal to the scene's
        host-built arrays."""
        st = BvhBuildStats()
        m = {"lbvh": 0, "sah": 1}[method]
        _check(lib().rt_renderer_build_bvh_ex(self._h, m, C.byref(st)), "rt_renderer_build_bvh_ex")
        self.gpu_bvh = True
        self.gpu_bvh4 = st.stack4 != RT_BVH_STACK4_UNUSED
        if self.params is not None:
            self.bvh4 = self.gpu_bvh4 and not self.params.flags & RT_RENDER_BVH2
            self.bvh4_f16 = self.bvh4  # the device tree carries binary16 records (BVHB_HALF)
        return st.as_dict()

    def export_bvh4(self):
        """The renderer's current BVH4 nodes (float32[N4, 32], rt_node4_t)."""
        n = C.c_uint32()
        _check(lib().rt_renderer_export_bvh4(self._h, None, C.byref(n)), "rt_renderer_export_bvh4")
        nodes4 = np.zeros((max(n.value, 1), 32), np.float32)
        _check(lib().rt_renderer_export_bvh4(self._h, nodes4.ctypes.data, C.byref(n)),
               "rt_renderer_export_bvh4")
        return nodes4[:n.value]

    def export_bvh4h(self):
        """The same nodes as rt_node4h_t records (uint8[N4, 64]: 24 binary16
        planes, 4 child refs) -- what the kernels read."""
        n = C.c_uint32()
        _check(lib().rt_renderer_export_bvh4h(self._h, None, C.byref(n)), "rt_renderer_export_bvh4h")
        out = np.zeros((max(n.value, 1), 64), np.uint8)
        _check(lib().rt_renderer_export_bvh4h(self._h, out.ctypes.data, C.byref(n)),
               "rt_renderer_export_bvh4h")
        return out[:n.value]

    def export_vis_tree(self):
        """The primary rays' tree of the current configuration: (refs
        int32[N, 4] child references, leaf_pids int32[M])."""
        nn, nl = C.c_uint32(), C.c_uint32()
        _check(lib().rt_renderer_export_vis_tree(self._h, None, C.byref(nn), None, C.byref(nl)),
               "rt_renderer_export_vis_tree")
        refs = np.zeros((max(nn.value, 1), 4), np.int32)
        pids = np.zeros(max(nl.value, 1), np.int32)
        _check(lib().rt_renderer_export_vis_tree(self._h, refs.ctypes.data, C.byref(nn),
                                                 pids.ctypes.data, C.byref(nl)),
               "rt_renderer_export_vis_tree")
        return refs[:nn.value], pids[:nl.value]

    def export_bvh(self):
        """The renderer's current BVH: (nodes float32[N, 16], tris float32[M, 12])."""
        nn, nt = C.c_uint32(), C.c_uint32()
        _check(lib().rt_renderer_export_bvh(self._h, None, None, C.byref(nn), C.byref(nt)),
               "rt_renderer_export_bvh")
        nodes = np.zeros((max(nn.value, 1), 16), np.float32)
        tris = np.zeros((max(nt.value, 1), 12), np.float32)
        _check(lib().rt_renderer_export_bvh(self._h, nodes.ctypes.data, tris.ctypes.data,
                                            C.byref(nn), C.byref(nt)), "rt_renderer_export_bvh")
        return nodes[:nn.value], tris[:nt.value]

    def render(self) -> None:
        _check(lib().rt_render(self._h), "rt_render")

    def start(self) -> None:
        _check(lib().rt_render_start(self._h), "rt_render_start")

    def wait(self) -> None:
        _check(lib().rt_render_wait(self._h), "rt_render_wait")

    # progressive path tracing (vx_rt.h rt_renderer_accum_begin; image pt_accum)
    def accum_begin(self) -> None:
        """Start accumulating samples per pixel on the configured path frame:
        one uint32 {sumR, sumG, sumB, n} record per framebuffer pixel on the
        device; the next accumulate() starts from zero.  configure() ends it."""
        _check(lib().rt_renderer_accum_begin(self._h), "rt_renderer_accum_begin")

    def accum_reset(self) -> None:
        """The next accumulate() starts the records over (a flag of that
        launch: nothing is queued).  set_light() does the same."""
        _check(lib().rt_renderer_accum_reset(self._h), "rt_renderer_accum_reset")

    def accumulate(self, samples: int, wait: bool = True) -> None:
        """One launch tracing `samples` (1..32) more samples of every pixel --
        sample i is the path frame of seed + i -- into the records; the
        framebuffer gets the rounded mean of all samples so far.
        wait=False: queued only (wait() later)."""
        if wait:
            _check(lib().rt_render_accumulate(self._h, int(samples)), "rt_render_accumulate")
        else:
            _check(lib().rt_render_accumulate_start(self._h, int(samples)), "rt_render_accumulate_start")

    def accum_samples(self) -> int:
        """Samples per pixel queued since the last reset."""
        n = C.c_uint32()
        _check(lib().rt_renderer_accum_samples(self._h, C.byref(n)), "rt_renderer_accum_samples")
        return n.value

    def accum(self) -> np.ndarray:
        """The records: uint32 [H, W, 4] = sumR, sumG, sumB, n (compact /
        sharded frames: the flat [local_tiles * 1024, 4] array in the compact
        framebuffer's order)."""
        p = self.params
        if p.shard_count > 1 or p.flags & RT_RENDER_COMPACT:
            n = self.stats()["local_tiles"] * TILE * TILE
            out = np.zeros((max(n, 1), 4), np.uint32)
            _check(lib().rt_read_accum(self._h, out.ctypes.data, n), "rt_read_accum")
            return out[:n]
        out = np.zeros((p.height, p.width, 4), np.uint32)
        _check(lib().rt_read_accum(self._h, out.ctypes.data, p.height * p.width), "rt_read_accum")
        return out

    # per-pixel visibility records (vx_rt.h rt_render_aov_start; image rt_aov)
    def aov(self, wait: bool = True):
        """One launch writing a visibility record per framebuffer pixel of the
        configured primary+shadow frame -- the shaded primitive, the winner's
        depth word and flags, the plane t, and per light in use whether it does
        NOT see the pixel -- with no shading and no texel reads; the framebuffer
        keeps the last frame.  Returns the records as a structured array
        (AOV_DTYPE) [H, W], or [local_tiles * 1024] in the compact framebuffer's
        order for compact / sharded frames.  wait=False: queued only, returns
        None (wait(), then aov_records())."""
        if not wait:
            _check(lib().rt_render_aov_start(self._h), "rt_render_aov_start")
            return None
        _check(lib().rt_render_aov(self._h), "rt_render_aov")
        return self.aov_records()

    def aov_records(self) -> np.ndarray:
        """The records of the last aov() launch (waits for the device)."""
        p = self.params
        if p is None:
            raise RtError("rt_read_aov failed: renderer not configured")
        if p.shard_count > 1 or p.flags & RT_RENDER_COMPACT:
            n = self.stats()["local_tiles"] * TILE * TILE
            out = np.zeros(max(n, 1), AOV_DTYPE)
            _check(lib().rt_read_aov(self._h, out.ctypes.data, n), "rt_read_aov")
            return out[:n]
        out = np.zeros((p.height, p.width), AOV_DTYPE)
        _check(lib().rt_read_aov(self._h, out.ctypes.data, out.size), "rt_read_aov")
        return out

    # relighting from the records (vx_rt.h rt_relight_capture_start; images rt_aov_base, rt_relight)
    def relight_capture(self, wait: bool = True) -> None:
        """One launch writing the visibility records of aov() -- the same records,
        aov_records() returns them -- and every pixel's base colour, the pixel
        shaded without shadows (relight_base()), under the lights in use.  What
        relight() needs; set_light(), set_lights(), set_path_lights() and
        configure() end it."""
        if wait:
            _check(lib().rt_relight_capture(self._h), "rt_relight_capture")
        else:
            _check(lib().rt_relight_capture_start(self._h), "rt_relight_capture_start")

    def relight(self, weights, wait: bool = True) -> None:
        """One streaming launch writing into the framebuffer the captured frame
        under per-light weights 0..255, one per light in use at capture time: per
        pixel and channel the weighted rounded mean of the single-light frames
        (weights 0 / 1: the set_lights frame of the lights with a 1).  No tracing,
        no host wait, no copy; launches queue back to back (wait=False)."""
        w = np.asarray(weights)
        if w.ndim != 1 or w.size == 0 or (w < 0).any() or (w > 255).any():
            raise RtError("rt_render_relight failed: weights are 0..255, one per light")
        w = np.ascontiguousarray(w, np.uint8)
        fn = lib().rt_render_relight if wait else lib().rt_render_relight_start
        _check(fn(self._h, w.ctypes.data, w.size), "rt_render_relight" if wait else "rt_render_relight_start")

    def relight_base(self) -> np.ndarray:
        """The base colours of the last relight_capture() (waits for the device):
        uint32 ARGB [H, W], or [local_tiles * 1024] in the compact framebuffer's
        order for compact / sharded frames."""
        p = self.params
        if p is None:
            raise RtError("rt_read_relight_base failed: renderer not configured")
        if p.shard_count > 1 or p.flags & RT_RENDER_COMPACT:
            n = self.stats()["local_tiles"] * TILE * TILE
            out = np.zeros(max(n, 1), np.uint32)
            _check(lib().rt_read_relight_base(self._h, out.ctypes.data, n), "rt_read_relight_base")
            return out[:n]
        out = np.zeros((p.height, p.width), np.uint32)
        _check(lib().rt_read_relight_base(self._h, out.ctypes.data, out.size), "rt_read_relight_base")
        return out

    # ambient occlusion from the records (vx_rt.h rt_renderer_ao_begin; images rt_ao, rt_ao_resolve)
    def ao_begin(self, radius: float = float("inf"), seed: int = AO_SEED) -> None:
        """Begin an ambient-occlusion session on the visibility records of the last
        aov() / relight_capture(): rays of at most `radius` (positive, or inf),
        sample c keyed by seed + c.  Linear framebuffers only.  set_light() and
        set_lights() do not end it; configure() does."""
        p = AoParams(float(radius), int(seed) & 0xFFFFFFFF)
        _check(lib().rt_renderer_ao_begin(self._h, C.byref(p)), "rt_renderer_ao_begin")

    def ao_reset(self) -> None:
        """The sample cursor back to 0; the next ao() launch overwrites the counts."""
        _check(lib().rt_renderer_ao_reset(self._h), "rt_renderer_ao_reset")

    def ao(self, samples: int, wait: bool = True) -> None:
        """One launch tracing `samples` (1..64) more any-hit rays per ray pixel --
        cosine-weighted about the pixel's geometric normal, the path tracer's first
        bounce -- and adding the occluded ones to the pixel's count (ao_records()).
        It writes neither the framebuffer nor the visibility records."""
        fn = lib().rt_render_ao if wait else lib().rt_render_ao_start
        _check(fn(self._h, int(samples)), "rt_render_ao" if wait else "rt_render_ao_start")

    def ao_samples(self) -> int:
        """N: the samples traced per ray pixel since ao_begin() / ao_reset()."""
        n = C.c_uint32()
        _check(lib().rt_renderer_ao_samples(self._h, C.byref(n)), "rt_renderer_ao_samples")
        return int(n.value)

    def ao_records(self) -> np.ndarray:
        """The occluded samples per pixel, uint32 [H, W] (waits for the device)."""
        p = self.params
        if p is None:
            raise RtError("rt_read_ao failed: renderer not configured")
        out = np.zeros((p.height, p.width), np.uint32)
        _check(lib().rt_read_ao(self._h, out.ctypes.data, out.size), "rt_read_ao")
        return out

    def ao_resolve(self, mode: str = "grey", weights=None, wait: bool = True) -> None:
        """One streaming launch writing the ambient term into the framebuffer in
        use: mode "grey" the term on white, rt.ao_resolve(0xffffffff, o, N);
        "modulate" the term on the relit pixel of the live relight_capture() under
        `weights` (as relight() takes them), or on the base colour itself with
        weights=None."""
        if mode not in AO_MODES:
            raise RtError(f"rt_render_ao_resolve failed: mode is one of {sorted(AO_MODES)}")
        wp, n = None, 0
        if weights is not None:
            w = np.asarray(weights)
            if w.ndim != 1 or w.size == 0 or (w < 0).any() or (w > 255).any():
                raise RtError("rt_render_ao_resolve failed: weights are 0..255, one per light")
            w = np.ascontiguousarray(w, np.uint8)
            wp, n = w.ctypes.data, w.size
        fn = lib().rt_render_ao_resolve if wait else lib().rt_render_ao_resolve_start
        _check(fn(self._h, AO_MODES[mode], wp, n), "rt_render_ao_resolve" if wait else "rt_render_ao_resolve_start")

    # caller-supplied rays (vx_rt.h rt_query_reserve; images rt_query, rt_query_keys)
    def query_reserve(self, n: int) -> None:
        """Reserve the device buffers for up to n rays per trace_rays() / query_keys()
        call (52 B per ray).  The renderer must be configured; the reserve survives
        configure(), set_light() and set_lights()."""
        _check(lib().rt_query_reserve(self._h, int(n)), "rt_query_reserve")

    def query_buffers(self) -> dict:
        """The reserve's device pointers (rays, hits, skip, perm, keys), its capacity
        in rays and the key grid's box float32[6] (lo.xyz, hi.xyz)."""
        b = QueryBuffers()
        _check(lib().rt_query_buffers(self._h, C.byref(b)), "rt_query_buffers")
        out = {k: getattr(b, k) for k in ("rays", "hits", "skip", "perm", "keys")}
        out["capacity"] = int(b.capacity)
        out["box"] = np.array(list(b.box), np.float32)
        return out

    def _query_upload(self, what: str, rays, skip):
        """rays (and skip) into the reserve, rays converted to rt_ray_t -> (n, on_device)"""
        n, dev = _query_check(what, rays, skip)
        if dev:
            import torch
            ext = torch.cuda.ExternalStream(self.device_stream())
            buf = self.query_buffers()
            if n > buf["capacity"]:
                raise RtError(f"{what} failed: {n} rays is above the reserve's capacity of {buf['capacity']}")
            ext.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(ext):
                conv = rays[:, list(_RAY_COLUMNS)].contiguous()
                keep = [conv]
                _hip_copy(buf["rays"], conv.data_ptr(), 32 * n, ext.cuda_stream)
                if skip is not None:
                    sk = skip.contiguous()
                    keep.append(sk)
                    _hip_copy(buf["skip"], sk.data_ptr(), 4 * n, ext.cuda_stream)
            self._query_keep = keep   # (alive until the next call: the copies are queued, not done)
            return n, True
        conv = np.ascontiguousarray(rays[:, list(_RAY_COLUMNS)])
        _check(lib().rt_query_write_rays(self._h, conv.ctypes.data, 0, n), "rt_query_write_rays")
        if skip is not None:
            sk = np.ascontiguousarray(skip)
            _check(lib().rt_query_write_skip(self._h, sk.ctypes.data, 0, n), "rt_query_write_skip")
        return n, False

    def _query_keys_device(self, n: int):
        """the keys of rays [0, n) as an int64 tensor (0 .. 2^32 - 1), on the renderer's stream"""
        import torch
        ext = torch.cuda.ExternalStream(self.device_stream())
        buf = self.query_buffers()
        with torch.cuda.stream(ext):
            raw = torch.empty(n, dtype=torch.int32, device="cuda")
            _hip_copy(raw.data_ptr(), buf["keys"], 4 * n, ext.cuda_stream)
            keys = raw.to(torch.int64) & 0xFFFFFFFF
        return keys, ext

    def query_keys(self, rays, wait: bool = True):
        """The coherence keys (vx_rt.h rt_query_key) of rays float32 [n, 8] in the
        oracle's column order (o, d, tmin, tmax), computed on the device: uint32 [n]
        for an array, an int64 tensor for a CUDA tensor."""
        n, dev = self._query_upload("rt_query_keys", rays, None)
        _check(lib().rt_query_keys_start(self._h, n), "rt_query_keys_start")
        if dev:
            import torch
            keys, ext = self._query_keys_device(n)
            torch.cuda.current_stream().wait_stream(ext)
            if wait:
                ext.synchronize()
                _check(lib().rt_render_wait(self._h), "rt_render_wait")
            return keys
        out = np.zeros(n, np.uint32)
        _check(lib().rt_query_read_keys(self._h, out.ctypes.data, 0, n), "rt_query_read_keys")
        return out

    def trace_rays(self, rays, mode: str = "closest", skip=None, sort: bool = False, wait: bool = True):
        """Trace rays float32 [n, 8] in the oracle's column order (o, d, tmin, tmax;
        clip (x, y, w) space, the space of Scene.prims()[:, :, (0, 1, 3)]) against
        the scene's geometry: mode "closest" the nearest hit (lowest pid on ties),
        "any" some occluder (rely on pid >= 0 only).  skip: int32 [n], the primitive
        a ray does not meet, -1 for none.  sort=True traces the rays in the order of
        their coherence keys (one more launch and a sort; the hits stay at the rays'
        own indices).  -> (pid int32 [n], t float32 [n]); a miss is (-1, 0.0).  A
        CUDA torch tensor is taken as it is on the renderer's stream and the hits
        come back as tensors.  wait=False returns None once the launch is queued:
        query_hits(n) reads the hits later."""
        if mode not in QUERY_MODES:
            raise RtError(f"rt_query_trace failed: mode is one of {sorted(QUERY_MODES)}")
        n, dev = self._query_upload("rt_query_trace", rays, skip)
        flags = RT_QUERY_SKIP if skip is not None else 0
        if sort:
            _check(lib().rt_query_keys_start(self._h, n), "rt_query_keys_start")
            flags |= RT_QUERY_PERM
            if dev:
                import torch
                keys, ext = self._query_keys_device(n)
                with torch.cuda.stream(ext):
                    perm = torch.sort(keys, stable=True).indices.to(torch.int32)
                    _hip_copy(self.query_buffers()["perm"], perm.data_ptr(), 4 * n, ext.cuda_stream)
                self._query_keep.append(perm)
            else:
                keys = np.zeros(n, np.uint32)
                _check(lib().rt_query_read_keys(self._h, keys.ctypes.data, 0, n), "rt_query_read_keys")
                perm = np.ascontiguousarray(np.argsort(keys, kind="stable"), np.uint32)
                _check(lib().rt_query_write_perm(self._h, perm.ctypes.data, 0, n), "rt_query_write_perm")
        _check(lib().rt_query_trace_start(self._h, n, QUERY_MODES[mode], flags), "rt_query_trace_start")
        if dev:
            import torch
            ext = torch.cuda.ExternalStream(self.device_stream())
            with torch.cuda.stream(ext):
                hits = torch.empty((n, 2), dtype=torch.int32, device="cuda")
                _hip_copy(hits.data_ptr(), self.query_buffers()["hits"], 8 * n, ext.cuda_stream)
            torch.cuda.current_stream().wait_stream(ext)
            if wait:
                ext.synchronize()
                _check(lib().rt_render_wait(self._h), "rt_render_wait")
            return hits[:, 0], hits[:, 1].view(torch.float32)
        return self.query_hits(n) if wait else None

    def query_hits(self, n: int):
        """The hits of rays [0, n) of the last trace_rays(): (pid int32 [n], t
        float32 [n]) (waits for the device)."""
        out = np.zeros(int(n), HIT_DTYPE)
        _check(lib().rt_query_read_hits(self._h, out.ctypes.data, 0, int(n)), "rt_query_read_hits")
        return out["pid"].copy(), out["t"].copy()

    # soft shadows from the records (vx_rt.h rt_renderer_soft_begin; images rt_soft, rt_soft_resolve)
    def soft_begin(self, radii, seed: int = RT_SOFT_DEFAULT_SEED) -> None:
        """Begin a soft-shadow session on the visibility records of the last aov() /
        relight_capture(): one radius (finite, >= 0) per light in use, sample c keyed
        by seed + c.  Linear framebuffers only.  configure(), set_light(),
        set_lights() and set_path_lights() end it; a refused begin leaves a session
        already begun as it was."""
        rad = np.ascontiguousarray(np.atleast_1d(np.asarray(radii, np.float32)))
        if rad.ndim != 1 or rad.size == 0:
            raise RtError("rt_renderer_soft_begin failed: radii is one float per light")
        p = SoftParams(rad.ctypes.data_as(C.POINTER(C.c_float)), rad.size, int(seed) & 0xFFFFFFFF)
        _check(lib().rt_renderer_soft_begin(self._h, C.byref(p)), "rt_renderer_soft_begin")
        self._soft_n = int(rad.size)

    def soft_reset(self) -> None:
        """The sample cursor back to 0; the next soft() launch overwrites the counts."""
        _check(lib().rt_renderer_soft_reset(self._h), "rt_renderer_soft_reset")

    def soft(self, samples: int, wait: bool = True) -> None:
        """One launch tracing `samples` (1..64) more segments per ray pixel and light
        -- to cosine-weighted points of the light's sphere that face the pixel --
        and adding the occluded ones to the (light, pixel) count (soft_records()).
        It writes neither the framebuffer nor the visibility records."""
        fn = lib().rt_render_soft if wait else lib().rt_render_soft_start
        _check(fn(self._h, int(samples)), "rt_render_soft" if wait else "rt_render_soft_start")

    def soft_samples(self) -> int:
        """N: the samples traced per ray pixel and light since soft_begin() / soft_reset()."""
        n = C.c_uint32()
        _check(lib().rt_renderer_soft_samples(self._h, C.byref(n)), "rt_renderer_soft_samples")
        return int(n.value)

    def soft_records(self) -> np.ndarray:
        """The occluded samples per light and pixel, uint16 [n, H, W] (waits for the device)."""
        p = self.params
        if p is None:
            raise RtError("rt_read_soft failed: renderer not configured")
        out = np.zeros((max(getattr(self, "_soft_n", 1), 1), p.height, p.width), np.uint16)
        _check(lib().rt_read_soft(self._h, out.ctypes.data, out.size), "rt_read_soft")
        return out

    def soft_resolve(self, mode: str = "lit", weights=None, wait: bool = True) -> None:
        """One streaming launch writing the soft-shadow term into the framebuffer in
        use: mode "lit" rt.soft_resolve over the base colours of the live
        relight_capture() under `weights` (one 0..255 per light; None: unit weights);
        "grey" the term on white under unit weights."""
        if mode not in SOFT_MODES:
            raise RtError(f"rt_render_soft_resolve failed: mode is one of {sorted(SOFT_MODES)}")
        wp, n = None, 0
        if weights is not None:
            w = np.asarray(weights)
            if w.ndim != 1 or w.size == 0 or (w < 0).any() or (w > 255).any():
                raise RtError("rt_render_soft_resolve failed: weights are 0..255, one per light")
            w = np.ascontiguousarray(w, np.uint8)
            wp, n = w.ctypes.data, w.size
        fn = lib().rt_render_soft_resolve if wait else lib().rt_render_soft_resolve_start
        _check(fn(self._h, SOFT_MODES[mode], wp, n),
               "rt_render_soft_resolve" if wait else "rt_render_soft_resolve_start")

    # denoising accumulated path frames (vx_rt.h rt_denoise_capture_start; images rt_aov_guide,
    # rt_denoise_prep, rt_denoise_pass)
    def denoise_capture(self, wait: bool = True) -> None:
        """One launch writing the filter's guide -- per pixel the shaded
        primitive, the depth word and geometry flag, the geometric normal -- and
        the base colour (the pixel shaded without shadows) of the configured path
        frame (linear framebuffer).  It depends on view and size only: lights,
        resets and further samples leave it valid; configure() releases it."""
        if wait:
            _check(lib().rt_denoise_capture(self._h), "rt_denoise_capture")
        else:
            _check(lib().rt_denoise_capture_start(self._h), "rt_denoise_capture_start")

    def denoise(self, passes: int = DENOISE_PASSES, depth_shift: int = DENOISE_DEPTH_SHIFT,
                color_shift: int = DENOISE_COLOR_SHIFT, wait: bool = True) -> None:
        """The edge-avoiding a-trous filter over the accumulated samples into
        the framebuffer in use: 1 + passes launches, no tracing, no host wait, no
        copy; the records are only read, accumulate() goes on afterwards.
        passes 1..5 (strides 1, 2, 4, 8, 16), depth_shift 0..23, color_shift
        0..16 (16: the irradiance stop is off).  wait=False: queued only."""
        vals = (passes, depth_shift, color_shift)
        if any(int(v) != v or v < 0 or v > 0xFFFFFFFF for v in vals):
            raise RtError("rt_render_denoise failed: passes, depth_shift and color_shift are small integers")
        prm = (C.c_uint32 * 3)(*[int(v) for v in vals])
        fn = lib().rt_render_denoise if wait else lib().rt_render_denoise_start
        _check(fn(self._h, C.addressof(prm)), "rt_render_denoise" if wait else "rt_render_denoise_start")

    def denoise_guide(self):
        """(guide, base) of the last denoise_capture() (waits for the device):
        the guide records as a structured array (DENOISE_GUIDE_DTYPE) [H, W] and
        the base colours uint32 ARGB [H, W]."""
        p = self.params
        if p is None:
            raise RtError("rt_read_denoise_guide failed: renderer not configured")
        guide = np.zeros((p.height, p.width), DENOISE_GUIDE_DTYPE)
        base = np.zeros((p.height, p.width), np.uint32)
        _check(lib().rt_read_denoise_guide(self._h, guide.ctypes.data, base.ctypes.data, base.size),
               "rt_read_denoise_guide")
        return guide, base

    def write_accum(self, rec) -> None:
        """Restore the accumulation records (checkpoint and resume): uint32
        [H, W, 4] (or the flat compact array) as accum() returns them, every
        record with the same n in 1..2^24, which becomes the sample cursor -- the
        next accumulate() continues from it.  Waits for the device."""
        a = np.ascontiguousarray(rec, np.uint32)
        if a.ndim < 2 or a.shape[-1] != 4 or a.size == 0:
            raise RtError("rt_write_accum failed: records are uint32 [..., 4]")
        n = int(a.reshape(-1, 4)[0, 3])
        _check(lib().rt_write_accum(self._h, a.ctypes.data, a.size // 4, n), "rt_write_accum")

    def stats(self) -> dict:
        s = Stats()
        _check(lib().rt_render_stats(self._h, C.byref(s)), "rt_render_stats")
        return s.as_dict()

    def kernel_ms(self) -> float:
        """HIP-event duration of the last launch (cheap: no counter read-back)."""
        ms = C.c_double()
        _check(lib().rt_render_kernel_ms(self._h, C.byref(ms)), "rt_render_kernel_ms")
        return ms.value

    def run_totals(self):
        """(summed kernel ms of the timed launches, timed launches, all
        launches) since the device opened; waits for every queued frame."""
        ms, nt, n = C.c_double(), C.c_uint64(), C.c_uint64()
        _check(lib().rt_render_run_totals(self._h, C.byref(ms), C.byref(nt), C.byref(n)),
               "rt_render_run_totals")
        return ms.value, nt.value, n.value

    def set_timing(self, timed: bool) -> None:
        """Events on the launches (True, the default) or none (False: no queue
        bound either, back-to-back frames for a host clock); waits for the
        in-flight frames."""
        _check(lib().rt_render_set_timing(self._h, 1 if timed else 0), "rt_render_set_timing")

    def framebuffer(self) -> np.ndarray:
        p = self.params
        if p.shard_count > 1 or p.flags & RT_RENDER_COMPACT:
            n = self.stats()["local_tiles"] * TILE * TILE
            out = np.zeros(max(n, 1), np.uint32)
            _check(lib().rt_read_framebuffer(self._h, out.ctypes.data, n), "rt_read_framebuffer")
            return out[:n]
        out = np.zeros((p.height, p.width), np.uint32)
        _check(lib().rt_read_framebuffer(self._h, out.ctypes.data, out.size), "rt_read_framebuffer")
        return out

    def framebuffer_prev(self) -> np.ndarray:
        """The frame started before the last one (overlapped configurations
        keep two framebuffers; an error when only one frame is kept)."""
        p = self.params
        out = np.zeros((p.height, p.width), np.uint32)
        _check(lib().rt_read_framebuffer_prev(self._h, out.ctypes.data, out.size),
               "rt_read_framebuffer_prev")
        return out

    def launch_rows(self) -> np.ndarray:
        """uint32 [grid, 16]: the last launch's per-workgroup counter rows."""
        n = C.c_uint64()
        _check(lib().rt_launch_rows(self._h, None, 0, C.byref(n)), "rt_launch_rows")
        out = np.zeros((max(n.value, 1), 16), np.uint32)
        _check(lib().rt_launch_rows(self._h, out.ctypes.data, n.value, C.byref(n)), "rt_launch_rows")
        return out[:n.value]

    def gather(self, comm) -> np.ndarray:
        """rt_render_gather over a shard.ShardComm: this rank's compact tiles
        to rank 0 (RCCL), assembled there; rank 0 gets the uint32 [H, W]
        frame, other ranks None."""
        p = self.params
        rank, _ = comm.info()
        out = np.zeros((p.height, p.width), np.uint32) if rank == 0 else None
        _check(lib().rt_render_gather(self._h, comm.handle, out.ctypes.data if out is not None else None),
               "rt_render_gather")
        return out

    def depthbuffer(self) -> np.ndarray:
        """RT_RENDER_RASTER: uint32 [H, W] depth/stencil words (stencil << 24 | depth)."""
        p = self.params
        out = np.zeros((p.height, p.width), np.uint32)
        _check(lib().rt_read_depthbuffer(self._h, out.ctypes.data, out.size), "rt_read_depthbuffer")
        return out

    def framebuffer_device(self):
        ptr, nbytes = C.c_void_p(), C.c_uint64()
        _check(lib().rt_framebuffer_device(self._h, C.byref(ptr), C.byref(nbytes)),
               "rt_framebuffer_device")
        return ptr.value, nbytes.value

    def device_stream(self) -> int:
        s = C.c_void_p()
        _check(lib().rt_device_stream(self._h, C.byref(s)), "rt_device_stream")
        return s.value

    def caps(self):
        c = (C.c_uint64 * 8)()
        _check(lib().rt_device_caps(self._h, c), "rt_device_caps")
        return list(c)

    def close(self) -> None:
        if self._h:
            lib().rt_renderer_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def accum_resolve(rec, alpha_argb: int) -> int:
    """rt_accum_resolve: the pixel an accumulation record {sumR, sumG, sumB, n}
    resolves to -- alpha_argb's alpha over the rounded means (2 * sum + n) // (2 * n)."""
    arr = (C.c_uint32 * 4)(*[int(v) for v in rec])
    return int(lib().rt_accum_resolve(arr, int(alpha_argb) & 0xFFFFFFFF))


def lights_resolve(argb: int, occluded: int, k: int) -> int:
    """rt_lights_resolve: the pixel of a shadow ray of primary colour argb that
    `occluded` of its k lights do not see -- per channel (2 * sum + k) // (2 * k),
    sum = (k - occluded) * c + occluded * (c >> 1); argb's alpha."""
    return int(lib().rt_lights_resolve(int(argb) & 0xFFFFFFFF, int(occluded), int(k)))


def aov_relight(plain_argb, light_mask, k: int):
    """rt_aov_relight: the k-light frame's pixel from the unshadowed frame's
    pixel and a visibility record's light_mask -- rt_lights_resolve(plain_argb,
    popcount(light_mask & (2^k - 1)), k); mask bits at or above k are ignored.
    Scalars give an int; arrays (broadcast against each other) a uint32 array,
    the library's function applied to every distinct (pixel, mask) pair."""
    fn = lib().rt_aov_relight
    if np.ndim(plain_argb) == 0 and np.ndim(light_mask) == 0:
        return int(fn(int(plain_argb) & 0xFFFFFFFF, int(light_mask) & 0xFFFFFFFF, int(k)))
    a, m = np.broadcast_arrays(np.asarray(plain_argb).astype(np.uint32), np.asarray(light_mask).astype(np.uint32))
    key = (a.astype(np.uint64) << np.uint64(32)) | m.astype(np.uint64)
    uniq, inv = np.unique(key.reshape(-1), return_inverse=True)
    vals = np.array([fn(int(u >> np.uint64(32)), int(u & np.uint64(0xFFFFFFFF)), int(k)) for u in uniq], np.uint32)
    return vals[inv.reshape(-1)].reshape(a.shape)


def relight_resolve(base_argb, depth_flags, light_mask, weights):
    """rt_relight_resolve: the relit pixel from its base colour and its visibility
    record's depth_flags and light_mask under per-light weights 0..255 (n =
    len(weights)): with RT_AOV_SHADOW_RAY set, per channel (2 * ((W - O) * c + O *
    (c >> 1)) + W) // (2 * W), W the weights' sum and O the sum over the lights
    whose mask bit is set, under the base colour's alpha; else the base colour.
    Scalars give an int; arrays (broadcast against each other) a uint32 array, the
    library's function applied to every distinct (pixel, flag, mask) triple."""
    fn = lib().rt_relight_resolve
    w = np.ascontiguousarray(np.asarray(weights, np.int64).reshape(-1).astype(np.uint8))
    wp, n = w.ctypes.data, int(w.size)
    if np.ndim(base_argb) == 0 and np.ndim(depth_flags) == 0 and np.ndim(light_mask) == 0:
        return int(fn(int(base_argb) & 0xFFFFFFFF, int(depth_flags) & 0xFFFFFFFF, int(light_mask) & 0xFFFFFFFF, wp, n))
    a, d, m = np.broadcast_arrays(np.asarray(base_argb).astype(np.uint32), np.asarray(depth_flags).astype(np.uint32),
                                  np.asarray(light_mask).astype(np.uint32))
    # (of depth_flags only the shadow-ray bit matters: a key of colour, that bit and the mask's low 16 bits)
    sray = (d & np.uint32(RT_AOV_SHADOW_RAY)) != 0
    key = (a.astype(np.uint64) << np.uint64(32)) | (sray.astype(np.uint64) << np.uint64(16)) | \
        (m & np.uint32(0xFFFF)).astype(np.uint64)
    uniq, inv = np.unique(key.reshape(-1), return_inverse=True)
    vals = np.array([fn(int(u >> np.uint64(32)), RT_AOV_SHADOW_RAY if (int(u) >> 16) & 1 else 0, int(u) & 0xFFFF, wp, n)
                     for u in uniq], np.uint32)
    return vals[inv.reshape(-1)].reshape(a.shape)


def ao_resolve(argb, occluded, n: int):
    """rt_ao_resolve: the ambient term on a pixel -- per colour channel c of argb
    (2 * c * (n - occluded) + n) // (2 * n) under argb's alpha byte; argb when n is
    0.  Scalars give an int; arrays (broadcast against each other) a uint32 array,
    the library's function applied to every distinct (pixel, count) pair."""
    fn = lib().rt_ao_resolve
    if np.ndim(argb) == 0 and np.ndim(occluded) == 0:
        return int(fn(int(argb) & 0xFFFFFFFF, int(occluded) & 0xFFFFFFFF, int(n)))
    a, o = np.broadcast_arrays(np.asarray(argb).astype(np.uint32), np.asarray(occluded).astype(np.uint32))
    key = (a.astype(np.uint64) << np.uint64(32)) | o.astype(np.uint64)
    uniq, inv = np.unique(key.reshape(-1), return_inverse=True)
    vals = np.array([fn(int(u >> np.uint64(32)), int(u & np.uint64(0xFFFFFFFF)), int(n)) for u in uniq], np.uint32)
    return vals[inv.reshape(-1)].reshape(a.shape)


# the oracle's ray row (o, d, tmin, tmax) -> rt_ray_t (o, tmin, d, tmax)
_RAY_COLUMNS = (0, 1, 2, 6, 3, 4, 5, 7)


def _is_tensor(a) -> bool:
    return hasattr(a, "is_cuda") and hasattr(a, "data_ptr")


def _query_check(what: str, rays, skip):
    """shapes and dtypes of a ray table and its skip words, before any device call
    -> (n, whether they are CUDA tensors)"""
    dev = _is_tensor(rays)
    if dev:
        import torch
        if not rays.is_cuda or rays.dtype != torch.float32:
            raise RtError(f"{what} failed: a ray tensor is float32 on a CUDA device")
    elif not isinstance(rays, np.ndarray) or rays.dtype != np.float32:
        raise RtError(f"{what} failed: rays are a float32 array (or CUDA tensor) [n, 8]")
    if rays.ndim != 2 or rays.shape[1] != 8 or rays.shape[0] == 0:
        raise RtError(f"{what} failed: rays are [n, 8] (o, d, tmin, tmax), n >= 1; got {tuple(rays.shape)}")
    n = int(rays.shape[0])
    if skip is not None:
        if _is_tensor(skip) != dev:
            raise RtError(f"{what} failed: skip is an array with array rays, a CUDA tensor with tensor rays")
        if dev:
            import torch
            ok = skip.is_cuda and skip.dtype == torch.int32
        else:
            ok = isinstance(skip, np.ndarray) and skip.dtype == np.int32
        if not ok or skip.ndim != 1 or skip.shape[0] != n:
            raise RtError(f"{what} failed: skip is int32 [n], one word per ray")
    return n, dev


_hip = None


def _hip_copy(dst: int, src: int, nbytes: int, stream: int) -> None:
    """hipMemcpyAsync device to device on `stream` (torch's HIP runtime, which the
    driver shares: _lib loads torch first)"""
    global _hip
    if _hip is None:
        h = C.CDLL("libamdhip64.so.7")
        h.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        h.hipMemcpyAsync.restype = C.c_int
        _hip = h
    rc = _hip.hipMemcpyAsync(dst, src, nbytes, 3, stream)  # hipMemcpyDeviceToDevice
    if rc != 0:
        raise RtError(f"hipMemcpyAsync failed ({rc})")


def query_key(ray, box):
    """rt_query_key: the coherence key of a ray float32 [8] in the oracle's column
    order (o, d, tmin, tmax) over box float32 [6] (lo.xyz, hi.xyz) -> int; rows
    [n, 8] -> uint32 [n]."""
    r = np.ascontiguousarray(np.asarray(ray, np.float32))
    b = (C.c_float * 6)(*[float(v) for v in np.asarray(box, np.float32).reshape(6)])
    if r.ndim == 1 and r.shape[0] != 8:
        raise RtError("rt_query_key failed: a ray is 8 floats (o, d, tmin, tmax)")
    if r.ndim not in (1, 2) or r.shape[-1] != 8:
        raise RtError("rt_query_key failed: rays are [n, 8] (o, d, tmin, tmax)")
    fn = lib().rt_query_key
    if r.ndim == 1:
        c = np.ascontiguousarray(r[list(_RAY_COLUMNS)])
        return int(fn(c.ctypes.data, b))
    c = np.ascontiguousarray(r[:, list(_RAY_COLUMNS)])
    base, out = c.ctypes.data, np.zeros(len(c), np.uint32)
    for i in range(len(c)):
        out[i] = fn(base + 32 * i, b)
    return out


def soft_resolve(base_argb, depth_flags, counts, n_samples: int, weights):
    """rt_soft_resolve: the soft-shadow pixel -- with D = n_samples * sum(weights) and
    O = sum(weights[i] * min(counts[i], n_samples)), per colour channel c of base_argb
    (2 * ((D - O) * c + O * (c >> 1)) + D) // (2 * D) under base_argb's alpha byte for
    a pixel with RT_AOV_GEOM, base_argb for any other.  counts is [n] or [n, ...]
    (a plane per light), weights one 0..255 per light.  Scalars give an int; arrays
    (broadcast against each other) a uint32 array, the library's function applied to
    every distinct (pixel, geometry bit, counts) row."""
    fn = lib().rt_soft_resolve
    w = np.ascontiguousarray(np.asarray(weights), np.uint8).reshape(-1)
    cnt = np.asarray(counts).astype(np.uint16)
    if cnt.shape[0] != w.size:
        raise RtError("rt_soft_resolve failed: one count plane per weight")
    N, n = int(n_samples), int(w.size)
    if np.ndim(base_argb) == 0 and np.ndim(depth_flags) == 0 and cnt.ndim == 1:
        c = np.ascontiguousarray(cnt)
        return int(fn(int(base_argb) & 0xFFFFFFFF, int(depth_flags) & 0xFFFFFFFF, c.ctypes.data, N, w.ctypes.data, n))
    a, f = np.broadcast_arrays(np.asarray(base_argb).astype(np.uint32), np.asarray(depth_flags).astype(np.uint32))
    planes = np.ascontiguousarray(np.broadcast_to(cnt.reshape((n,) + cnt.shape[1:]), (n,) + a.shape)).reshape(n, -1)
    rows = np.concatenate([a.reshape(1, -1).astype(np.uint64), (f.reshape(1, -1) & RT_AOV_GEOM).astype(np.uint64),
                           planes.astype(np.uint64)], 0).T
    uniq, inv = np.unique(rows, axis=0, return_inverse=True)
    vals = np.empty(len(uniq), np.uint32)
    for k, u in enumerate(uniq):
        c = np.ascontiguousarray(u[2:], np.uint16)
        vals[k] = fn(int(u[0]), int(u[1]), c.ctypes.data, N, w.ctypes.data, n)
    return vals[np.asarray(inv).reshape(-1)].reshape(a.shape)


def path_lights_resolve(sums, k: int, alpha_argb: int) -> int:
    """rt_path_lights_resolve: the pixel whose k single-light 8-bit values sum
    to sums = (R, G, B) -- per channel (2 * sum + k) // (2 * k) -- under
    alpha_argb's alpha byte."""
    arr = (C.c_uint32 * 3)(*[int(x) for x in sums])
    return int(lib().rt_path_lights_resolve(arr, int(k), int(alpha_argb) & 0xFFFFFFFF))


def deinterleave_tiles(shards, width: int, height: int) -> np.ndarray:
    """Assemble per-rank compact tile buffers (rank r holds tiles t with
    t % G == r, each 32x32 in 8x8-block/lane task order) into a W x H image."""
    from .shard import deinterleave_tiles as _d
    return _d(shards, width, height)
