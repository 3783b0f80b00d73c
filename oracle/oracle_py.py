"""ctypes binding of the CPU oracle (oracle/_build/liboracle.so).

TEST INFRASTRUCTURE: imported only by tests/, __graft_entry__.smoke() and bench.py's
cpu_baseline leg. The product package (stratum_amd) never imports this module.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from stratum_amd import wire

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "_build", "liboracle.so")
_lib = None


def build(force=False):
    # make decides: the Makefile lists every dependency (both sources and the three shared headers under include/)
    subprocess.check_call(["make", "-C", _HERE, "-s"] + (["-B"] if force else []))
    return _LIB_PATH


_NATIVE_PATH = os.path.join(_HERE, "_build", "liboracle_native.so")
_native = None


def build_native():
    """The -O3 -march=native build bench.py's cpu_baseline times. Compiled on the box it runs on; call
    this BEFORE the process initialises the GPU (it starts make / g++ as children)."""
    # always rebuilt (-B): a copy compiled for another machine's -march=native may have travelled with the tree
    subprocess.check_call(["make", "-C", _HERE, "-s", "-B", "native"])
    return _NATIVE_PATH


def lib_native():
    """The native build, already built by build_native(); never builds by itself."""
    global _native
    if _native is None:
        if not os.path.exists(_NATIVE_PATH):
            raise RuntimeError("liboracle_native.so is missing: call oracle_py.build_native() first")
        _native = _bind(C.CDLL(_NATIVE_PATH))
    return _native


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            build()
        _lib = _bind(C.CDLL(_LIB_PATH))
    return _lib


def _bind(L):
    if True:
        L.orc_scene_create.restype = C.c_void_p
        L.orc_scene_create.argtypes = [C.POINTER(wire.SceneDesc)]
        L.orc_scene_destroy.argtypes = [C.c_void_p]
        L.orc_render.restype = C.c_int
        L.orc_render.argtypes = [
            C.c_void_p,
            C.POINTER(wire.BDPTPushConstants),
            C.c_uint32,
            C.c_uint32,
            C.POINTER(wire.FrameDesc),
            C.c_uint32,
            C.c_uint32,
            C.POINTER(wire.Outputs),
            C.c_int,
            C.c_void_p,
        ]
        L.orc_render_window.restype = C.c_int
        L.orc_render_window.argtypes = L.orc_render.argtypes + [C.c_void_p]
        L.orc_trace_rays.restype = C.c_int
        L.orc_trace_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p]
        L.orc_pcg.restype = C.c_uint32
        L.orc_pcg.argtypes = [C.c_uint32]
        L.orc_xxhash32.restype = C.c_uint32
        L.orc_xxhash32.argtypes = [C.c_uint32]
    return L


class OracleScene:
    def __init__(self, scene, native=False):
        self.scene = scene  # keep the arrays alive
        self._L = lib_native() if native else lib()
        d = scene.desc()
        self.h = self._L.orc_scene_create(C.byref(d))
        if not self.h:
            raise RuntimeError("orc_scene_create failed")

    def close(self):
        if getattr(self, "h", None) and getattr(self, "_L", None) is not None:
            self._L.orc_scene_destroy(self.h)
        self.h = None

    def __del__(self):
        self.close()

    def render(self, frame, push_constants, sampling_flags=wire.DEFAULT_SAMPLING_FLAGS, seed_begin=0, seed_count=1, threads=0, aovs=True, window=None, debug_mode=0, debug_image=None):
        """window = (x0, y0, x1, y1): render only that rectangle of the frame (the same pixels the whole frame has there);
        the arrays returned are still W x H, zero outside the window."""
        W, H = frame.width, frame.height
        out = {
            "radiance": np.zeros((H, W, 4), np.float32),
            "ray_count": np.zeros(2, np.uint64),
            "stats": np.zeros(4, np.uint64),
        }
        o = wire.Outputs()
        o.device_ptrs = 0
        o.gRadiance = wire.ptr(out["radiance"])
        o.gRayCount = wire.ptr(out["ray_count"])
        if aovs:
            out["albedo"] = np.zeros((H, W, 4), np.float32)
            out["visibility"] = np.zeros((H, W), wire.VisibilityInfo)
            out["depth"] = np.zeros((H, W), wire.DepthInfo)
            out["prev_uv"] = np.zeros((H, W, 2), np.float32)
            o.gAlbedo = wire.ptr(out["albedo"])
            o.gVisibility = wire.ptr(out["visibility"])
            o.gDepth = wire.ptr(out["depth"])
            o.gPrevUVs = wire.ptr(out["prev_uv"])
        if debug_mode:  # BDPTDebugMode -> gDebugImage, in / out (a copy of what the caller passes, or zeros)
            out["debug"] = np.ascontiguousarray(debug_image, np.float32).copy() if debug_image is not None else np.zeros((H, W, 4), np.float32)
            o.debug_mode = debug_mode
            o.gDebugImage = wire.ptr(out["debug"])
        if self.scene.volumes:
            frame.view_medium_instances = self.scene.view_medium_instances(frame.view_transforms)
        fd = frame.desc()
        win = np.asarray(window, np.uint32) if window is not None else None
        rc = self._L.orc_render_window(
            self.h, C.byref(push_constants), sampling_flags, self.scene.scene_flags, C.byref(fd), seed_begin, seed_count, C.byref(o), threads, wire.ptr(out["stats"]),
            wire.ptr(win) if win is not None else None,
        )
        if rc != 0:
            raise RuntimeError("orc_render failed: %d" % rc)
        return out

    def trace(self, rays, any_hit=False, brute=False, threads=0, alpha_test=False, flip_uvs=False):
        rays = np.ascontiguousarray(rays, dtype=wire.Ray)
        hits = np.zeros(rays.shape[0], wire.Hit)
        counters = np.zeros(2, np.uint64)
        rc = self._L.orc_trace_rays(self.h, wire.ptr(rays), rays.shape[0], wire.ptr(hits), (1 if any_hit else 0) | (2 if brute else 0) | (4 if alpha_test else 0) | (8 if flip_uvs else 0), threads, wire.ptr(counters))
        if rc != 0:
            raise RuntimeError("orc_trace_rays failed: %d" % rc)
        return hits, counters

    def sample_light(self, push_constants, rnd4, ref_pos, sampling_flags=wire.DEFAULT_SAMPLING_FLAGS):
        """sample_point_on_light (light.hlsli:37-152) -> dict of arrays"""
        rnd4 = np.ascontiguousarray(rnd4, np.float32).reshape(-1, 4)
        ref_pos = np.ascontiguousarray(np.broadcast_to(np.asarray(ref_pos, np.float32), (rnd4.shape[0], 3)))
        out = np.zeros((rnd4.shape[0], 16), np.float32)
        self._L.orc_sample_light(C.c_void_p(self.h), C.byref(push_constants), C.c_uint32(sampling_flags), C.c_uint32(self.scene.scene_flags), wire.ptr(rnd4), wire.ptr(ref_pos), wire.ptr(out), C.c_uint32(rnd4.shape[0]))
        return {
            "radiance": out[:, 0:3],
            "pdf": out[:, 3],
            "to_light": out[:, 4:7],
            "dist": out[:, 7],
            "position": out[:, 8:11],
            "normal": out[:, 11:14],
            "pdf_area_measure": out[:, 14] != 0,
            "is_environment": out[:, 15] != 0,
        }

    def delta_track(self, medium_address, keys, origin, direction, t_max, beta=1.0, can_scatter=True, max_null_collisions=64):
        """Medium::delta_track (medium.hlsli:74-127), one call per row -> dict of arrays"""
        keys = np.ascontiguousarray(keys, np.uint32).reshape(-1, 4)
        n = keys.shape[0]
        q = np.zeros((n, 8), np.float32)
        q[:, 0:3], q[:, 3:6], q[:, 6], q[:, 7] = origin, direction, t_max, beta
        out = np.zeros((n, 16), np.float32)
        self._L.orc_delta_track(C.c_void_p(self.h), C.c_uint32(medium_address), wire.ptr(keys), wire.ptr(q), C.c_uint32(1 if can_scatter else 0), C.c_uint32(max_null_collisions), wire.ptr(out), C.c_uint32(n))
        return {"beta": out[:, 0:3], "dir_pdf": out[:, 3:6], "nee_pdf": out[:, 6:9], "position": out[:, 9:12], "scattered": out[:, 12] != 0, "draws": out[:, 13].astype(np.int64)}

    def sample_image(self, index, uv_size, ray_cones=True):
        q = np.ascontiguousarray(uv_size, np.float32).reshape(-1, 3)
        out = np.zeros((q.shape[0], 4), np.float32)
        self._L.orc_sample_image(C.c_void_p(self.h), C.c_uint32(index), wire.ptr(q), C.c_uint32(1 if ray_cones else 0), wire.ptr(out), C.c_uint32(q.shape[0]))
        return out

    def shading_data(self, inst_prim, bary):
        inst_prim = np.ascontiguousarray(inst_prim, np.uint32)
        bary = np.ascontiguousarray(bary, np.float32)
        out = np.zeros(inst_prim.shape[0], wire.ShadingData)
        self._L.orc_shading_data(C.c_void_p(self.h), wire.ptr(inst_prim), wire.ptr(bary), wire.ptr(out), C.c_uint32(inst_prim.shape[0]))
        return out


# ---- unit functions ----
def pcg4d(v):
    v = np.ascontiguousarray(v, np.uint32).reshape(-1, 4).copy()
    lib().orc_pcg4d(wire.ptr(v), C.c_uint32(v.shape[0]))
    return v


def rng_floats(x, y, seed, counter0, n):
    out = np.zeros(n, np.float32)
    lib().orc_rng_floats(C.c_uint32(x), C.c_uint32(y), C.c_uint32(seed), C.c_uint32(counter0), wire.ptr(out), C.c_uint32(n))
    return out


def _map(fn, inputs, out_shape, out_dtype):
    n = inputs[0].shape[0]
    out = np.zeros((n,) + out_shape, out_dtype)
    getattr(lib(), fn)(*[wire.ptr(a) for a in inputs], wire.ptr(out), C.c_uint32(n))
    return out


def pack_normal(v):
    return _map("orc_pack_normal", [np.ascontiguousarray(v, np.float32)], (), np.uint32)


def unpack_normal(p):
    return _map("orc_unpack_normal", [np.ascontiguousarray(p, np.uint32)], (3,), np.float32)


def ray_offset(pos, nrm):
    return _map("orc_ray_offset", [np.ascontiguousarray(pos, np.float32), np.ascontiguousarray(nrm, np.float32)], (3,), np.float32)


def f32tof16(v):
    return _map("orc_f32tof16", [np.ascontiguousarray(v, np.float32)], (), np.uint32)


def f16tof32(v):
    return _map("orc_f16tof32", [np.ascontiguousarray(v, np.uint32)], (), np.float32)


def sincos(x):
    x = np.ascontiguousarray(x, np.float32)
    s = np.zeros_like(x)
    c = np.zeros_like(x)
    lib().orc_sincos(wire.ptr(x), wire.ptr(s), wire.ptr(c), C.c_uint32(x.shape[0]))
    return s, c


def log(x):
    return _map("orc_log", [np.ascontiguousarray(x, np.float32)], (), np.float32)


def exp(x):
    return _map("orc_exp", [np.ascontiguousarray(x, np.float32)], (), np.float32)


def atan2(y, x):
    return _map("orc_atan2", [np.ascontiguousarray(y, np.float32), np.ascontiguousarray(x, np.float32)], (), np.float32)


def acos(x):
    return _map("orc_acos", [np.ascontiguousarray(x, np.float32)], (), np.float32)


def asin(x):
    return _map("orc_asin", [np.ascontiguousarray(x, np.float32)], (), np.float32)


def pow(a, b):
    return _map("orc_pow", [np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)], (), np.float32)


def disney_eval(material_record, dir_in, dir_out):
    rec = np.ascontiguousarray(material_record, wire.MaterialRecord).reshape(1)
    di, do = np.ascontiguousarray(dir_in, np.float32), np.ascontiguousarray(dir_out, np.float32)
    out = np.zeros((di.shape[0], 5), np.float32)
    lib().orc_disney_eval(wire.ptr(rec), wire.ptr(di), wire.ptr(do), wire.ptr(out), C.c_uint32(di.shape[0]))
    return out


def disney_eval_adjoint(material_record, dir_in, dir_out, adjoint):
    rec = np.ascontiguousarray(material_record, wire.MaterialRecord).reshape(1)
    di, do = np.ascontiguousarray(dir_in, np.float32), np.ascontiguousarray(dir_out, np.float32)
    out = np.zeros((di.shape[0], 5), np.float32)
    lib().orc_disney_eval_adjoint(wire.ptr(rec), wire.ptr(di), wire.ptr(do), wire.ptr(out), C.c_uint32(di.shape[0]), C.c_uint32(1 if adjoint else 0))
    return out


def shading_normal_correction(rows5, shadow_fix=False, adjoint=False):
    q = np.ascontiguousarray(rows5, np.float32).reshape(-1, 5)
    out = np.zeros(q.shape[0], np.float32)
    lib().orc_shading_normal_correction(wire.ptr(q), wire.ptr(out), C.c_uint32(q.shape[0]), C.c_uint32(1 if shadow_fix else 0), C.c_uint32(1 if adjoint else 0))
    return out


def connection_dvc(rows3, specular=False):
    q = np.ascontiguousarray(rows3, np.float32).reshape(-1, 3)
    out = np.zeros(q.shape[0], np.float32)
    lib().orc_connection_dvc(wire.ptr(q), wire.ptr(out), C.c_uint32(q.shape[0]), C.c_uint32(1 if specular else 0))
    return out


def mis(rows2):
    q = np.ascontiguousarray(rows2, np.float32).reshape(-1, 2)
    out = np.zeros(q.shape[0], np.float32)
    lib().orc_mis(wire.ptr(q), wire.ptr(out), C.c_uint32(q.shape[0]))
    return out


def disney_sample(material_record, dir_in, rnd):
    rec = np.ascontiguousarray(material_record, wire.MaterialRecord).reshape(1)
    di, r = np.ascontiguousarray(dir_in, np.float32), np.ascontiguousarray(rnd, np.float32)
    out = np.zeros((di.shape[0], 13), np.float32)
    lib().orc_disney_sample(wire.ptr(rec), wire.ptr(di), wire.ptr(r), wire.ptr(out), C.c_uint32(di.shape[0]))
    return out


# ---- steps after the path (post_oracle.cpp) ----
def tonemap_state(radiance, state, albedo=None, mode=0, modulate_albedo=False, gamma_correction=True, exposure=0.0, exposure_alpha=0.0):
    """orc_tonemap_state: `state` (6 floats) is read as the previous frame's and overwritten with this frame's."""
    img = np.ascontiguousarray(radiance, np.float32)
    alb = np.ascontiguousarray(albedo, np.float32) if albedo is not None else None
    out = np.empty_like(img)
    mx = np.zeros(4, np.float32)
    lib().orc_tonemap_state(
        wire.ptr(img), wire.ptr(alb) if alb is not None else None, wire.ptr(out), C.c_uint32(img.shape[1]), C.c_uint32(img.shape[0]), C.c_uint32(mode),
        C.c_uint32(1 if modulate_albedo else 0), C.c_uint32(1 if gamma_correction else 0), C.c_float(exposure), wire.ptr(mx), C.c_float(exposure_alpha), wire.ptr(state),
    )
    return out, mx


def tonemap(radiance, albedo=None, mode=0, modulate_albedo=False, gamma_correction=True, exposure=0.0):
    img = np.ascontiguousarray(radiance, np.float32)
    alb = np.ascontiguousarray(albedo, np.float32) if albedo is not None else None
    out = np.empty_like(img)
    mx = np.zeros(4, np.float32)
    lib().orc_tonemap(
        wire.ptr(img),
        wire.ptr(alb) if alb is not None else None,
        wire.ptr(out),
        C.c_uint32(img.shape[1]),
        C.c_uint32(img.shape[0]),
        C.c_uint32(mode),
        C.c_uint32(1 if modulate_albedo else 0),
        C.c_uint32(1 if gamma_correction else 0),
        C.c_float(exposure),
        wire.ptr(mx),
    )
    return out, mx


def image_compare(image1, image2, metric=0, quantization=1024):
    a = np.ascontiguousarray(image1, np.float32)
    b = np.ascontiguousarray(image2, np.float32)
    s, o = C.c_uint32(0), C.c_uint32(0)
    lib().orc_image_compare(wire.ptr(a), wire.ptr(b), C.c_uint32(a.shape[1]), C.c_uint32(a.shape[0]), C.c_uint32(metric), C.c_uint32(quantization), C.byref(s), C.byref(o))
    return s.value, bool(o.value)


def accumulate(frame_out, history, views, reprojection=True, demodulate_albedo=False, history_limit=0.0, instance_index_map=None):
    """orc_accumulate over the same descriptor the product takes (stratum_amd.post.accumulate_desc)."""
    from stratum_amd.post import accumulate_desc

    keep = []
    d, out_c, out_m = accumulate_desc(frame_out, history, views, reprojection, demodulate_albedo, history_limit, instance_index_map, keep)
    lib().orc_accumulate(C.byref(d))
    return out_c, out_m



def nvdb_probe(grid_bytes, coords, points):
    """The oracle's NanoVDB reader on its own: (bbox_min, bbox_max, root_max, values at coords, maps of points)."""
    L = lib()
    grid = np.ascontiguousarray(grid_bytes, dtype=np.uint8)
    coords = np.ascontiguousarray(coords, dtype=np.int32)
    points = np.ascontiguousarray(points, dtype=np.float32)
    n, m = coords.shape[0], points.shape[0]
    values, header, maps = np.zeros(n, np.float32), np.zeros(8, np.int32), np.zeros((m, 4, 3), np.float32)
    root_max = C.c_float()
    rc = L.orc_nvdb_probe(
        grid.ctypes.data_as(C.c_void_p), C.c_uint64(grid.size), coords.ctypes.data_as(C.c_void_p), n, values.ctypes.data_as(C.c_void_p),
        header.ctypes.data_as(C.c_void_p), C.byref(root_max), points.ctypes.data_as(C.c_void_p), m, maps.ctypes.data_as(C.c_void_p),
    )
    if rc != 0:
        raise RuntimeError("orc_nvdb_probe failed (%d)" % rc)
    return header[:3].copy(), header[3:6].copy(), root_max.value, values, maps
