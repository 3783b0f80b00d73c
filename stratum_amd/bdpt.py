"""Host-side mirror of the reference renderer component `stm::BDPT` (src/Node/BDPT.{hpp,cpp})
above the C ABI of libstratum_hip.so.

Same knobs, same defaults, same flag resolution: the constructor sets the default sampling
flags and push constants of BDPT.cpp:55-76 and parses the reference's `--key=value` arguments
(`minPathVertices`, `maxPathVertices`, `maxDiffuseVertices`, repeated `bdptFlag=[~]name`,
BDPT.cpp:78-127); `update()` is where the reference binds the scene descriptors
(BDPT.cpp:341-421) and here uploads the scene arrays; `render()` replaces the recorded
dispatch sequence (BDPT.cpp:423-838) by one sthip_render call.
"""
import ctypes as C
import os

import numpy as np

from . import wire
from ._lib import StratumHipError, lib


def _flag_key(name):
    # to_string(BDPTFlagBits) lower-cased with spaces removed (BDPT.cpp:107-116)
    table = {
        "ePerformanceCounters": "performancecounters",
        "eRemapThreads": "remapthreads",
        "eCoherentRR": "coherentrr",
        "eCoherentSampling": "coherentsampling",
        "eFlipTriangleUVs": "fliptriangleuvs",
        "eFlipNormalMaps": "flipnormalmaps",
        "eAlphaTest": "alphatest",
        "eNormalMaps": "normalmaps",
        "eShadingNormalShadowFix": "shadingnormalshadowfix",
        "eRayCones": "raycones",
        "eSampleBSDFs": "samplebsdfs",
        "eNEE": "nee",
        "eNEEReservoirs": "neereservoirs",
        "eNEEReservoirReuse": "neereservoirreuse",
        "eMIS": "mis",
        "eSampleLightPower": "samplelightpower",
        "eUniformSphereSampling": "uniformspheresampling",
        "ePresampleLights": "presamplelights",
        "eDeferShadowRays": "defershadowrays",
        "eConnectToViews": "connecttoviews",
        "eConnectToLightPaths": "connecttolightpaths",
        "eLVC": "lightvertexcache",
        "eLVCReservoirs": "lvcreservoirs",
        "eLVCReservoirReuse": "lvcreservoirreuse",
        "eHashGridJitter": "jitterhashgridlookups",
        "eSampleEnvironmentMapDirectly": "sampleenvironmentmapdirectly",
    }
    return table[name]


_FLAG_BY_KEY = {_flag_key(n): i for i, n in enumerate(wire.FLAG_NAMES)}


def known_flag(arg):
    """Whether --bdptFlag would act on `arg` (BDPT.cpp:94-127 ignores a name it does not know; a tool that measures may not)."""
    return bool(arg) and arg.lstrip("~!").lower() in _FLAG_BY_KEY


class BDPT:
    def __init__(self, device=0, args=None):
        self._lib = lib()
        h = C.c_void_p()
        rc = self._lib.sthip_create(device, C.byref(h))
        if rc != 0:
            raise StratumHipError("sthip_create(%d) failed (%d): %s" % (device, rc, self._lib.sthip_last_error(None).decode()))
        self._h = h
        self.device = device
        self._scene = None
        self._stale_volumes = set()  # indices of gVolumes that set_volume replaced: the scene object's grids are older
        self.volume_world_bbox = {}  # volume index -> world box (6 doubles) of the grid set_volume installed
        self._device_images = set()  # indices of gImages whose texels set_images took from a device pointer: the scene object's are older
        self._prev_result = None
        self.half_color_precision = False  # BDPT.hpp mHalfColorPrecision: colour images RGBA16F (set_half_color_precision)
        self.set_args(args)

    def set_args(self, args=None):
        """The renderer arguments of the constructor, from the defaults (BDPT.cpp:55-127): what `args` does not name goes back to
        its default. A living renderer may call it again; the scene, the options and the colour precision stay."""
        self.mSamplingFlags = wire.DEFAULT_SAMPLING_FLAGS
        self.mPushConstants = wire.default_push_constants(0, 0, 0)
        self.mPushConstants.gLightPathCount = 64  # BDPT.cpp:70: the size of the light vertex cache unless --lightPathCount says otherwise (without eLVC: one path per pixel, :469-470)
        args = args or {}
        for key, field in (
            ("minPathVertices", "gMinPathVertices"),
            ("maxPathVertices", "gMaxPathVertices"),
            ("maxDiffuseVertices", "gMaxDiffuseVertices"),
            ("maxNullCollisions", "gMaxNullCollisions"),
            ("lightPresampleTileSize", "gLightPresampleTileSize"),
            ("lightPresampleTileCount", "gLightPresampleTileCount"),
            ("lightPathCount", "gLightPathCount"),
            ("reservoirM", "gReservoirM"),
            ("reservoirMaxM", "gReservoirMaxM"),
            ("reservoirSpatialM", "gReservoirSpatialM"),
            ("hashGridBucketCount", "gHashGridBucketCount"),
        ):
            if key in args:
                setattr(self.mPushConstants, field, int(args[key]))
        if "environmentSampleProbability" in args:  # BDPT.cpp:82
            self.mPushConstants.gEnvironmentSampleProbability = float(args["environmentSampleProbability"])
        for a in args.get("bdptFlag", []):
            self.set_flag(a)

    # BDPT.cpp:94-127
    def set_flag(self, arg):
        if not arg:
            return
        on = True
        if arg[0] in "~!":
            on, arg = False, arg[1:]
        bit = _FLAG_BY_KEY.get(arg.lower())
        if bit is None:
            if os.environ.get("STHIP_STRICT_FLAGS"):  # the measuring tools and bench.py set it: a misspelt flag is an error there
                raise ValueError("unknown --bdptFlag name %r" % (arg,))
            return  # the reference silently ignores unknown names
        if on:
            self.mSamplingFlags |= 1 << bit
        else:
            self.mSamplingFlags &= ~(1 << bit)

    def _check(self, rc, what):
        if rc != 0:
            raise StratumHipError("%s failed (%d): %s" % (what, rc, self._lib.sthip_last_error(self._h).decode()))

    def close(self):
        if getattr(self, "_h", None):
            for ptr in getattr(self, "_host_blocks", []):  # alloc_host_outputs (completes the frames in flight first)
                self._lib.sthip_host_free(self._h, C.c_void_p(ptr))
            self._host_blocks = []
            self._tickets = {}
            self._lib.sthip_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- BDPT::update: (re)bind the scene ----
    def update(self, scene):
        if scene is self._scene and self._device_images:  # the same object goes up again: its arrays first take what is resident
            for index in sorted(self._device_images):
                scene.images[index] = self.read_image(index, 0)
        self._device_images = set()
        if scene is self._scene and self._stale_volumes:  # ... and the grids set_volume left newer on the device
            for index in sorted(self._stale_volumes):
                scene.volumes[index] = self.read_volume(index)
        self._stale_volumes = set()
        d = scene.desc()
        formats, formats1 = scene.formats()
        if formats.any() or formats1.any():  # some image is a uint8 array: it goes up, and stays resident, as 8-bit texels
            rc = self._lib.sthip_scene_upload_formats(self._h, C.byref(d), wire.ptr(formats) if formats.size else None, wire.ptr(formats1) if formats1.size else None)
            self._check(rc, "sthip_scene_upload_formats")
        else:
            self._check(self._lib.sthip_scene_upload(self._h, C.byref(d)), "sthip_scene_upload")
        scene.dirty_vertices = None  # (the whole vertex array went up)
        self._scene = scene
        if getattr(scene, "environment_tables", "host") == "device":  # SceneBuilder.build(environment_tables="device"): zero-filled tables went up
            self.set_environment()

    def update_transforms(self, scene):
        """Only instance transforms changed since update(scene) (SceneData.set_instance_transform): the top level of the
        acceleration structure is rebuilt, the bottom levels stay in HBM (the reference's cached BLASes, Scene.cpp:435-459).
        Raises StratumHipError (unsupported) if an instance of the merged identity-transform mesh moved: call update()."""
        rc = self._lib.sthip_scene_update_transforms(
            self._h, wire.ptr(scene.transforms), wire.ptr(scene.inverse_transforms), wire.ptr(scene.motion_transforms), scene.instances.shape[0]
        )
        self._check(rc, "sthip_scene_update_transforms")
        self._scene = scene

    def set_transforms(self, transforms, inverse=None, motion=None, derive_motion=False, top_level="host"):
        """New instance transforms for the resident scene from host or device memory (sthip_scene_set_transforms). Each array is
        a wire.TransformData / float32 (n, 3, 4) numpy array, or anything with data_ptr() (a contiguous float32 torch tensor
        of n x 12 values on this device); all given arrays must be of one kind. inverse=None: the library derives the inverse
        (scene.transform_inverse's arithmetic); motion=None: the identity, or with derive_motion=True tmul(resident transform
        before the call, new inverse). top_level: "host" (binned SAH) or "device" (top_level.hip). The scene object handed to
        update() does NOT follow: read_transforms() says what is resident. Returns sthip_transforms_info as a dict."""
        if top_level not in ("host", "device"):
            raise ValueError('set_transforms: top_level is "host" or "device"')
        d = wire.TransformsDesc()
        keep = []
        device = hasattr(transforms, "data_ptr")

        def pointer(a, name):
            if a is None:
                return None
            if hasattr(a, "data_ptr") != device:
                raise ValueError("set_transforms: host and device arrays cannot be mixed")
            if device:
                if "float32" not in str(a.dtype) or not a.is_contiguous() or a.numel() % 12:
                    raise ValueError("set_transforms: %s must be a contiguous float32 tensor of n x 12 values" % name)
                count = a.numel() // 12
                ptr = int(a.data_ptr())
            else:
                a = np.asarray(a)
                a = np.ascontiguousarray(a["m"] if a.dtype == wire.TransformData else a, dtype=np.float32).reshape(-1, 3, 4)
                keep.append(a)
                count, ptr = a.shape[0], a.ctypes.data
            if name == "transforms":
                d.instance_count = count
            elif count != d.instance_count:
                raise ValueError("set_transforms: %s has %d records, transforms %d" % (name, count, d.instance_count))
            return ptr

        d.transforms = pointer(transforms, "transforms")
        d.inverse_transforms = pointer(inverse, "inverse")
        d.motion_transforms = pointer(motion, "motion")
        d.device_ptr = 1 if device else 0
        d.top_level = 1 if top_level == "device" else 0
        d.derive_motion = 1 if derive_motion else 0
        info = wire.TransformsInfo()
        self._check(self._lib.sthip_scene_set_transforms(self._h, C.byref(d), C.sizeof(d), C.byref(info)), "sthip_scene_set_transforms")
        return {f: getattr(info, f) for f, _ in wire.TransformsInfo._fields_}

    def read_transforms(self, first=0, count=None):
        """The resident transforms, inverse transforms and motion transforms [first, first + count) as three float32 arrays
        (count, 3, 4) (sthip_scene_read_transforms); all instances by default."""
        n = int((self._scene.instances.shape[0] - first if self._scene is not None else 0) if count is None else count)
        out = [np.zeros((n, 3, 4), np.float32) for _ in range(3)]
        self._check(self._lib.sthip_scene_read_transforms(self._h, int(first), n, *[wire.ptr(a) if n else None for a in out]), "sthip_scene_read_transforms")
        return tuple(out)

    def read_top_level(self):
        """The resident top level (sthip_scene_read_top_level): {"entry_boxes": float32 (entries, 2, 3) lo / hi, exact;
        "nodes": a wire.TopNode array; "root": node index or 0xFFFFFFFF (no top level); "center": float32 (3,); "radius"}."""
        ne, nn, root = C.c_uint32(), C.c_uint32(), C.c_uint32()
        cr = np.zeros(4, np.float32)
        self._check(self._lib.sthip_scene_read_top_level(self._h, None, None, 0, C.byref(ne), C.byref(nn), C.byref(root), wire.ptr(cr)), "sthip_scene_read_top_level")
        boxes = np.zeros((ne.value, 2, 3), np.float32)
        nodes = np.zeros(nn.value, wire.TopNode)
        rc = self._lib.sthip_scene_read_top_level(
            self._h, wire.ptr(boxes) if ne.value else None, wire.ptr(nodes) if nn.value else None, nn.value, C.byref(ne), C.byref(nn), C.byref(root), wire.ptr(cr)
        )
        self._check(rc, "sthip_scene_read_top_level")
        return {"entry_boxes": boxes, "nodes": nodes, "root": root.value, "center": cr[:3].copy(), "radius": float(cr[3])}

    def update_vertices(self, scene):
        """Only vertex records changed since update(scene) (SceneData.set_vertices): the dirty range goes to the device, the
        leaf triangles are gathered again and the bottom levels refitted in place (sthip_scene_update_vertices). Returns
        sthip_refit_info as a dict; `rebuilt` = 1 when the resident layout had to be built again from the kept scene.
        Raises StratumHipError (unsupported) for such a layout with keep_scene = 0: call update()."""
        lo, hi = scene.dirty_vertices or (0, 0)
        info = wire.RefitInfo()
        part = scene.vertices[lo:hi] if hi > lo else scene.vertices[:0]
        rc = self._lib.sthip_scene_update_vertices(self._h, wire.ptr(part) if hi > lo else wire.ptr(scene.vertices), lo, hi - lo, C.byref(info))
        self._check(rc, "sthip_scene_update_vertices")
        scene.dirty_vertices = None
        self._scene = scene
        return {f: getattr(info, f) for f, _ in wire.RefitInfo._fields_ if f != "pad"}

    def set_rigs(self, rigs):
        """Make rigs resident (sthip_scene_set_rigs). `rigs`: a list of dicts with "first_vertex", "vertex_count", optionally
        "blend_targets" (up to 4 wire.PackedVertexData arrays of vertex_count records), and "weights" (a wire.VertexWeight
        array of vertex_count records) with "bone_count". The rest pose of each rig is the resident records of its range as
        they are now. An empty list drops the rigs; so does update()."""
        n = len(rigs)
        descs = (wire.RigDesc * max(1, n))()
        keep = []  # (the arrays the descriptors point into, alive for the call)
        for d, rig in zip(descs, rigs):
            d.first_vertex, d.vertex_count = int(rig["first_vertex"]), int(rig["vertex_count"])
            targets = list(rig.get("blend_targets") or [])
            d.blend_target_count = len(targets)
            for k, t in enumerate(targets[:4]):
                t = np.ascontiguousarray(t, dtype=wire.PackedVertexData)
                if t.shape[0] != d.vertex_count:
                    raise ValueError("a blend target has %d records, the rig %d" % (t.shape[0], d.vertex_count))
                keep.append(t)
                d.blend_targets[k] = t.ctypes.data
            d.bone_count = int(rig.get("bone_count", 0))
            w = rig.get("weights")
            if w is not None:
                w = np.ascontiguousarray(w, dtype=wire.VertexWeight)
                if w.shape[0] != d.vertex_count:
                    raise ValueError("weights has %d records, the rig %d" % (w.shape[0], d.vertex_count))
                keep.append(w)
                d.weights = w.ctypes.data
        self._check(self._lib.sthip_scene_set_rigs(self._h, descs, n), "sthip_scene_set_rigs")

    def animate(self, poses):
        """Pose the resident rigs on the device and refit (sthip_scene_animate). `poses`: one dict per rig with optionally
        "blend_factors" (up to 4 floats) and "bones" (a wire.TransformData array, or float32 of shape (bone_count, 3, 4)).
        Only the pose crosses to the device. Returns sthip_refit_info as a dict, as update_vertices does."""
        n = len(poses)
        c_poses = (wire.RigPose * max(1, n))()
        keep = []
        for c, pose in zip(c_poses, poses):
            for k, f in enumerate(list(pose.get("blend_factors", ()))[:4]):
                c.blend_factors[k] = float(f)
            b = pose.get("bones")
            if b is not None:
                b = np.asarray(b)
                b = np.ascontiguousarray(b["m"] if b.dtype == wire.TransformData else b, dtype=np.float32).reshape(-1, 3, 4)
                keep.append(b)
                c.bones = b.ctypes.data
        info = wire.RefitInfo()
        self._check(self._lib.sthip_scene_animate(self._h, c_poses, n, C.byref(info)), "sthip_scene_animate")
        return {f: getattr(info, f) for f, _ in wire.RefitInfo._fields_ if f != "pad"}

    def set_vertices(self, first_vertex, positions, normals=None, texcoords=None, recompute_normals=False):
        """New vertices for the resident scene from strided streams (sthip_scene_set_vertices): records first_vertex ..
        first_vertex + N - 1 become {positions[i], u, normals[i], v}, bit copies; an absent stream leaves its fields as they
        are resident. With recompute_normals=True (and normals=None) the shading normals of the range are made again on the
        device from the moved positions: the normalised sum of the area-weighted face vectors around each vertex, in the order
        include/sthip.h fixes. Each stream is a float32 numpy array of shape (N, 3) / (N, 2) with any row stride and inner
        stride 1, or anything with data_ptr(), shape and stride() (a float32 torch tensor or view on this device); all given
        streams must be of one kind. Strides come from the object. The gather, the refit and the top level follow as for
        update_vertices. The scene object handed to update() does NOT follow: its `vertices` are behind the device from here
        on, and read_vertices() says what is resident. Returns sthip_refit_info as a dict."""
        d = wire.VertexStreams()
        d.struct_size = C.sizeof(wire.VertexStreams)
        d.first_vertex = int(first_vertex)
        d.recompute_normals = 1 if recompute_normals else 0
        device = hasattr(positions, "data_ptr")
        keep = []

        def stream(a, name, width):
            if a is None:
                return None, 0
            if hasattr(a, "data_ptr") != device:
                raise ValueError("set_vertices: host and device streams cannot be mixed")
            if device:
                if "float32" not in str(a.dtype) or len(a.shape) != 2 or a.shape[1] != width or (a.shape[0] and a.stride(1) != 1):
                    raise ValueError("set_vertices: %s must be a float32 tensor of shape (N, %d) with inner stride 1" % (name, width))
                count, pointer, step = int(a.shape[0]), int(a.data_ptr()), int(a.stride(0)) * 4
            else:
                a = np.asarray(a)
                if a.dtype != np.float32 or a.ndim != 2 or a.shape[1] != width or (a.shape[0] and a.strides[1] != 4):
                    raise ValueError("set_vertices: %s must be a float32 array of shape (N, %d) with inner stride 1" % (name, width))
                keep.append(a)
                count, pointer, step = int(a.shape[0]), int(a.ctypes.data), int(a.strides[0])
            if name == "positions":
                d.vertex_count = count
            elif count != d.vertex_count:
                raise ValueError("set_vertices: %s has %d elements, positions %d" % (name, count, d.vertex_count))
            if step < 0:
                raise ValueError("set_vertices: %s has a negative row stride" % name)
            return pointer, step

        d.positions, d.position_stride = stream(positions, "positions", 3)
        d.normals, d.normal_stride = stream(normals, "normals", 3)
        d.texcoords, d.texcoord_stride = stream(texcoords, "texcoords", 2)
        d.device_ptr = 1 if device else 0
        info = wire.RefitInfo()
        self._check(self._lib.sthip_scene_set_vertices(self._h, C.byref(d), C.byref(info)), "sthip_scene_set_vertices")
        return {f: getattr(info, f) for f, _ in wire.RefitInfo._fields_ if f != "pad"}

    def read_vertices(self, first, count):
        """The resident vertex records [first, first + count) as a wire.PackedVertexData array (sthip_scene_read_vertices)."""
        out = np.zeros(int(count), dtype=wire.PackedVertexData)
        self._check(self._lib.sthip_scene_read_vertices(self._h, int(first), int(count), wire.ptr(out)), "sthip_scene_read_vertices")
        return out

    def read_image(self, index, level=0):
        """The stored texels of one level of gImages[index] in the image's resident format (sthip_scene_read_image): a
        float32 array (h, w, 4) of an RGBA32F image, a uint8 array (h, w, 4) of an RGBA8_UNORM one."""
        im = self._scene.images[int(index)]
        h, w = max(1, im.shape[0] >> int(level)), max(1, im.shape[1] >> int(level))
        out = np.zeros((h, w, 4), im.dtype)
        self._check(self._lib.sthip_scene_read_image(self._h, int(index), int(level), wire.ptr(out), out.nbytes), "sthip_scene_read_image")
        return out

    def set_environment(self, value=None, image=None, device_ptr=False):
        """Replace the environment of the resident scene (sthip_scene_set_environment): `value` = three floats, the new
        ImageValue3::value; `image` = the new texels of the environment's image, a C-contiguous float32 array (H, W, 4) of the
        resident extent, or with device_ptr=True anything with data_ptr() and shape (a torch tensor on this device: float32,
        contiguous, (H, W, 4)). The mip chain and the four dist2d tables are made again on the device. With neither, the tables
        are built from the resident texels. The scene object handed to update() follows (value, host image; with a device
        image and for the tables, read_image / read_distributions say what is resident). After a host image the scene object's
        `distributions` no longer belong to its image: it is marked environment_tables = "device", so that a later update(scene)
        has the device build them again behind the upload. Returns sthip_environment_info as a dict."""
        scene = self._scene
        d = wire.EnvironmentDesc()
        d.struct_size = C.sizeof(wire.EnvironmentDesc)
        d.material_address = (scene.environment_address if scene is not None else 0) & 0xFFFFFFFF
        keep = []
        if value is not None:
            v = np.ascontiguousarray(np.asarray(value, dtype=np.float32).reshape(3))
            keep.append(v)
            d.value = v.ctypes.data
        if image is not None:
            if device_ptr:
                if tuple(image.shape[2:]) != (4,) or "float32" not in str(image.dtype) or not image.is_contiguous():
                    raise ValueError("set_environment: a device image must be a contiguous float32 tensor (H, W, 4)")
                d.pixels, d.device_ptr = int(image.data_ptr()), 1
            else:
                if image.dtype != np.float32 or not image.flags["C_CONTIGUOUS"] or image.ndim != 3 or image.shape[2] != 4:
                    raise ValueError("set_environment: the image must be a C-contiguous float32 array (H, W, 4)")
                d.pixels = image.ctypes.data
            d.height, d.width = int(image.shape[0]), int(image.shape[1])
        info = wire.EnvironmentInfo()
        self._check(self._lib.sthip_scene_set_environment(self._h, C.byref(d), C.byref(info)), "sthip_scene_set_environment")
        if value is not None:  # the arrays a later update() would send hold what is resident
            a = scene.environment_address
            scene.materials[a : a + 12] = keep[0].view(np.uint8)
        if image is not None and not device_ptr:
            index = int(scene.materials[scene.environment_address + 12 : scene.environment_address + 16].view(np.uint32)[0])
            scene.images[index] = image
            scene.environment_tables = "device"  # (scene.distributions are the tables of the image before)
        return {"device_ms": info.device_ms, "total_ms": info.total_ms}

    def read_distributions(self, first=0, count=None):
        """The resident gDistributions[first, first + count) as a float32 array (sthip_scene_read_distributions); all by default."""
        n = int((self._scene.distributions.size - first if self._scene is not None else 0) if count is None else count)  # (no scene: the library says so)
        out = np.zeros(n, np.float32)
        self._check(self._lib.sthip_scene_read_distributions(self._h, int(first), n, wire.ptr(out) if n else None), "sthip_scene_read_distributions")
        return out

    def set_images(self, images=None, masks=None, device_ptr=False):
        """Replace level 0 of resident images (sthip_scene_set_images). `images`: {index: texels} for gImages, `masks`: {index:
        texels} for gImage1s — or a list of (index, texels) pairs. Texels are C-contiguous numpy arrays in the image's resident
        format and extent: (H, W, 4) float32 or uint8 for gImages, (H, W) for gImage1s (the arrays convert_material returns go
        in as they are); with device_ptr=True anything with data_ptr() and shape (a contiguous torch tensor on this device) of
        that layout. All entries of one call are applied together; the mip chains, the scan of the images materials name and
        the material analysis are made again. The scene object handed to update() follows host texels at once. Texels of
        gImages that came from a device pointer are fetched into it (read_image) if the same object is handed to update()
        again; until then, and for alpha masks from a device pointer (there is no read call for them: keep your own copy),
        the scene object holds the texels before. Returns sthip_images_info as a dict."""
        if self._scene is None:
            raise StratumHipError("set_images: no scene is bound (update() has not run)")
        entries = []
        for which, group in ((0, images), (1, masks)):
            for index, a in (group.items() if isinstance(group, dict) else (group or ())):
                entries.append((which, int(index), a))
        arr = (wire.ImageUpdate * max(1, len(entries)))()
        for e, (which, index, a) in zip(arr, entries):
            shape = tuple(a.shape)
            if len(shape) != (2 if which else 3) or (not which and shape[2] != 4):
                raise ValueError("set_images: %s[%d] takes texels of shape %s" % ("gImage1s" if which else "gImages", index, "(H, W)" if which else "(H, W, 4)"))
            if device_ptr:
                if not a.is_contiguous():
                    raise ValueError("set_images: a device image must be contiguous")
                e.pixels, e.device_ptr = int(a.data_ptr()), 1
            else:
                if a.dtype not in (np.float32, np.uint8) or not a.flags["C_CONTIGUOUS"]:
                    raise ValueError("set_images: texels must be a C-contiguous float32 or uint8 array")
                e.pixels = a.ctypes.data
            resident = self._scene.images1 if which else self._scene.images
            if index < len(resident) and str(resident[index].dtype) not in str(a.dtype):
                raise ValueError("set_images: %s[%d] is resident as %s (a change of format is an upload)" % ("gImage1s" if which else "gImages", index, resident[index].dtype))
            e.which, e.index, e.height, e.width = which, index, int(shape[0]), int(shape[1])
        info = wire.ImagesInfo()
        self._check(self._lib.sthip_scene_set_images(self._h, arr, len(entries), C.sizeof(wire.ImageUpdate), C.byref(info)), "sthip_scene_set_images")
        for which, index, a in entries:
            if not device_ptr:  # the arrays a later update() would send hold what is resident
                (self._scene.images1 if which else self._scene.images)[index] = a
                if not which:
                    self._device_images.discard(index)
            elif not which:
                self._device_images.add(index)
        return {f: getattr(info, f) for f, _ in wire.ImagesInfo._fields_ if f != "pad"}

    def set_material_data(self, offset, data):
        """Replace bytes of the resident gMaterialData (sthip_scene_set_material_data): `data` is anything numpy views as bytes
        (a float32 array of constants, a uint32 image index, a wire.MaterialRecord ...); offset and size are multiples of 4.
        The material analysis runs again. The scene object handed to update() follows. Returns sthip_images_info as a dict."""
        if self._scene is None:
            raise StratumHipError("set_material_data: no scene is bound (update() has not run)")
        b = np.ascontiguousarray(data).reshape(-1).view(np.uint8)
        info = wire.ImagesInfo()
        self._check(self._lib.sthip_scene_set_material_data(self._h, int(offset), wire.ptr(b) if b.size else None, b.size, C.byref(info)), "sthip_scene_set_material_data")
        self._scene.materials[int(offset) : int(offset) + b.size] = b
        return {f: getattr(info, f) for f, _ in wire.ImagesInfo._fields_ if f != "pad"}

    def read_image_range(self, index):
        """(lo, hi, nan_mask) the context holds for gImages[index]: two float32 arrays of 4 and an int (sthip_scene_read_image_range)."""
        lo, hi, mask = np.zeros(4, np.float32), np.zeros(4, np.float32), C.c_uint32(0)
        self._check(self._lib.sthip_scene_read_image_range(self._h, int(index), wire.ptr(lo), wire.ptr(hi), C.byref(mask)), "sthip_scene_read_image_range")
        return lo, hi, int(mask.value)

    def convert_material(self, kind, diffuse=None, specular=None, transmittance=None, roughness=None, input=None, output_format=1):
        """sthip_convert_material in its host form (kernels/material_convert.hlsl). `kind`: a name of wire.CONVERT or its
        number. Sources are C-contiguous uint8 or float32 arrays, (H, W, 4) or, for `roughness` / `input`, (H, W), or a
        wire.TexelImage (an asset's image in its own texel format, decoded in the kernel; a one-channel source takes its
        channel 0); None = absent. Returns a dict: "output" (three (H, W, 4) arrays), "alpha_mask" ((H, W), or None without
        `diffuse`) and "min_alpha" (int) for the two material kinds, "roughness" ((H, W)) for the two roughness kinds; uint8
        with output_format 1, float32 with 0."""
        kind = wire.CONVERT[kind] if isinstance(kind, str) else int(kind)
        sources = {"gDiffuse": diffuse, "gSpecular": specular, "gTransmittance": transmittance, "gRoughness": roughness, "gInput": input}
        formats = {"gDiffuse": "diffuse_format", "gSpecular": "specular_format", "gTransmittance": "transmittance_format", "gRoughness": "roughness_format", "gInput": "input_format"}
        d = wire.ConvertMaterialDesc()
        d.kind, d.device_ptrs, d.output_format = kind, 0, int(output_format)
        extent = None
        for name, a in sources.items():
            if a is None:
                continue
            channels = 1 if name in ("gRoughness", "gInput") else 4
            if isinstance(a, wire.TexelImage):
                shape, address = (a.height, a.width), a.data.ctypes.data
                fmt = {0: 31, 1: 19}.get(a.format, a.format) if channels == 1 else a.format  # (0 / 1 of a TexelImage are the four-channel forms)
            else:
                if a.dtype not in (np.uint8, np.float32) or not a.flags["C_CONTIGUOUS"] or a.ndim != (2 if channels == 1 else 3) or (channels == 4 and a.shape[2] != 4):
                    raise ValueError("%s must be a C-contiguous uint8 or float32 array of %d channel(s), or a TexelImage" % (name, channels))
                shape, address, fmt = a.shape[:2], a.ctypes.data, (1 if a.dtype == np.uint8 else 0)
            if extent is None:
                extent = shape
            elif shape != extent:
                raise ValueError("%s has the extent %s, the first image %s: all sources must have one extent" % (name, shape, extent))
            setattr(d, name, address)
            setattr(d, formats[name], fmt)
        if extent is None:
            raise ValueError("convert_material: no source image")
        H, W = extent
        d.width, d.height = W, H
        out_dtype = np.uint8 if output_format else np.float32
        if kind in (wire.CONVERT["GltfPbr"], wire.CONVERT["DiffuseSpecular"]):
            out = [np.zeros((H, W, 4), out_dtype) for _ in range(3)]
            mask = np.zeros((H, W), out_dtype) if diffuse is not None else None
            min_alpha = np.zeros(1, np.uint32)
            for k in range(3):
                d.gOutput[k] = out[k].ctypes.data
            d.gOutputAlphaMask = mask.ctypes.data if mask is not None else None
            d.gOutputMinAlpha = min_alpha.ctypes.data
            self._check(self._lib.sthip_convert_material(self._h, C.byref(d)), "sthip_convert_material")
            return {"output": out, "alpha_mask": mask, "min_alpha": int(min_alpha[0])}
        rough = np.zeros((H, W), out_dtype)
        d.gRoughnessRW = rough.ctypes.data
        self._check(self._lib.sthip_convert_material(self._h, C.byref(d)), "sthip_convert_material")
        return {"roughness": rough}

    def decode_texels(self, image, dst_format=0, channel=None):
        """sthip_decode_texels in its host form: a wire.TexelImage (an asset's image in its own texel format: sRGB, 16-bit,
        BC1-BC5, ...) to an (H, W, 4) array, or with `channel` 0..3 to the (H, W) array of that channel; float32 with
        dst_format 0, uint8 with 1."""
        if not hasattr(self._lib, "sthip_decode_texels"):
            raise StratumHipError("this libstratum_hip.so has no sthip_decode_texels")
        d = wire.DecodeTexelsDesc()
        d.src_format, d.width, d.height, d.device_ptrs, d.dst_format = image.format, image.width, image.height, 0, int(dst_format)
        d.dst_channels, d.channel = (4, 0) if channel is None else (1, int(channel))
        out = np.zeros((image.height, image.width, 4) if channel is None else (image.height, image.width), np.uint8 if dst_format else np.float32)
        d.src, d.dst = image.data.ctypes.data, out.ctypes.data
        self._check(self._lib.sthip_decode_texels(self._h, C.byref(d)), "sthip_decode_texels")
        return out

    def build_volume(self, dense, origin=(0, 0, 0), voxel_size=1.0, translation=(0.0, 0.0, 0.0), name="", dims=None, out=None, capacity=None):
        """sthip_build_volume: a NanoVDB float grid (FogVolume) from a dense box, built on the device; the bytes are those of
        nvdb.dense_to_nanovdb. `dense`: a C-contiguous float32 [nx, ny, nz] array, or an int — a device pointer, with `dims`.
        `out` None: the grid comes back as a uint8 array (two calls: the size, then the grid); `out` an int: a device pointer
        of `capacity` bytes the grid is built into. Returns (grid or None, info dict)."""
        d, _keep = self._dense_desc(dense, origin, voxel_size, translation, name, dims)
        info = wire.VolumeInfo()
        as_dict = lambda: {f: (list(getattr(info, f)) if hasattr(getattr(info, f), "__len__") else getattr(info, f)) for f, _ in wire.VolumeInfo._fields_}
        if out is not None:
            self._check(self._lib.sthip_build_volume(self._h, C.byref(d), C.c_void_p(int(out)), int(capacity), 1, C.byref(info)), "sthip_build_volume")
            return None, as_dict()
        rc = self._lib.sthip_build_volume(self._h, C.byref(d), None, 0, 0, C.byref(info))  # the size (refused: capacity 0)
        if info.bytes == 0:
            self._check(rc, "sthip_build_volume")
        grid = np.empty(int(info.bytes), np.uint8)
        self._check(self._lib.sthip_build_volume(self._h, C.byref(d), wire.ptr(grid), grid.size, 0, C.byref(info)), "sthip_build_volume")
        return grid, as_dict()

    def _dense_desc(self, dense, origin, voxel_size, translation, name, dims):
        """(sthip_dense_volume_desc, what must stay alive) for a numpy array or a device pointer with `dims`."""
        d = wire.DenseVolumeDesc()
        d.struct_size = C.sizeof(wire.DenseVolumeDesc)
        if isinstance(dense, np.ndarray):
            if dense.dtype != np.float32 or dense.ndim != 3 or not dense.flags["C_CONTIGUOUS"]:
                raise ValueError("dense must be a C-contiguous float32 [nx, ny, nz] array")
            d.dense, d.dense_is_device, dims = dense.ctypes.data, 0, dense.shape
        else:
            d.dense, d.dense_is_device = int(dense.data_ptr() if hasattr(dense, "data_ptr") else dense), 1
        for k in range(3):
            d.dims[k], d.origin[k], d.translation[k] = int(dims[k]), int(origin[k]), float(translation[k])
        d.voxel_size = float(voxel_size)
        d.name = name.encode() if isinstance(name, str) else name
        return d, dense

    def set_volume(self, index, grid=None, dense=None, origin=(0, 0, 0), voxel_size=1.0, translation=(0.0, 0.0, 0.0), name="", dims=None, grid_bytes=None):
        """sthip_scene_set_volume: resident grid `index` is replaced without an upload, by a finished NanoVDB buffer (`grid`: a
        uint8 array, or a device pointer with `grid_bytes`) or by a dense box built on the device (`dense`: as build_volume
        takes it). The scene object's copy of the grid is marked stale and fetched (read_volume) before the scene is packed
        again by update(). Returns the info dict; its world_bbox is kept in self.volume_world_bbox[index] for
        view_medium_instances."""
        if (grid is None) == (dense is None):
            raise ValueError("set_volume: exactly one of grid and dense")
        s = wire.VolumeSource()
        s.struct_size = C.sizeof(wire.VolumeSource)
        if dense is not None:
            d, keep = self._dense_desc(dense, origin, voxel_size, translation, name, dims)
            s.dense = C.pointer(d)
        elif isinstance(grid, np.ndarray):
            keep = np.ascontiguousarray(grid, dtype=np.uint8)
            s.data, s.bytes, s.data_is_device = keep.ctypes.data, keep.size, 0
        else:
            keep = grid
            s.data, s.bytes, s.data_is_device = int(grid.data_ptr() if hasattr(grid, "data_ptr") else grid), int(grid_bytes), 1
        info = wire.VolumeInfo()
        self._check(self._lib.sthip_scene_set_volume(self._h, int(index), C.byref(s), C.byref(info)), "sthip_scene_set_volume")
        self._stale_volumes.add(int(index))
        out = {f: (list(getattr(info, f)) if hasattr(getattr(info, f), "__len__") else getattr(info, f)) for f, _ in wire.VolumeInfo._fields_}
        if dense is None and isinstance(grid, np.ndarray) and keep.size >= 608:
            out["world_bbox"] = [float(x) for x in keep[560:608].view("<f8")]  # GridData::mWorldBBox of the finished buffer
        if dense is not None or isinstance(grid, np.ndarray):
            self.volume_world_bbox[int(index)] = out["world_bbox"]
        else:
            self.volume_world_bbox.pop(int(index), None)  # (a finished device buffer: its header is the caller's to read)
        return out

    def read_volume(self, index):
        """The bytes of resident grid `index` (sthip_scene_read_volume)."""
        n = C.c_uint64(0)
        self._lib.sthip_scene_read_volume(self._h, int(index), None, 0, C.byref(n))
        if n.value == 0:
            self._check(self._lib.sthip_scene_read_volume(self._h, int(index), None, 0, C.byref(n)), "sthip_scene_read_volume")
        grid = np.empty(int(n.value), np.uint8)
        self._check(self._lib.sthip_scene_read_volume(self._h, int(index), wire.ptr(grid), grid.size, C.byref(n)), "sthip_scene_read_volume")
        return grid

    def set_stream(self, stream_handle):
        self._check(self._lib.sthip_set_stream(self._h, C.c_void_p(stream_handle)), "sthip_set_stream")

    def set_option(self, name, value):
        self._check(self._lib.sthip_set_option(self._h, name.encode(), int(value)), "sthip_set_option")

    def set_half_color_precision(self, on):
        """The reference's "Half precision" switch (BDPT.cpp:231,553-558): while on, radiance, albedo and the debug image are
        RGBA16F (np.float16 host arrays, float16 device buffers), as are the colour images of the post calls that follow this
        renderer (post.py). Results are the binary32 ones rounded to nearest even (include/sthip.h: "half_color_precision")."""
        self.set_option("half_color_precision", 1 if on else 0)
        self.half_color_precision = bool(on)

    @property
    def color_dtype(self):
        """numpy dtype of the colour images (radiance, albedo, debug) under the current precision."""
        return np.float16 if self.half_color_precision else np.float32

    CEILINGS = {"triad": 0, "node_gather_table": 1, "node_gather_l2": 2, "node_gather_l1": 3}

    def measure_ceiling(self, kind):
        """Measured memory-system ceiling in GB/s (include/sthip.h: sthip_measure_ceiling)."""
        v = C.c_double(0.0)
        self._check(self._lib.sthip_measure_ceiling(self._h, self.CEILINGS[kind], C.byref(v)), "sthip_measure_ceiling")
        return float(v.value)

    def stats(self):
        s = wire.Stats()
        self._check(self._lib.sthip_get_stats(self._h, C.byref(s)), "sthip_get_stats")
        return {f: (list(getattr(s, f)) if hasattr(getattr(s, f), "__len__") else getattr(s, f)) for f, _ in wire.Stats._fields_}

    def push_constants(self, frame):
        pc = wire.BDPTPushConstants.from_buffer_copy(self.mPushConstants)
        pc.gOutputExtent[0], pc.gOutputExtent[1] = frame.width, frame.height
        pc.gViewCount = frame.views.shape[0]
        pc.gLightCount = self._scene.light_count
        if not (self.mSamplingFlags >> wire.FLAG_NAMES.index("eLVC")) & 1:  # BDPT.cpp:469-470: with the cache on it stays the user's value
            pc.gLightPathCount = frame.width * frame.height
        # BDPT.cpp:393,486-496
        pc.gEnvironmentMaterialAddress = self._scene.environment_address
        if self._scene.environment_address == 0xFFFFFFFF:
            pc.gEnvironmentSampleProbability = 0.0
        if pc.gLightCount == 0:
            pc.gEnvironmentSampleProbability = 1.0
        if not (self._scene.scene_flags & wire.BDPT_FLAG_HAS_MEDIA):  # BDPT.cpp:497-500
            pc.gMaxNullCollisions = 0
        return pc

    # ---- BDPT::render ----
    def render(self, frame, seed_begin=0, seed_count=1, aovs=True, device_outputs=None, packed_tiles=False, debug_mode=0, debug_image=None, host_outputs=None):
        """Host outputs by default (dict of numpy arrays; `host_outputs` = such a dict from an earlier call: its arrays are
        written in place instead of fresh ones — a caller's own buffers). `device_outputs` = dict of raw device pointers
        {"radiance": ptr, ["albedo", "visibility", "depth", "prev_uv", "ray_count"]} renders in place on the
        GPU without synchronising. packed_tiles: "radiance" holds only this shard's tiles in slot order
        (shard_slot_count() float4 entries) — the form ranks exchange, see assemble_tiles. With half_color_precision the
        colour arrays (radiance, albedo, debug) are np.float16 (device buffers: 8 bytes per pixel)."""
        if self._scene is None:
            raise StratumHipError("BDPT.render before BDPT.update(scene)")
        pc = self.push_constants(frame)
        if self._scene.volumes:  # gViewMediumInstances, BDPT.cpp:456-466
            frame.view_medium_instances = self._scene.view_medium_instances(frame.view_transforms)
        fd = frame.desc()
        o = wire.Outputs()
        out = None
        o.radiance_layout = wire.LAYOUT_SHARD_TILES if packed_tiles else wire.LAYOUT_IMAGE
        if device_outputs is not None:
            o.device_ptrs = 1
            o.gRadiance = device_outputs["radiance"]
            o.gAlbedo = device_outputs.get("albedo")
            o.gVisibility = device_outputs.get("visibility")
            o.gDepth = device_outputs.get("depth")
            o.gPrevUVs = device_outputs.get("prev_uv")
            o.gRayCount = device_outputs.get("ray_count")
            if debug_mode:
                o.debug_mode = debug_mode
                o.gDebugImage = device_outputs["debug"]
        else:
            W, H = frame.width, frame.height
            cd = self.color_dtype
            cb = 4 * np.dtype(cd).itemsize  # bytes of one colour pixel
            if host_outputs is None:
                out = {"radiance": np.zeros((self.shard_slot_count(frame), 4) if packed_tiles else (H, W, 4), cd), "ray_count": np.zeros(2, np.uint64)}
            else:
                out = {k: host_outputs[k] for k in ("radiance", "ray_count")}
                if out["radiance"].nbytes != (self.shard_slot_count(frame) if packed_tiles else H * W) * cb or out["radiance"].dtype != cd or not out["radiance"].flags["C_CONTIGUOUS"]:
                    raise ValueError("host_outputs['radiance'] does not fit the frame")
            o.device_ptrs = 0
            o.gRadiance = wire.ptr(out["radiance"])
            o.gRayCount = wire.ptr(out["ray_count"])
            if debug_mode:  # BDPTDebugMode -> gDebugImage (in / out: a copy of what the caller passes, or zeros)
                out["debug"] = np.ascontiguousarray(debug_image).astype(cd) if debug_image is not None else np.zeros((H, W, 4), cd)
                o.debug_mode = debug_mode
                o.gDebugImage = wire.ptr(out["debug"])
            if aovs and host_outputs is not None:
                for k, dtype, per_pixel in (("albedo", cd, cb), ("visibility", wire.VisibilityInfo, None), ("depth", wire.DepthInfo, None), ("prev_uv", np.float32, 8)):
                    a = host_outputs[k]
                    if a.dtype != dtype or a.nbytes != H * W * (per_pixel or a.dtype.itemsize) or not a.flags["C_CONTIGUOUS"]:
                        raise ValueError("host_outputs[%r] does not fit the frame" % k)
                    out[k] = a
            elif aovs:
                out["albedo"] = np.zeros((H, W, 4), cd)
                out["visibility"] = np.zeros((H, W), wire.VisibilityInfo)
                out["depth"] = np.zeros((H, W), wire.DepthInfo)
                out["prev_uv"] = np.zeros((H, W, 2), np.float32)
            if aovs:
                o.gAlbedo = wire.ptr(out["albedo"])
                o.gVisibility = wire.ptr(out["visibility"])
                o.gDepth = wire.ptr(out["depth"])
                o.gPrevUVs = wire.ptr(out["prev_uv"])
        rc = self._lib.sthip_render(self._h, C.byref(pc), self.mSamplingFlags, self._scene.scene_flags, C.byref(fd), seed_begin, seed_count, C.byref(o))
        self._check(rc, "sthip_render")
        if out is not None:
            self._prev_result = out["radiance"]
        return out

    # ---- pipelined host outputs (include/sthip.h: sthip_render_async) ----
    def _host_output_spec(self, frame, aovs, packed_tiles):
        """(key, shape, dtype) of the host arrays render() would make for this frame."""
        W, H = frame.width, frame.height
        cd = self.color_dtype
        spec = [("radiance", (self.shard_slot_count(frame), 4) if packed_tiles else (H, W, 4), cd)]
        if aovs:
            spec += [("albedo", (H, W, 4), cd), ("visibility", (H, W), wire.VisibilityInfo), ("depth", (H, W), wire.DepthInfo), ("prev_uv", (H, W, 2), np.float32)]
        return spec + [("ray_count", (2,), np.uint64)]

    def alloc_host_outputs(self, frame, aovs=True, packed_tiles=False):
        """The dict of arrays render() returns for this frame, over pinned memory of sthip_host_alloc (the kind a device-to-host
        copy overlaps the next frame with), zero-filled; colour images in color_dtype. The memory is freed in close(): the
        arrays must not be used after it."""
        if not getattr(self, "_h", None):
            raise StratumHipError("BDPT.alloc_host_outputs on a closed renderer")
        out = {}
        for key, shape, dtype in self._host_output_spec(frame, aovs, packed_tiles):
            nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
            ptr = C.c_void_p()
            self._check(self._lib.sthip_host_alloc(self._h, max(1, nbytes), C.byref(ptr)), "sthip_host_alloc")
            self.__dict__.setdefault("_host_blocks", []).append(ptr.value)
            buf = (C.c_uint8 * nbytes).from_address(ptr.value)
            out[key] = np.frombuffer(buf, dtype=dtype).reshape(shape)
            out[key][...] = np.zeros((), dtype)
        return out

    def render_async(self, frame, seed_begin=0, seed_count=1, host_outputs=None, aovs=True, packed_tiles=False):
        """render() with host outputs, but only enqueued: returns a ticket for wait() / ready(). `host_outputs`: a dict from
        alloc_host_outputs (pinned: the copy overlaps the next frame) or of any C-contiguous numpy arrays of the right shapes
        (pageable: correct, but the submit may block); None = fresh pinned arrays. The arrays and the descriptors of a ticket
        are kept alive here until it has been waited for."""
        if self._scene is None:
            raise StratumHipError("BDPT.render_async before BDPT.update(scene)")
        if host_outputs is None:
            host_outputs = self.alloc_host_outputs(frame, aovs=aovs, packed_tiles=packed_tiles)
        out = {}
        for key, shape, dtype in self._host_output_spec(frame, aovs, packed_tiles):
            a = host_outputs[key]
            if a.dtype != dtype or a.nbytes != int(np.prod(shape)) * np.dtype(dtype).itemsize or not a.flags["C_CONTIGUOUS"]:
                raise ValueError("host_outputs[%r] does not fit the frame" % key)
            out[key] = a
        pc = self.push_constants(frame)
        if self._scene.volumes:  # gViewMediumInstances, BDPT.cpp:456-466
            frame.view_medium_instances = self._scene.view_medium_instances(frame.view_transforms)
        fd = frame.desc()
        o = wire.Outputs()
        o.device_ptrs = 0
        o.radiance_layout = wire.LAYOUT_SHARD_TILES if packed_tiles else wire.LAYOUT_IMAGE
        o.gRadiance = wire.ptr(out["radiance"])
        o.gRayCount = wire.ptr(out["ray_count"])
        if aovs:
            o.gAlbedo = wire.ptr(out["albedo"])
            o.gVisibility = wire.ptr(out["visibility"])
            o.gDepth = wire.ptr(out["depth"])
            o.gPrevUVs = wire.ptr(out["prev_uv"])
        ticket = C.c_uint64(0)
        rc = self._lib.sthip_render_async(self._h, C.byref(pc), self.mSamplingFlags, self._scene.scene_flags, C.byref(fd), seed_begin, seed_count, C.byref(o), C.byref(ticket))
        self._check(rc, "sthip_render_async")
        self.__dict__.setdefault("_tickets", {})[ticket.value] = (out, o, fd, pc)
        return ticket.value

    def ready(self, ticket):
        """Whether the outputs of `ticket` are in host memory; never blocks."""
        rc = self._lib.sthip_outputs_ready(self._h, int(ticket))
        if rc < 0:
            self._check(rc, "sthip_outputs_ready")
        return rc == 1

    def wait(self, ticket):
        """Blocks until the outputs of `ticket` (and of every earlier one) are in host memory; returns its dict of arrays
        (None for a ticket already collected)."""
        self._check(self._lib.sthip_wait_outputs(self._h, int(ticket)), "sthip_wait_outputs")
        kept = getattr(self, "_tickets", {}).pop(int(ticket), None)
        if kept is None:
            return None
        self._prev_result = kept[0]["radiance"]
        return kept[0]

    # ---- multi-GPU assembly (include/sthip.h: sthip_shard_slot_count / sthip_assemble_tiles) ----
    def set_shard(self, rank, count, tile_w=64, tile_h=32):
        self._check(self._lib.sthip_set_shard(self._h, rank, count, tile_w, tile_h), "sthip_set_shard")
        self._shard = (rank, count, tile_w, tile_h)

    def shard_slot_count(self, frame, rank=None):
        r, n, tw, th = getattr(self, "_shard", (0, 1, 64, 32))
        return int(self._lib.sthip_shard_slot_count(frame.width, frame.height, r if rank is None else rank, n, tw, th))

    def assemble_tiles(self, frame, packed_ptr, rank_stride, frame_ptr):
        """packed_ptr: device buffer with rank r's tiles at r * rank_stride float4 entries; frame_ptr: W x H RGBA32F (with
        half_color_precision: 8-byte RGBA16F entries and image)."""
        _, n, tw, th = getattr(self, "_shard", (0, 1, 64, 32))
        self._check(self._lib.sthip_assemble_tiles(self._h, packed_ptr, rank_stride, n, tw, th, frame.width, frame.height, frame_ptr), "sthip_assemble_tiles")

    def radiance_to_sums(self, image_ptr, entries, back=False):
        """(mean over the seeds, their number) -> (sum, number) in place, or back: what the seed-split replica mode reduces
        (device pointer; include/sthip.h: sthip_radiance_to_sums). Refused (StratumHipError) with half_color_precision."""
        self._check(self._lib.sthip_radiance_to_sums(self._h, image_ptr, entries, 1 if back else 0), "sthip_radiance_to_sums")

    def pack_tiles(self, frame, image_ptr, entry_bytes, packed_ptr):
        """This shard's tiles of a W x H image of entry_bytes per pixel (a G-buffer output of render) in slot order: what the
        ranks exchange (device pointers; include/sthip.h: sthip_pack_tiles)."""
        self._check(self._lib.sthip_pack_tiles(self._h, image_ptr, frame.width, frame.height, entry_bytes, packed_ptr), "sthip_pack_tiles")

    def assemble_tiles_bytes(self, frame, packed_ptr, rank_stride, frame_ptr, entry_bytes):
        """assemble_tiles for entries of entry_bytes (albedo / depth 16, visibility / prev-uv 8)."""
        n, tw, th = self._shard[1], self._shard[2], self._shard[3]
        self._check(self._lib.sthip_assemble_tiles_bytes(self._h, packed_ptr, rank_stride, n, tw, th, frame.width, frame.height, entry_bytes, frame_ptr), "sthip_assemble_tiles_bytes")

    def prev_result(self):  # BDPT.hpp:18
        return self._prev_result

    # ---- the traversal contract on its own ----
    def trace(self, rays, any_hit=False, alpha_test=False, flip_uvs=False):
        rays = np.ascontiguousarray(rays, dtype=wire.Ray)
        hits = np.zeros(rays.shape[0], wire.Hit)
        mode = (1 if any_hit else 0) | (2 if alpha_test else 0) | (4 if flip_uvs else 0)
        rc = self._lib.sthip_trace_rays(self._h, wire.ptr(rays), rays.shape[0], wire.ptr(hits), mode, 0)
        self._check(rc, "sthip_trace_rays")
        return hits

    # ---- the reuse hash grid on its own ----
    def build_hash_grid(self, bucket_count, keys=None, slots=None, records=None, lvc=False):
        """sthip_build_hash_grid (include/sthip.h): the reuse grid's device build on its own, read back. Keys form: `keys`, a
        (count, 2) uint32 array of (home bucket, checksum) pairs, with `slots` >= count (default: max(count, 1)). Records form:
        `records`, a (slots, 4, 4) float32 array of NEE append records or, with `lvc`, (slots, 6, 4) of LVC append records,
        holes included. Returns a dict: checksums / counters / indices (bucket_count + 32 words), dest (count words), count,
        special_cells, serial_rebuild, dropped, and for records also keys (count, 2) and data (slots, 3 or 5, 4) float32.
        Drops the grids kept for the next render."""
        if not hasattr(self._lib, "sthip_build_hash_grid"):
            raise StratumHipError("this libstratum_hip.so has no sthip_build_hash_grid")
        d, info = wire.HashGridDesc(), wire.HashGridInfo()
        d.struct_size, d.bucket_count = C.sizeof(wire.HashGridDesc), int(bucket_count)
        buckets = int(bucket_count) + 32
        table = [np.full(max(buckets, 1), 0xA5A5A5A5, np.uint32) for _ in range(3)]
        d.checksums, d.counters, d.indices = (t.ctypes.data for t in table)
        if records is None:
            keys = np.ascontiguousarray(np.zeros((0, 2), np.uint32) if keys is None else keys, dtype=np.uint32).reshape(-1, 2)
            d.form, d.count = 0, keys.shape[0]
            d.slots = max(keys.shape[0], 1) if slots is None else int(slots)
            d.keys = keys.ctypes.data if keys.shape[0] else None
            dest = np.full(max(keys.shape[0], 1), 0xA5A5A5A5, np.uint32)
            out_keys = data = None
        else:
            rec, out_rec = (6, 5) if lvc else (4, 3)
            records = np.ascontiguousarray(records, dtype=np.float32)
            if records.ndim != 3 or records.shape[1:] != (rec, 4) or not records.shape[0]:
                raise ValueError("build_hash_grid: records must be a (slots, %d, 4) float32 array" % rec)
            d.form, d.slots, d.records = (2 if lvc else 1), records.shape[0], records.ctypes.data
            dest = np.full(records.shape[0], 0xA5A5A5A5, np.uint32)
            out_keys = np.full((records.shape[0], 2), 0xA5A5A5A5, np.uint32)
            data = np.full((records.shape[0], out_rec, 4), np.float32(-7.0))
            d.compacted_keys, d.data = out_keys.ctypes.data, data.ctypes.data
        d.dest = dest.ctypes.data
        self._check(self._lib.sthip_build_hash_grid(self._h, C.byref(d), C.byref(info)), "sthip_build_hash_grid")
        out = {"checksums": table[0][:buckets], "counters": table[1][:buckets], "indices": table[2][:buckets], "dest": dest[: info.count], "count": int(info.count),
               "special_cells": int(info.special_cells), "serial_rebuild": int(info.serial_rebuild), "dropped": int(info.dropped)}
        if records is not None:
            out["keys"], out["data"] = out_keys[: info.count], data
        return out
