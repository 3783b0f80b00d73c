"""Wire structs of the boundary as numpy dtypes and ctypes structures.

Mirrors include/sthip_wire.h and include/sthip.h field for field (which in turn
restate src/Shaders/{scene,bdpt,transform,shading_data}.h of the reference).
"""
import ctypes as C

import numpy as np

# ---- numpy dtypes (array payloads) --------------------------------------------------------
InstanceData = np.dtype([("packed", "<u4", (4,))])
PackedVertexData = np.dtype([("position", "<f4", (3,)), ("u", "<f4"), ("normal", "<f4", (3,)), ("v", "<f4")])
TransformData = np.dtype([("m", "<f4", (3, 4))])
VertexWeight = np.dtype([("weights", "<f4", (4,)), ("indices", "<u4", (4,))])  # sthip_VertexWeight (kernels/anim.hlsl:6-9)
ProjectionData = np.dtype(
    [
        ("scale", "<f4", (2,)),
        ("offset", "<f4", (2,)),
        ("near_plane", "<f4"),
        ("far_plane", "<f4"),
        ("sensor_area", "<f4"),
        ("vertical_fov", "<f4"),
    ]
)
ViewData = np.dtype([("projection", ProjectionData), ("image_min", "<i4", (2,)), ("image_max", "<i4", (2,))])
VisibilityInfo = np.dtype([("instance_primitive_index", "<u4"), ("packed_normal", "<u4")])
DepthInfo = np.dtype([("z", "<f4"), ("prev_z", "<f4"), ("dz_dxy", "<f4", (2,))])
ShadingData = np.dtype(
    [
        ("position", "<f4", (3,)),
        ("flags", "<u4"),
        ("packed_geometry_normal", "<u4"),
        ("packed_shading_normal", "<u4"),
        ("packed_tangent", "<u4"),
        ("shape_area", "<f4"),
        ("uv", "<f4", (2,)),
        ("uv_screen_size", "<f4"),
        ("mean_curvature", "<f4"),
    ]
)
ImageValue4 = np.dtype([("value", "<f4", (4,)), ("image_index", "<u4")])
MaterialRecord = np.dtype(
    [("values", ImageValue4, (3,)), ("alpha_mask_index", "<u4"), ("bump_index", "<u4"), ("bump_strength", "<f4")]
)
Ray = np.dtype([("origin", "<f4", (3,)), ("tmin", "<f4"), ("direction", "<f4", (3,)), ("tmax", "<f4")])
Hit = np.dtype([("t", "<f4"), ("b1", "<f4"), ("b2", "<f4"), ("instance_primitive_index", "<u4")])

assert InstanceData.itemsize == 16 and PackedVertexData.itemsize == 32 and TransformData.itemsize == 48 and VertexWeight.itemsize == 32
assert ViewData.itemsize == 48 and VisibilityInfo.itemsize == 8 and DepthInfo.itemsize == 16
assert ShadingData.itemsize == 48 and MaterialRecord.itemsize == 72 and Ray.itemsize == 32 and Hit.itemsize == 16

# ---- BDPTFlagBits (bdpt.h:12-40) ----------------------------------------------------------
FLAG_NAMES = [
    "ePerformanceCounters",
    "eRemapThreads",
    "eCoherentRR",
    "eCoherentSampling",
    "eFlipTriangleUVs",
    "eFlipNormalMaps",
    "eAlphaTest",
    "eNormalMaps",
    "eShadingNormalShadowFix",
    "eRayCones",
    "eSampleBSDFs",
    "eNEE",
    "eNEEReservoirs",
    "eNEEReservoirReuse",
    "eMIS",
    "eSampleLightPower",
    "eUniformSphereSampling",
    "ePresampleLights",
    "eDeferShadowRays",
    "eConnectToViews",
    "eConnectToLightPaths",
    "eLVC",
    "eLVCReservoirs",
    "eLVCReservoirReuse",
    "eHashGridJitter",
    "eSampleEnvironmentMapDirectly",
]
FLAG = {n: i for i, n in enumerate(FLAG_NAMES)}

BDPT_FLAG_HAS_ENVIRONMENT = 1
BDPT_FLAG_HAS_EMISSIVES = 2
BDPT_FLAG_HAS_MEDIA = 4
BDPT_FLAG_TRACE_LIGHT = 8

INSTANCE_TYPE_TRIANGLES, INSTANCE_TYPE_SPHERE, INSTANCE_TYPE_VOLUME = 0, 1, 2
LAYOUT_IMAGE, LAYOUT_SHARD_TILES = 0, 1
INVALID_INSTANCE = 0xFFFF
MISS = 0xFFFFFFFF


def flag_mask(*names):
    m = 0
    for n in names:
        m |= 1 << FLAG[n]
    return m


# default sampling flags of the reference renderer (BDPT.cpp:55-62)
DEFAULT_SAMPLING_FLAGS = flag_mask(
    "eRemapThreads", "eRayCones", "eSampleBSDFs", "eCoherentRR", "eNormalMaps", "eNEE", "eMIS", "eDeferShadowRays"
)


# ---- ctypes structures (call descriptors) -------------------------------------------------
class BDPTPushConstants(C.Structure):
    _pack_ = 1
    _fields_ = [
        ("gOutputExtent", C.c_uint32 * 2),
        ("gViewCount", C.c_uint32),
        ("gLightCount", C.c_uint32),
        ("gLightDistributionPDF", C.c_uint32),
        ("gLightDistributionCDF", C.c_uint32),
        ("gEnvironmentMaterialAddress", C.c_uint32),
        ("gEnvironmentSampleProbability", C.c_float),
        ("gRandomSeed", C.c_uint32),
        ("gMinPathVertices", C.c_uint32),
        ("gMaxPathVertices", C.c_uint32),
        ("gMaxDiffuseVertices", C.c_uint32),
        ("gMaxNullCollisions", C.c_uint32),
        ("gLightPresampleTileSize", C.c_uint32),
        ("gLightPresampleTileCount", C.c_uint32),
        ("gLightPathCount", C.c_uint32),
        ("gReservoirM", C.c_uint32),
        ("gReservoirMaxM", C.c_uint32),
        ("gReservoirSpatialM", C.c_uint32),
        ("gHashGridBucketCount", C.c_uint32),
        ("gHashGridMinBucketRadius", C.c_float),
        ("gHashGridBucketPixelRadius", C.c_float),
        ("gDebugViewPathLength", C.c_uint32),
        ("gDebugLightPathLength", C.c_uint32),
    ]


assert C.sizeof(BDPTPushConstants) == 96


class SceneDesc(C.Structure):
    _fields_ = [
        ("gVertices", C.c_void_p),
        ("vertex_count", C.c_uint32),
        ("gIndices", C.c_void_p),
        ("indices_bytes", C.c_uint32),
        ("gInstances", C.c_void_p),
        ("instance_count", C.c_uint32),
        ("gInstanceTransforms", C.c_void_p),
        ("gInstanceInverseTransforms", C.c_void_p),
        ("gInstanceMotionTransforms", C.c_void_p),
        ("gMaterialData", C.c_void_p),
        ("material_bytes", C.c_uint32),
        ("gLightInstances", C.c_void_p),
        ("light_count", C.c_uint32),
        ("gImages", C.c_void_p),
        ("image_count", C.c_uint32),
        ("gDistributions", C.c_void_p),
        ("distribution_count", C.c_uint32),
        ("gImage1s", C.c_void_p),
        ("image1_count", C.c_uint32),
        ("gVolumes", C.c_void_p),
        ("volume_count", C.c_uint32),
    ]


class VolumeDesc(C.Structure):
    _fields_ = [("data", C.c_void_p), ("bytes", C.c_uint64)]


class ImageDesc(C.Structure):
    _fields_ = [("pixels", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32)]


# sthip_image_format (include/sthip.h): the resident texel format of an image, per image (sthip_scene_upload_formats)
IMAGE_FORMAT_RGBA32F = 0
IMAGE_FORMAT_RGBA8_UNORM = 1  # gImages: width * height * 4 bytes; a byte b decodes to float32(b) / float32(255)
IMAGE_FORMAT_R32F = 0
IMAGE_FORMAT_R8_UNORM = 1  # gImage1s: width * height bytes
MAX_MIPS = 16  # levels of a mip chain at most (STHIP_MAX_MIPS)


class FrameDesc(C.Structure):
    _fields_ = [
        ("gViews", C.c_void_p),
        ("gViewTransforms", C.c_void_p),
        ("gInverseViewTransforms", C.c_void_p),
        ("gPrevViews", C.c_void_p),
        ("gPrevInverseViewTransforms", C.c_void_p),
        ("view_count", C.c_uint32),
        ("gViewMediumInstances", C.c_void_p),
    ]


class Outputs(C.Structure):
    _fields_ = [
        ("device_ptrs", C.c_uint32),
        ("radiance_layout", C.c_uint32),  # LAYOUT_IMAGE / LAYOUT_SHARD_TILES
        ("gRadiance", C.c_void_p),
        ("gAlbedo", C.c_void_p),
        ("gVisibility", C.c_void_p),
        ("gDepth", C.c_void_p),
        ("gPrevUVs", C.c_void_p),
        ("gRayCount", C.c_void_p),
        ("debug_mode", C.c_uint32),  # BDPTDebugMode (DEBUG_*), with gDebugImage (RGBA32F, in / out)
        ("gDebugImage", C.c_void_p),
    ]


# BDPTDebugMode, bdpt.h:177-193 (include/sthip.h: STHIP_DEBUG_*)
(DEBUG_NONE, DEBUG_ALBEDO, DEBUG_SPECULAR, DEBUG_EMISSION, DEBUG_SHADING_NORMAL, DEBUG_GEOMETRY_NORMAL, DEBUG_DIR_OUT, DEBUG_PREV_UV, DEBUG_ENVIRONMENT_SAMPLE_TEST,
 DEBUG_ENVIRONMENT_SAMPLE_PDF, DEBUG_RESERVOIR_WEIGHT, DEBUG_PATH_LENGTH_CONTRIBUTION, DEBUG_LIGHT_TRACE_CONTRIBUTION, DEBUG_VIEW_TRACE_CONTRIBUTION, DEBUG_MODE_COUNT) = range(15)


class Stats(C.Structure):
    _fields_ = [
        ("rays_total", C.c_uint64),
        ("rays_path", C.c_uint64),
        ("rays_shadow", C.c_uint64),
        ("nodes_visited", C.c_uint64),
        ("tris_tested", C.c_uint64),
        ("nodes_visited_shadow", C.c_uint64),
        ("tris_tested_shadow", C.c_uint64),
        ("ms_trace", C.c_float),
        ("ms_shade", C.c_float),
        ("ms_total", C.c_float),
        ("launches_trace", C.c_uint32),
        ("bvh_node_bytes", C.c_uint32),
        ("bvh_tri_bytes", C.c_uint32),
        ("bvh_nodes", C.c_uint64),
        ("bvh_tris", C.c_uint64),
        ("bvh_build_ms", C.c_float),
        ("bvh_build_gpu_ms", C.c_float),
        ("inner_slots", C.c_uint64 * 2),
        ("tri_slots", C.c_uint64 * 2),
        ("round_slots", C.c_uint64 * 2),
        ("busy_rounds", C.c_uint64 * 2),
        ("rays_primary_packets", C.c_uint64),
        ("nodes_visited_primary", C.c_uint64),
        ("tris_tested_primary", C.c_uint64),
        ("ms_trace_primary", C.c_float),
        ("launches_primary", C.c_uint32),
        ("lane_states", C.c_uint64 * 8),
        ("rays_answered", C.c_uint64),
        ("paths_per_seed", C.c_uint32),
        ("seeds_in_flight", C.c_uint32),
        ("max_paths_in_flight", C.c_uint64),
        ("batch_halvings", C.c_uint32),
        ("full_rebuilds", C.c_uint32),
        ("leaf_records", C.c_uint32),
        ("reserved0", C.c_uint32),
    ]


class RefitInfo(C.Structure):  # sthip_refit_info
    _fields_ = [
        ("device_ms", C.c_float),
        ("total_ms", C.c_float),
        ("sah_cost", C.c_float),
        ("sah_cost_at_build", C.c_float),
        ("rebuilt", C.c_uint32),
        ("pad", C.c_uint32),
    ]


REFIT_INFO_BYTES = 24  # sizeof(sthip_refit_info), include/sthip.h
assert C.sizeof(RefitInfo) == REFIT_INFO_BYTES


class RigDesc(C.Structure):  # sthip_rig_desc
    _fields_ = [
        ("first_vertex", C.c_uint32),
        ("vertex_count", C.c_uint32),
        ("blend_target_count", C.c_uint32),
        ("bone_count", C.c_uint32),
        ("blend_targets", C.c_void_p * 4),
        ("weights", C.c_void_p),
    ]


class RigPose(C.Structure):  # sthip_rig_pose
    _fields_ = [("blend_factors", C.c_float * 4), ("bones", C.c_void_p)]


RIG_DESC_BYTES, RIG_POSE_BYTES, VERTEX_WEIGHT_BYTES = 56, 24, 32  # sizeof of the C structs, include/sthip.h and sthip_wire.h
assert C.sizeof(RigDesc) == RIG_DESC_BYTES and C.sizeof(RigPose) == RIG_POSE_BYTES


class VertexStreams(C.Structure):  # sthip_vertex_streams
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("first_vertex", C.c_uint32),
        ("vertex_count", C.c_uint32),
        ("device_ptr", C.c_uint32),
        ("recompute_normals", C.c_uint32),
        ("position_stride", C.c_uint32),
        ("normal_stride", C.c_uint32),
        ("texcoord_stride", C.c_uint32),
        ("positions", C.c_void_p),
        ("normals", C.c_void_p),
        ("texcoords", C.c_void_p),
    ]


VERTEX_STREAMS_BYTES = 56  # sizeof(sthip_vertex_streams), include/sthip.h
assert C.sizeof(VertexStreams) == VERTEX_STREAMS_BYTES


def ptr(a):
    """void* of a C-contiguous numpy array (None -> NULL)."""
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.c_void_p)


def default_push_constants(width, height, light_count, view_count=1):
    """Defaults of the reference renderer (BDPT.cpp:63-76) plus the per-frame fields BDPT::render
    fills in (BDPT.cpp:469-503): no environment, no media."""
    pc = BDPTPushConstants()
    pc.gOutputExtent[0], pc.gOutputExtent[1] = width, height
    pc.gViewCount = view_count
    pc.gLightCount = light_count
    pc.gLightDistributionPDF = 0
    pc.gLightDistributionCDF = 0
    pc.gEnvironmentMaterialAddress = 0xFFFFFFFF
    pc.gEnvironmentSampleProbability = 0.5  # BDPT.cpp:67; BDPT::render forces 0 / 1 without an environment / without emitters (:488-496)
    pc.gRandomSeed = 0
    pc.gMinPathVertices = 4
    pc.gMaxPathVertices = 8
    pc.gMaxDiffuseVertices = 2
    pc.gMaxNullCollisions = 64  # BDPT.cpp:62; BDPT::render zeroes it for scenes without media (:497-500)
    pc.gLightPresampleTileSize = 1024
    pc.gLightPresampleTileCount = 128
    pc.gLightPathCount = width * height
    pc.gReservoirM = 16
    pc.gReservoirMaxM = 64
    pc.gReservoirSpatialM = 4
    pc.gHashGridBucketCount = 200000
    pc.gHashGridMinBucketRadius = 0.1
    pc.gHashGridBucketPixelRadius = 6
    return pc


# ---- after the path (include/sthip.h, "display transform, image metric, HDR export") ----
TONEMAP_MODES = [  # TonemapMode, tonemap.h:8-21
    "Raw",
    "Reinhard",
    "ReinhardExtended",
    "ReinhardLuminance",
    "ReinhardLuminanceExtended",
    "Uncharted2",
    "Filmic",
    "ACES",
    "ACESApprox",
    "ViridisR",
    "ViridisLengthRGB",
]
TONEMAP = {n: i for i, n in enumerate(TONEMAP_MODES)}
COMPARE_MODES = ["SMAPE", "MSE", "Average"]  # ImageCompareMode, image_compare.hlsl:5-9
COMPARE = {n: i for i, n in enumerate(COMPARE_MODES)}


class TonemapDesc(C.Structure):
    _fields_ = [
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("mode", C.c_uint32),
        ("modulate_albedo", C.c_uint32),
        ("gamma_correction", C.c_uint32),
        ("exposure", C.c_float),
        ("device_ptrs", C.c_uint32),
        ("exposure_alpha", C.c_float),
        ("gInput", C.c_void_p),
        ("gAlbedo", C.c_void_p),
        ("gOutput", C.c_void_p),
        ("out_max", C.c_void_p),
        ("exposure_state", C.c_void_p),
    ]


class AccumulateDesc(C.Structure):
    _fields_ = [
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("view_count", C.c_uint32),
        ("reprojection", C.c_uint32),
        ("demodulate_albedo", C.c_uint32),
        ("history_limit", C.c_float),
        ("device_ptrs", C.c_uint32),
        ("instance_count", C.c_uint32),
        ("gViews", C.c_void_p),
        ("gRadiance", C.c_void_p),
        ("gAlbedo", C.c_void_p),
        ("gVisibility", C.c_void_p),
        ("gDepth", C.c_void_p),
        ("gPrevUVs", C.c_void_p),
        ("gPrevVisibility", C.c_void_p),
        ("gPrevDepth", C.c_void_p),
        ("gPrevAccumColor", C.c_void_p),
        ("gPrevAccumMoments", C.c_void_p),
        ("gInstanceIndexMap", C.c_void_p),
        ("gAccumColor", C.c_void_p),
        ("gAccumMoments", C.c_void_p),
    ]



FILTER_TYPES = ["Atrous", "Box3", "Box5", "Subsampled", "Box3Subsampled", "Box5Subsampled"]  # FilterKernelType, filter_type.h:8-16
FILTER = {n: i for i, n in enumerate(FILTER_TYPES)}


class DenoiseDesc(C.Structure):
    _fields_ = [
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("view_count", C.c_uint32),
        ("device_ptrs", C.c_uint32),
        ("instance_count", C.c_uint32),
        ("iterations", C.c_uint32),
        ("filter_type", C.c_uint32),
        ("history_tap", C.c_uint32),
        ("history_limit", C.c_float),
        ("variance_boost_length", C.c_float),
        ("sigma_luminance_boost", C.c_float),
        ("pad_", C.c_uint32),
        ("gViews", C.c_void_p),
        ("gVisibility", C.c_void_p),
        ("gDepth", C.c_void_p),
        ("gInstanceIndexMap", C.c_void_p),
        ("gAccumColor", C.c_void_p),
        ("gAccumMoments", C.c_void_p),
        ("gFilterImages", C.c_void_p * 2),
        ("pass_ms", C.c_void_p),
    ]


# sthip_convert_material (include/sthip.h): the four kernels of kernels/material_convert.hlsl
CONVERT_KINDS = ["GltfPbr", "DiffuseSpecular", "AlphaToRoughness", "ShininessToRoughness"]  # STHIP_CONVERT_*
CONVERT = {n: i for i, n in enumerate(CONVERT_KINDS)}


# sthip_texel_format (include/sthip.h): the formats an asset's images come in, decoded on the way in
TEXEL_FORMATS = {"RGBA32F": 0, "RGBA8_UNORM": 1}
for _c, _class in enumerate(("8_UNORM", "8_SRGB", "16_UNORM", "32F")):
    for _n, _channels in enumerate(("R", "RG", "RGB", "RGBA")):
        if _channels + _class not in TEXEL_FORMATS:  # (RGBA8_UNORM and RGBA32F keep 1 and 0; 19 and 31 name the same texels)
            TEXEL_FORMATS[_channels + _class] = 16 + 4 * _c + _n
TEXEL_FORMATS.update({"BC1_RGB": 32, "BC2": 33, "BC3": 34, "BC4_UNORM": 35, "BC5_UNORM": 36, "BC1_RGB_SRGB": 37, "BC2_SRGB": 38, "BC3_SRGB": 39})
TEXEL_UNSUPPORTED = {"BC4_SNORM": 48, "BC5_SNORM": 49, "BC6H_UFLOAT": 50, "BC6H_SFLOAT": 51, "BC7_UNORM": 52, "BC7_SRGB": 53, "R8_SNORM": 56, "R16_SNORM": 60, "R8_UINT": 64}  # named, refused


def texel_format(f):
    """The number of a sthip_texel_format given by name or number."""
    return TEXEL_FORMATS[f] if isinstance(f, str) else int(f)


def texel_format_info(f):
    """(block bytes or 0, channels, component bytes, sRGB) of a built format: the layout rules of include/sthip.h."""
    f = {0: 31, 1: 19}.get(texel_format(f), texel_format(f))
    if not 16 <= f < 40:
        raise ValueError("%d is no built sthip_texel_format" % f)
    if f >= 32:
        return (8 if f in (32, 35, 37) else 16), {35: 1, 36: 2, 32: 3, 37: 3}.get(f, 4), 0, f >= 37
    cls = (f - 16) >> 2
    return 0, ((f - 16) & 3) + 1, (1, 1, 2, 4)[cls], cls == 1


def texel_image_bytes(f, width, height):
    block, channels, size, _ = texel_format_info(f)
    return ((width + 3) // 4) * ((height + 3) // 4) * block if block else width * height * channels * size


class TexelImage:
    """An image in an asset's own texel format: `data` (any C-contiguous array or bytes of exactly the image's size), a
    sthip_texel_format by name or number, and the extent."""

    def __init__(self, data, format, width, height):
        import numpy as np

        self.format, self.width, self.height = texel_format(format), int(width), int(height)
        self.data = np.ascontiguousarray(np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray)) else data).view(np.uint8).reshape(-1)
        if self.data.size != texel_image_bytes(self.format, self.width, self.height):
            raise ValueError("a %d x %d image of format %d has %d bytes, not %d" % (self.width, self.height, self.format, texel_image_bytes(self.format, self.width, self.height), self.data.size))


class DecodeTexelsDesc(C.Structure):  # sthip_decode_texels_desc
    _fields_ = [
        ("src_format", C.c_uint32),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("device_ptrs", C.c_uint32),
        ("dst_format", C.c_uint32),
        ("dst_channels", C.c_uint32),
        ("channel", C.c_uint32),
        ("pad_", C.c_uint32),
        ("src", C.c_void_p),
        ("dst", C.c_void_p),
    ]


class HashGridDesc(C.Structure):  # sthip_hash_grid_desc
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("form", C.c_uint32),
        ("slots", C.c_uint32),
        ("count", C.c_uint32),
        ("bucket_count", C.c_uint32),
        ("reserved0", C.c_uint32),
        ("keys", C.c_void_p),
        ("records", C.c_void_p),
        ("checksums", C.c_void_p),
        ("counters", C.c_void_p),
        ("indices", C.c_void_p),
        ("dest", C.c_void_p),
        ("compacted_keys", C.c_void_p),
        ("data", C.c_void_p),
    ]


class HashGridInfo(C.Structure):  # sthip_hash_grid_info
    _fields_ = [("count", C.c_uint32), ("special_cells", C.c_uint32), ("serial_rebuild", C.c_uint32), ("dropped", C.c_uint32)]


HASH_GRID_DESC_BYTES = 88  # sizeof(sthip_hash_grid_desc), include/sthip.h
assert C.sizeof(HashGridDesc) == HASH_GRID_DESC_BYTES and C.sizeof(HashGridInfo) == 16


class DenseVolumeDesc(C.Structure):  # sthip_dense_volume_desc
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("dense_is_device", C.c_uint32),
        ("dense", C.c_void_p),
        ("dims", C.c_uint32 * 3),
        ("origin", C.c_int32 * 3),
        ("voxel_size", C.c_double),
        ("translation", C.c_double * 3),
        ("name", C.c_char_p),
    ]


class VolumeInfo(C.Structure):  # sthip_volume_info
    _fields_ = [
        ("bytes", C.c_uint64),
        ("bbox_min", C.c_int32 * 3),
        ("bbox_max", C.c_int32 * 3),
        ("world_bbox", C.c_double * 6),
        ("min", C.c_float),
        ("max", C.c_float),
        ("active_voxels", C.c_uint64),
        ("leaf_count", C.c_uint32),
        ("lower_count", C.c_uint32),
        ("upper_count", C.c_uint32),
        ("root_tiles", C.c_uint32),
        ("device_ms", C.c_float),
        ("call_ms", C.c_float),
    ]


class VolumeSource(C.Structure):  # sthip_volume_source
    _fields_ = [("struct_size", C.c_uint32), ("data_is_device", C.c_uint32), ("data", C.c_void_p), ("bytes", C.c_uint64), ("dense", C.POINTER(DenseVolumeDesc))]


DENSE_VOLUME_DESC_BYTES, VOLUME_INFO_BYTES = 80, 120  # sizeof(sthip_dense_volume_desc), sizeof(sthip_volume_info), include/sthip.h
assert C.sizeof(DenseVolumeDesc) == DENSE_VOLUME_DESC_BYTES and C.sizeof(VolumeInfo) == VOLUME_INFO_BYTES and C.sizeof(VolumeSource) == 32


class EnvironmentDesc(C.Structure):  # sthip_environment_desc
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("material_address", C.c_uint32),
        ("value", C.c_void_p),
        ("pixels", C.c_void_p),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("device_ptr", C.c_uint32),
        ("pad", C.c_uint32),
    ]


class EnvironmentInfo(C.Structure):  # sthip_environment_info
    _fields_ = [("device_ms", C.c_float), ("total_ms", C.c_float)]


ENVIRONMENT_DESC_BYTES = 40  # sizeof(sthip_environment_desc), include/sthip.h
assert C.sizeof(EnvironmentDesc) == ENVIRONMENT_DESC_BYTES


class ImageUpdate(C.Structure):  # sthip_image_update
    _fields_ = [
        ("which", C.c_uint32),
        ("index", C.c_uint32),
        ("pixels", C.c_void_p),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("device_ptr", C.c_uint32),
        ("pad", C.c_uint32),
    ]


class ImagesInfo(C.Structure):  # sthip_images_info
    _fields_ = [
        ("device_ms", C.c_float),
        ("total_ms", C.c_float),
        ("has_specular_before", C.c_uint32),
        ("has_specular_after", C.c_uint32),
        ("images_scanned", C.c_uint32),
        ("pad", C.c_uint32),
    ]


IMAGE_UPDATE_BYTES = 32  # sizeof(sthip_image_update), include/sthip.h
assert C.sizeof(ImageUpdate) == IMAGE_UPDATE_BYTES and C.sizeof(ImagesInfo) == 24


class TransformsDesc(C.Structure):  # sthip_transforms_desc
    _fields_ = [
        ("transforms", C.c_void_p),
        ("inverse_transforms", C.c_void_p),
        ("motion_transforms", C.c_void_p),
        ("instance_count", C.c_uint32),
        ("device_ptr", C.c_uint32),
        ("top_level", C.c_uint32),
        ("derive_motion", C.c_uint32),
    ]


class TransformsInfo(C.Structure):  # sthip_transforms_info
    _fields_ = [
        ("device_ms", C.c_float),
        ("total_ms", C.c_float),
        ("top_level_nodes", C.c_uint32),
        ("top_level_depth", C.c_uint32),
        ("rebuilt", C.c_uint32),
        ("builder_used", C.c_uint32),
    ]


TRANSFORMS_DESC_BYTES = 40  # sizeof(sthip_transforms_desc), include/sthip.h
assert C.sizeof(TransformsDesc) == TRANSFORMS_DESC_BYTES and C.sizeof(TransformsInfo) == 24
# sthip_top_node: the union of a top-level node's two child boxes and its children (a node index, or 0x80000000 | entry)
TopNode = np.dtype([("lo", np.float32, 3), ("child0", np.uint32), ("hi", np.float32, 3), ("child1", np.uint32)])
assert TopNode.itemsize == 32


class ConvertMaterialDesc(C.Structure):
    _fields_ = [
        ("kind", C.c_uint32),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("device_ptrs", C.c_uint32),
        ("output_format", C.c_uint32),
        ("diffuse_format", C.c_uint8),
        ("specular_format", C.c_uint8),
        ("transmittance_format", C.c_uint8),
        ("roughness_format", C.c_uint8),
        ("input_format", C.c_uint8),
        ("pad_", C.c_uint8 * 7),
        ("gDiffuse", C.c_void_p),
        ("gSpecular", C.c_void_p),
        ("gTransmittance", C.c_void_p),
        ("gRoughness", C.c_void_p),
        ("gInput", C.c_void_p),
        ("gOutput", C.c_void_p * 3),
        ("gOutputAlphaMask", C.c_void_p),
        ("gOutputMinAlpha", C.c_void_p),
        ("gRoughnessRW", C.c_void_p),
    ]
