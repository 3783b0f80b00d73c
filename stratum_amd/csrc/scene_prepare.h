// scene_prepare.h — the host part of sthip_scene_upload that needs neither the built tree nor the device: the argument checks,
// the scan of the materials, and the tables the upload copies to HBM as they are (bvh.h holds their layouts). No HIP, like
// bvh_build.cpp: tests/cpp/scene_prepare_check.cpp runs it on the CPU under ASan / UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/sthip.h"
#include "../../include/sthip_wire.h"
#include "bvh.h"
#include "bvh_build.h"

namespace sthip {

// Every refusal of an upload that can be decided from the arguments alone, in the order the checks have always had. false:
// `code` (sthip_status) and `message` say why, and the caller changes nothing of its context. The image_formats /
// image1_formats arrays are those of sthip_scene_upload_formats (NULL: all 0).
bool check_scene(const sthip_scene_desc* s, const uint8_t* image_formats, const uint8_t* image1_formats, int& code, std::string& message);

// The per-channel extremes of level 0 of one image of gImages (include/sthip.h, "image ranges"): lo / hi over the texels that
// are not NaN; a channel in which a NaN was seen (bit c of nan_mask), or an image without texels, is unknown: -inf / +inf.
// known = 0: nobody has scanned the image; the analysis treats every channel of it as unknown.
struct ImageRange {
  float lo[4] = {0, 0, 0, 0}, hi[4] = {0, 0, 0, 0};
  uint32_t nan_mask = 0;
  uint32_t known = 0;
};

// What the materials of a checked scene say about the kernels it needs, and k_cull_terminal's per-instance table
struct MaterialAnalysis {
  bool has_specular = false;  // some material can satisfy DisneyMaterial::is_specular (or a medium Medium::is_specular)
  bool textured = false;      // some material binds an image of gImages
  bool any_alpha = false;     // some triangle instance's material has an alpha mask
  bool has_spheres = false, has_volumes = false;
  uint32_t volume_instances = 0;
  std::vector<uint8_t> instance_is_volume;  // per instance
  std::vector<uint8_t> inst_flags;          // per instance (at least one entry): INST_FLAG_*
  std::vector<uint8_t> image_in_material;   // per image of gImages: 1 = some instance's material record names it (its texels were scanned above)
  std::vector<ImageRange> image_ranges;      // analyse_materials(s, formats) only: per image of gImages, what its scan found (known = 0: not scanned)
};
MaterialAnalysis analyse_materials(const sthip_scene_desc& s, const uint8_t* image_formats);

// ---- the two halves of analyse_materials (sthip_scene_set_images / sthip_scene_set_material_data run them apart) ----
// The scan on the host (ImageRange, above): `count` texels of RGBA32F, or of RGBA8_UNORM (rgba8; a byte decodes as (float)b / 255.0f)
ImageRange scan_image_range(const void* pixels, size_t count, bool rgba8);
// What the analysis reads of an instance: 8 bytes, kept by the context whatever "keep_scene" says
struct MaterialInstance {
  uint32_t address;  // InstanceData::material_address
  uint32_t type;     // STHIP_INSTANCE_TYPE_*
};
// Which images of gImages the records name (MaterialAnalysis::image_in_material) and which of them the analysis reads the range
// of (an image value whose constant has a positive component): the upload scans the latter on the host.
void material_images(const MaterialInstance* instances, uint32_t instance_count, const uint8_t* materials, uint32_t image_count, std::vector<uint8_t>& named, std::vector<uint8_t>& range_read);
// The rest of the analysis, with the ranges already known (`ranges`: image_count entries). analyse_materials(s, formats) is
// material_images + scan_image_range of the images whose range is read + this.
MaterialAnalysis analyse_materials(const MaterialInstance* instances, uint32_t instance_count, const uint8_t* materials, uint32_t image_count, const ImageRange* ranges);

// ---- sthip_scene_set_images / sthip_scene_set_material_data: what of them needs no device ----
struct ResidentImages {
  bool has_scene = false;
  const DeviceImage* images = nullptr;  // the tables as uploaded
  uint32_t image_count = 0;
  const DeviceImage1* images1 = nullptr;
  uint32_t image1_count = 0;
};
// Every refusal of sthip_scene_set_images (sthip.h), from the arguments and the host-side tables alone. false: `code` and
// `message` say why and the caller changes nothing.
bool check_images(const ResidentImages& scene, const sthip_image_update* entries, uint32_t n, uint32_t struct_size, int& code, std::string& message);

struct ResidentMaterials {
  bool has_scene = false;
  const uint8_t* materials = nullptr;  // gMaterialData as resident
  size_t material_bytes = 0;
  const MaterialInstance* instances = nullptr;
  uint32_t instance_count = 0;
  uint32_t image_count = 0, image1_count = 0, volume_count = 0;
};
// Every refusal of sthip_scene_set_material_data. true: `edited` is gMaterialData as it is after the edit (every instance's
// record in it passes the material checks of check_scene, and nothing the trees or the light tables were built from differs).
bool check_material_data(const ResidentMaterials& scene, uint32_t offset, const void* data, uint32_t bytes, std::vector<uint8_t>& edited, int& code, std::string& message);

// EmitterBounds from the exact box of an emitter's vertices: widened by 2^-15 of its coordinates' magnitude, as the packed nodes
// of the tree are, and the sphere that sizes the per-ray padding. false: not finite (the table cannot be used).
bool pad_emitter_bounds(EmitterBounds& b);
// ---- sthip_scene_set_environment: what of it needs no device ----
// What the context knows of the resident scene, as far as the environment call consults it
struct ResidentEnvironmentScene {
  bool has_scene = false;
  const uint8_t* materials = nullptr;  // gMaterialData as uploaded
  size_t material_bytes = 0;
  const DeviceImage* images = nullptr;  // the image table as uploaded
  uint32_t image_count = 0;
  const uint8_t* image_in_material = nullptr;  // MaterialAnalysis::image_in_material (image_count entries, or NULL: none)
  uint32_t distribution_count = 0;
};
// What an accepted call does
struct EnvironmentPlan {
  bool has_image = false;       // the record binds an image (and names four tables)
  bool replace_pixels = false;  // level 0 from the caller, further levels again
  bool build_tables = false;    // the four tables again
  bool set_value = false;       // the record's three floats
  uint32_t image_index = 0, width = 0, height = 0;
  uint32_t table[4] = {0, 0, 0, 0};  // offsets in gDistributions: marginal_pdf, row_pdf, marginal_cdf, row_cdf
};
// Every refusal of sthip_scene_set_environment (sthip.h), decided from the arguments and the host-side state alone. false:
// `code` and `message` say why and the caller changes nothing.
bool check_environment(const ResidentEnvironmentScene& scene, const sthip_environment_desc* d, EnvironmentPlan& plan, int& code, std::string& message);
// s[y] = sin(M_PI * (y + 0.5f) * (1 / (float)H)) for the H rows of a lat-long image, with libm (sthip.h: the device gets them as they are)
void environment_row_sines(uint32_t height, std::vector<double>& out);

// ---- sthip_scene_set_vertices: what of it needs no device ----
// Every refusal of the call (sthip.h), from the arguments and the resident vertex count alone. false: `code` and `message`
// (which names the field) say why and the caller changes nothing.
bool check_vertex_streams(bool has_scene, uint32_t scene_vertex_count, const sthip_vertex_streams* d, int& code, std::string& message);
// A mesh of the normal contract: the tuple its triangle instances share
struct VertexMesh {
  uint32_t indices_byte_offset, first_vertex, index_stride, prim_count;
};
// The meshes of a scene: the distinct tuples of its triangle instances in ascending order (spheres and volumes have none)
std::vector<VertexMesh> list_vertex_meshes(const sthip_InstanceData* instances, uint32_t instance_count);

// The bounds of the emissive triangle instances (bvh.h: EmitterBounds), from the validated scene arrays: the box of the
// vertices an instance's triangles refer to, widened by 2^-15 of its coordinates' magnitude as the packed nodes of the
// tree are, in world space for an instance with identity transforms (that is where its triangles are tested, whether the
// builder merged it or not: the identity's fmaf chain returns the world-space ray) and in object space otherwise. `out` stays
// empty when the table cannot be used (more than STHIP_MAX_EMITTER_BOUNDS emitters, a box that is not finite). It reads
// gIndices at offsets only build_scene_bvh validates: call it after that has succeeded on the same arrays.
void emitter_bounds(const sthip_scene_desc& s, const std::vector<uint8_t>& inst_flags, std::vector<EmitterBounds>& out);

// gImages as they lie in HBM: the table, the float images' texels with their mip chains (2x2 box filter), and the size of the
// RGBA8 images' array in words (their layout only: level 0 goes up as it is and mips.hip makes the rest)
struct ImageLayout {
  std::vector<DeviceImage> table;
  std::vector<float> texels;
  size_t texels8 = 0;
  const char* error = nullptr;  // set: the RGBA8 images exceed the 32-bit texel offsets (STHIP_ERR_UNSUPPORTED); the rest is not filled
};
ImageLayout layout_images(const sthip_scene_desc& s, const uint8_t* image_formats);

// gImage1s (alpha masks: level 0 only): the table, the R32F texels and the R8 bytes, each array back to back
struct MaskLayout {
  std::vector<DeviceImage1> table;
  std::vector<float> texels;
  std::vector<uint8_t> texels8;
  const char* error = nullptr;  // as ImageLayout::error, for the R8 masks
};
MaskLayout layout_alpha_masks(const sthip_scene_desc& s, const uint8_t* image1_formats);

// gVolumes back to back as 32-bit words: the first word of each grid; returns the words in all
size_t volume_first_words(const sthip_scene_desc& s, std::vector<uint32_t>& out);

}  // namespace sthip
