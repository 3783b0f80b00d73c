// material_convert_ref.cpp — a scalar C++ restatement of kernels/material_convert.hlsl (from_gltf_pbr :46-76,
// from_diffuse_specular :78-108, alpha_to_roughness :28-35, shininess_to_roughness :37-44), written from the shader, statement
// by statement, with the decisions of include/sthip.h (sthip_convert_material). It shares no code with the library or with the
// numpy statement in tests/test_material_convert.py, which it pins bit for bit. Build with -ffp-contract=off.
//   material_convert_ref <in.bin> <out.bin>
// in.bin:  uint32 kind, texels, use (bit 0 gDiffuse, 1 gSpecular, 2 gTransmittance, 3 gRoughness), source_bytes, output_bytes;
//          then every present source in that order (kinds 2, 3: gInput), 4 channels (gRoughness / gInput: 1) per texel,
//          as bytes (source_bytes) or floats.
// out.bin: gOutput[0..2], gOutputAlphaMask (with gDiffuse), uint32 gOutputMinAlpha; kinds 2, 3: gRoughnessRW.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

struct float3 {
  float x, y, z;
};
struct float4 {
  float x, y, z, w;
};
static float saturate(float a) { return a > 0 ? (a < 1 ? a : 1) : 0; }
static float luminance(float3 c) { return (c.x * 0.2126f + c.y * 0.7152f) + c.z * 0.0722f; }
static uint32_t quantise(float v) { return (uint32_t)(saturate(v) * 255.0f + 0.5f); }

struct DisneyMaterialData {  // disney_data.h
  float data[3][4];
  void base_color(float3 v) { data[0][0] = v.x, data[0][1] = v.y, data[0][2] = v.z; }
  float3 base_color() const { return float3{data[0][0], data[0][1], data[0][2]}; }
  void metallic(float v) { data[1][0] = v; }
  void roughness(float v) { data[1][1] = v; }
  void transmission(float v) { data[2][2] = v; }
};

struct Reader {
  std::vector<uint8_t> bytes;
  size_t at = 0;
  uint32_t u32() {
    uint32_t v;
    std::memcpy(&v, bytes.data() + at, 4);
    at += 4;
    return v;
  }
  // `channels` values of texel i of an image that starts at `base`
  float channel(size_t base, bool as_bytes, size_t index) const {
    if (as_bytes) return (float)bytes[base + index] / 255.0f;
    float v;
    std::memcpy(&v, bytes.data() + base + index * 4, 4);
    return v;
  }
};

struct Writer {
  std::vector<uint8_t> bytes;
  bool as_bytes;
  void put(std::vector<uint8_t>& to, float v) const {
    if (as_bytes) {
      to.push_back((uint8_t)quantise(v));
    } else {
      uint8_t b[4];
      std::memcpy(b, &v, 4);
      to.insert(to.end(), b, b + 4);
    }
  }
};

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: material_convert_ref in.bin out.bin\n");
    return 2;
  }
  Reader r;
  {
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return std::fprintf(stderr, "cannot read %s\n", argv[1]), 1;
    uint8_t buf[65536];
    size_t got;
    while ((got = std::fread(buf, 1, sizeof(buf), f)) > 0) r.bytes.insert(r.bytes.end(), buf, buf + got);
    std::fclose(f);
  }
  if (r.bytes.size() < 20) return std::fprintf(stderr, "short header\n"), 1;
  const uint32_t kind = r.u32(), texels = r.u32(), use = r.u32(), source_bytes = r.u32(), output_bytes = r.u32();
  const bool gUseDiffuse = use & 1, gUseSpecular = use & 2, gUseTransmittance = use & 4, gUseRoughness = use & 8;
  const size_t c4 = source_bytes ? 4 : 16, c1 = source_bytes ? 1 : 4;
  Writer w;
  w.as_bytes = output_bytes != 0;
  std::vector<uint8_t> out;
  if (kind >= 2) {
    if (r.bytes.size() != r.at + (size_t)texels * c1) return std::fprintf(stderr, "wrong size\n"), 1;
    for (uint32_t i = 0; i < texels; i++) {
      const float x = r.channel(r.at, source_bytes, i);
      w.put(out, kind == 2 ? saturate(std::sqrt(x)) : saturate(std::sqrt(2 / (x + 2))));
    }
  } else {
    size_t at = r.at;
    const size_t diffuse_at = at;
    at += gUseDiffuse ? texels * c4 : 0;
    const size_t specular_at = at;
    at += gUseSpecular ? texels * c4 : 0;
    const size_t transmittance_at = at;
    at += gUseTransmittance ? texels * c4 : 0;
    const size_t roughness_at = at;
    at += gUseRoughness ? texels * c1 : 0;
    if (r.bytes.size() != at) return std::fprintf(stderr, "wrong size\n"), 1;
    auto fetch4 = [&](size_t base, uint32_t i) { return float4{r.channel(base, source_bytes, 4 * (size_t)i), r.channel(base, source_bytes, 4 * (size_t)i + 1), r.channel(base, source_bytes, 4 * (size_t)i + 2), r.channel(base, source_bytes, 4 * (size_t)i + 3)}; };
    std::vector<uint8_t> o[3], mask;
    uint32_t gOutputMinAlpha = 0xFFFFFFFFu;
    for (uint32_t i = 0; i < texels; i++) {
      DisneyMaterialData m;
      for (int k = 0; k < 3; k++)
        for (int c = 0; c < 4; c++) m.data[k][c] = 1;
      if (kind == 0) {  // from_gltf_pbr
        const float4 diffuse = gUseDiffuse ? fetch4(diffuse_at, i) : float4{1, 1, 1, 1};
        if (gUseDiffuse) {
          w.put(mask, diffuse.w);
          if (diffuse.w < 1) {
            const uint32_t a = (uint32_t)(saturate(diffuse.w) * 4294967296.0f);  // InterlockedMin(.., saturate(a) * 0xFFFFFFFF)
            if (a < gOutputMinAlpha) gOutputMinAlpha = a;
          }
        }
        const float4 metallic_roughness = gUseSpecular ? fetch4(specular_at, i) : float4{1, 1, 1, 1};
        m.base_color(float3{diffuse.x, diffuse.y, diffuse.z});
        m.metallic(metallic_roughness.z);
        m.roughness(metallic_roughness.y);
        const float l = luminance(m.base_color());
        float transmission = 0;
        if (gUseTransmittance) {
          const float4 t = fetch4(transmittance_at, i);
          transmission = saturate(luminance(float3{t.x, t.y, t.z}) / (l > 0 ? l : 1));
        }
        m.transmission(transmission);
      } else {  // from_diffuse_specular
        const float4 diffuse = gUseDiffuse ? fetch4(diffuse_at, i) : float4{0, 0, 0, 0};
        if (gUseDiffuse) {
          w.put(mask, diffuse.w);
          if (diffuse.w < 1) {
            const uint32_t a = (uint32_t)(saturate(diffuse.w) * 4294967296.0f);
            if (a < gOutputMinAlpha) gOutputMinAlpha = a;
          }
        }
        float3 specular{0, 0, 0}, transmittance{0, 0, 0};
        if (gUseSpecular) {
          const float4 s = fetch4(specular_at, i);
          specular = float3{s.x, s.y, s.z};
        }
        if (gUseTransmittance) {
          const float4 t = fetch4(transmittance_at, i);
          transmittance = float3{t.x, t.y, t.z};
        }
        const float ld = luminance(float3{diffuse.x, diffuse.y, diffuse.z});
        const float ls = luminance(specular);
        const float lt = luminance(transmittance);
        const float sum = ls + ld + lt;
        m.base_color(float3{(diffuse.x * ld + specular.x * ls + transmittance.x * lt) / sum, (diffuse.y * ld + specular.y * ls + transmittance.y * lt) / sum,
                            (diffuse.z * ld + specular.z * ls + transmittance.z * lt) / sum});
        if (gUseSpecular) m.metallic(saturate(ls / (ld + ls + lt)));
        if (gUseRoughness) m.roughness(r.channel(roughness_at, source_bytes, i));
        if (gUseTransmittance) m.transmission(saturate(lt / (ld + ls + lt)));
      }
      for (int k = 0; k < 3; k++)
        for (int c = 0; c < 4; c++) w.put(o[k], m.data[k][c]);
    }
    for (int k = 0; k < 3; k++) out.insert(out.end(), o[k].begin(), o[k].end());
    out.insert(out.end(), mask.begin(), mask.end());
    uint8_t b[4];
    std::memcpy(b, &gOutputMinAlpha, 4);
    out.insert(out.end(), b, b + 4);
  }
  FILE* f = std::fopen(argv[2], "wb");
  if (!f) return std::fprintf(stderr, "cannot write %s\n", argv[2]), 1;
  std::fwrite(out.data(), 1, out.size(), f);
  std::fclose(f);
  return 0;
}
