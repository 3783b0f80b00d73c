// texel_decode_host_check.cpp — csrc/texel_decode.h (the text the kernels compile) run on the host: the same interface as
// texel_decode_ref.cpp's `decode` mode, so that the tests compare the two without a GPU, and under the sanitizers.
// Build: g++ -std=c++17 -O2 -ffp-contract=off texel_decode_host_check.cpp
//   texel_decode_host_check IN OUT   IN: uint32 format, width, height, then the image's bytes. OUT: width * height * 4 floats.
#include <stdio.h>

#include <vector>

#include "../../stratum_amd/csrc/texel_decode.h"

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: texel_decode_host_check IN OUT\n");
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 1;
  uint32_t head[3];
  if (fread(head, 4, 3, f) != 3 || !sthip::texel_format_built(head[0]) || !head[1] || !head[2] || (uint64_t)head[1] * head[2] > (1u << 24)) return 1;
  const uint32_t format = sthip::texel_canonical(head[0]), w = head[1], h = head[2];
  // exactly the image's bytes in an allocation of its own (16-byte aligned, as operator new gives): a read beyond it shows
  const size_t bytes = (size_t)sthip::texel_image_bytes(format, w, h);
  uint8_t* image = new uint8_t[bytes];
  if (fread(image, 1, bytes, f) != bytes || fgetc(f) != EOF) return 1;
  fclose(f);
  std::vector<float> out((size_t)w * h * 4);
  for (uint32_t y = 0; y < h; y++)
    for (uint32_t x = 0; x < w; x++) {
      const sthip::Texel4 v = sthip::decode_texel(format, image, w, h, x, y);
      float* o = &out[((size_t)y * w + x) * 4];
      o[0] = v.x, o[1] = v.y, o[2] = v.z, o[3] = v.w;
    }
  delete[] image;
  f = fopen(argv[2], "wb");
  if (!f) return 1;
  const bool ok = fwrite(out.data(), 4, out.size(), f) == out.size();
  return fclose(f) == 0 && ok ? 0 : 1;
}
