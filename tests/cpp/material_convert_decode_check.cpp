// material_convert_decode_check.cpp — sthip::decode_unorm8 (stratum_amd/csrc/material_convert.h), the division-free decode the
// conversion kernels use, against the contract's (float)b / 255.0f for all 256 bytes, bit for bit. Build with -ffp-contract=off.
#include <cstdio>
#include <cstring>

#include "../../stratum_amd/csrc/material_convert.h"

int main() {
  int bad = 0;
  for (unsigned b = 0; b < 256; b++) {
    const float want = (float)b / 255.0f, got = sthip::decode_unorm8(b);
    if (std::memcmp(&want, &got, 4)) {
      std::printf("byte %u: %a, not %a\n", b, got, want);
      bad++;
    }
  }
  std::printf("DECODE bad=%d\n", bad);
  return bad ? 1 : 0;
}
