// environment_ref.cpp — a scalar restatement of the two derived forms of an image environment, written from the text of
// include/sthip.h ("the environment of a resident scene"): the dist2d tables and the float mip chain. It pins the reference
// the GPU tests of tests/test_environment.py compare against: it must equal scene.py build_distributions and a numpy
// statement of the mip rule bit for bit. Stand-alone (also built with -fsanitize=address,undefined).
//   environment_ref tables <in> <out>   in: u32 H, u32 W, H*W*4 floats; out: marginal_pdf | row_pdf | marginal_cdf | row_cdf
//   environment_ref mips <in> <out>     out: level 1, level 2, ... back to back (nothing for a 1 x 1 image)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace {

struct Image {
  uint32_t w = 0, h = 0;
  std::vector<float> rgba;
  const float* texel(uint32_t x, uint32_t y) const { return &rgba[4 * ((size_t)y * w + x)]; }
};

bool read_image(const char* path, Image& im) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  uint32_t head[2];
  bool ok = std::fread(head, 4, 2, f) == 2 && head[0] && head[1];
  if (ok) {
    im.h = head[0], im.w = head[1];
    im.rgba.resize((size_t)im.w * im.h * 4);
    ok = std::fread(im.rgba.data(), 4, im.rgba.size(), f) == im.rgba.size();
  }
  std::fclose(f);
  return ok;
}

bool write_floats(const char* path, const std::vector<float>& v) {
  FILE* f = std::fopen(path, "wb");
  if (!f) return false;
  const bool ok = v.empty() || std::fwrite(v.data(), 4, v.size(), f) == v.size();
  std::fclose(f);
  return ok;
}

// f(x, y) of the contract: binary32 luminance times the binary64 sine of the row
struct Weights {
  const Image& im;
  std::vector<double> s;
  explicit Weights(const Image& image) : im(image), s(image.h) {
    const float inv_h = 1 / (float)im.h;
    for (uint32_t y = 0; y < im.h; y++) {
      const float row = y + 0.5f;
      s[y] = std::sin(M_PI * row * inv_h);
    }
  }
  double operator()(uint32_t x, uint32_t y) const {
    const float* t = im.texel(x, y);
    const float rg = t[0] * 0.2126f + t[1] * 0.7152f;
    const float lum = rg + t[2] * 0.0722f;
    return (double)lum * s[y];
  }
};

std::vector<float> tables(const Image& im) {
  const uint32_t W = im.w, H = im.h;
  std::vector<float> out((size_t)H + (size_t)H * W + (H + 1) + (size_t)H * (W + 1));
  float* marginal_pdf = out.data();
  float* row_pdf = marginal_pdf + H;
  float* marginal_cdf = row_pdf + (size_t)H * W;
  float* row_cdf = marginal_cdf + H + 1;
  const Weights f(im);
  std::vector<float> weight(H);  // what each row contributes to the marginal
  for (uint32_t y = 0; y < H; y++) {
    float* row = row_cdf + (size_t)y * (W + 1);
    float* pdf = row_pdf + (size_t)y * W;
    float running = 0;
    row[0] = running;
    for (uint32_t x = 0; x < W; x++) {
      running = (float)((double)running + f(x, y));
      row[x + 1] = running;
    }
    const float integral = running;
    if (integral > 0) {
      for (uint32_t x = 0; x < W; x++) {
        row[x] = row[x] / integral;
        pdf[x] = (float)(f(x, y) / (double)integral);
      }
      weight[y] = integral;
    } else {  // zero, negative or NaN: uniform
      for (uint32_t x = 0; x < W; x++) {
        pdf[x] = 1.0f / (float)W;
        row[x] = (float)x / (float)W;
      }
      weight[y] = 1;
    }
    row[W] = 1;  // (the contract sets it last; nothing reads it in between but the marginal, which has `weight`)
  }
  float total = 0;
  marginal_cdf[0] = 0;
  for (uint32_t y = 0; y < H; y++) {
    total = total + weight[y];
    marginal_cdf[y + 1] = total;
  }
  for (uint32_t y = 0; y < H; y++) {
    if (total > 0) {
      marginal_cdf[y] = marginal_cdf[y] / total;
      marginal_pdf[y] = weight[y] / total;
    } else {
      marginal_pdf[y] = 1.0f / (float)H;
      marginal_cdf[y] = (float)y / (float)H;
    }
  }
  marginal_cdf[H] = 1;
  return out;
}

std::vector<float> mips(Image level) {
  std::vector<float> out;
  while (level.w > 1 || level.h > 1) {
    Image next;
    next.w = level.w / 2 ? level.w / 2 : 1;
    next.h = level.h / 2 ? level.h / 2 : 1;
    next.rgba.resize((size_t)next.w * next.h * 4);
    auto clamp = [](uint32_t v, uint32_t last) { return v < last ? v : last; };
    for (uint32_t y = 0; y < next.h; y++)
      for (uint32_t x = 0; x < next.w; x++) {
        const uint32_t x0 = clamp(2 * x, level.w - 1), x1 = clamp(2 * x + 1, level.w - 1), y0 = clamp(2 * y, level.h - 1), y1 = clamp(2 * y + 1, level.h - 1);
        const float *a = level.texel(x0, y0), *b = level.texel(x1, y0), *c = level.texel(x0, y1), *e = level.texel(x1, y1);
        for (int k = 0; k < 4; k++) {
          const float top = a[k] + b[k], bottom = c[k] + e[k];
          next.rgba[4 * ((size_t)y * next.w + x) + k] = (top + bottom) * 0.25f;
        }
      }
    out.insert(out.end(), next.rgba.begin(), next.rgba.end());
    level = std::move(next);
  }
  return out;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) return std::fprintf(stderr, "usage: environment_ref tables|mips <in> <out>\n"), 2;
  Image im;
  if (!read_image(argv[2], im)) return std::fprintf(stderr, "cannot read %s\n", argv[2]), 2;
  const std::string mode = argv[1];
  if (mode != "tables" && mode != "mips") return 2;
  return write_floats(argv[3], mode == "tables" ? tables(im) : mips(im)) ? 0 : 2;
}
