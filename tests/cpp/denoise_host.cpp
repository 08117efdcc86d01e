// Host run of raytrace2_amd/csrc/denoise.h, the arithmetic of the GPU's a-trous filter
// (tests/test_denoise_host.py). Reads one case from the binary file argv[1]:
//   int32 width, height, iterations, normal_power_log2; float32 sigma_l, sigma_p, sigma_a, eps_l;
//   float32 color[h][w][3], variance[h][w], features[h][w][16]
// and writes float32 color'[h][w][3], variance'[h][w] to the file argv[2].
#include <cstdint>
#include <cstdio>
#include <vector>

#include "denoise.h"

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t hdr[4];
  float sig[4];
  if (std::fread(hdr, sizeof(hdr), 1, f) != 1 || std::fread(sig, sizeof(sig), 1, f) != 1) return 3;
  const int w = hdr[0], h = hdr[1];
  if (w <= 0 || h <= 0 || (long)w * h > (1L << 24)) return 3;
  const rt2::DenoiseParams k{hdr[2], hdr[3], sig[0], sig[1], sig[2], sig[3]};
  if (!rt2::DenoiseParamsValid(k)) return 4;
  const size_t n = (size_t)w * (size_t)h;
  std::vector<float> color(3 * n), variance(n), features((size_t)rt2::kDenoiseFeatureFloats * n);
  if (std::fread(color.data(), sizeof(float), color.size(), f) != color.size() ||
      std::fread(variance.data(), sizeof(float), variance.size(), f) != variance.size() ||
      std::fread(features.data(), sizeof(float), features.size(), f) != features.size())
    return 3;
  std::fclose(f);
  std::vector<rt2::DenoisePixel> px(n), scratch(n);
  for (size_t i = 0; i < n; i++) {
    rt2::DenoisePixel& p = px[i];
    p.c[0] = color[3 * i], p.c[1] = color[3 * i + 1], p.c[2] = color[3 * i + 2];
    p.v = variance[i];
    rt2::DenoiseUnpackFeatures(&features[(size_t)rt2::kDenoiseFeatureFloats * i], p);
  }
  rt2::DenoiseHost(px.data(), scratch.data(), w, h, k);
  for (size_t i = 0; i < n; i++) {
    color[3 * i] = px[i].c[0], color[3 * i + 1] = px[i].c[1], color[3 * i + 2] = px[i].c[2];
    variance[i] = px[i].v;
  }
  std::FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 2;
  const bool ok = std::fwrite(color.data(), sizeof(float), color.size(), o) == color.size() &&
                  std::fwrite(variance.data(), sizeof(float), variance.size(), o) == variance.size();
  return std::fclose(o) == 0 && ok ? 0 : 5;
}
