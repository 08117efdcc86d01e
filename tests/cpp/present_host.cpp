// Host run of raytrace2_amd/csrc/present.h, the arithmetic of the GPU's tone map
// (tests/test_present_host.py). Reads one case from the binary file argv[1]:
//   int32 width, height; float32 color[h][w][3]
// and writes uint8 rgba[h][w][4] to the file argv[2].
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "present.h"

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t hdr[2];
  if (std::fread(hdr, sizeof(hdr), 1, f) != 1) return 3;
  const int w = hdr[0], h = hdr[1];
  if (w <= 0 || h <= 0 || (long)w * h > (1L << 24)) return 3;
  const size_t n = (size_t)w * (size_t)h;
  std::vector<float> color(3 * n);
  if (std::fread(color.data(), sizeof(float), color.size(), f) != color.size()) return 3;
  std::fclose(f);
  std::vector<uint8_t> rgba(4 * n);
  for (size_t i = 0; i < n; i++) {
    const uint32_t word = rt2::PresentPixel(&color[3 * i]);
    // the word as the GPU stores it: little-endian, R first
    const uint8_t b[4] = {(uint8_t)(word & 0xFFu), (uint8_t)((word >> 8) & 0xFFu), (uint8_t)((word >> 16) & 0xFFu),
                          (uint8_t)(word >> 24)};
    std::memcpy(&rgba[4 * i], b, 4);
  }
  std::FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 2;
  const bool ok = std::fwrite(rgba.data(), 1, rgba.size(), o) == rgba.size();
  return std::fclose(o) == 0 && ok ? 0 : 5;
}
