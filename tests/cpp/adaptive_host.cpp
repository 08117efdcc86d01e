// Host run of raytrace2_amd/csrc/adaptive.h, the per-pixel rules of the GPU's adaptive check
// (tests/test_adaptive_host.py): AdaptiveOver per pixel, then AdaptiveWindowOver along the row. Reads rows
// from the file argv[1]: a header line
//   threshold window width          (threshold as float32 bits in hexadecimal; window, width decimal)
// followed by `width` pixel lines
//   n a_r a_g a_b q_r q_g q_b active   (n, active decimal; a, q float32 bits in hexadecimal)
// and prints per pixel
//   over finite stays               (0/1 each; stays = active && some pixel over within the window)
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "adaptive.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  uint32_t thr_bits;
  int window, width, rows = 0;
  while (std::fscanf(f, "%" SCNx32 " %d %d", &thr_bits, &window, &width) == 3) {
    if (width < 1 || window < 0 || window > rt2::kAdaptiveWindowMax) return 4;
    float thr;
    std::memcpy(&thr, &thr_bits, sizeof(thr));
    std::vector<uint8_t> over((size_t)width), finite((size_t)width), active((size_t)width);
    for (int x = 0; x < width; x++) {
      unsigned n, act;
      uint32_t w[6];
      if (std::fscanf(f, "%u %" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32 " %u", &n, &w[0],
                      &w[1], &w[2], &w[3], &w[4], &w[5], &act) != 8)
        return 4;
      float a[3], q[3];
      std::memcpy(a, w, sizeof(a));
      std::memcpy(q, w + 3, sizeof(q));
      const rt2::PixelOver o = rt2::AdaptiveOver(a, q, (uint32_t)n, (double)thr);
      over[(size_t)x] = o.over ? 1 : 0;
      finite[(size_t)x] = o.finite ? 1 : 0;
      active[(size_t)x] = act ? 1 : 0;
    }
    for (int x = 0; x < width; x++) {
      const bool stays = active[(size_t)x] && rt2::AdaptiveWindowOver(over.data(), 0, x, width, window);
      std::printf("%d %d %d\n", (int)over[(size_t)x], (int)finite[(size_t)x], stays ? 1 : 0);
    }
    rows++;
  }
  std::fclose(f);
  return rows > 0 ? 0 : 3;
}
