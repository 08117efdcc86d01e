// Host run of raytrace2_amd/csrc/noise.h NoiseOfPixel, the per-pixel function of the GPU's noise kernel
// (tests/test_noise_host.py). Reads cases from the file argv[1], one per line as hexadecimal bit patterns
//   n a_r a_g a_b q_r q_g q_b        (n decimal; a, q float32)
// and prints per case
//   sem_r sem_g sem_b err finite     (sem float32 bits, err float64 bits, finite 0/1)
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "noise.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  long long n;
  uint32_t w[6];
  int cases = 0;
  while (std::fscanf(f, "%lld %" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32, &n, &w[0], &w[1],
                     &w[2], &w[3], &w[4], &w[5]) == 7) {
    float a[3], q[3];
    std::memcpy(a, w, sizeof(a));
    std::memcpy(q, w + 3, sizeof(q));
    const rt2::PixelNoise p = rt2::NoiseOfPixel(a, q, (int64_t)n);
    uint32_t s[3];
    uint64_t e;
    std::memcpy(s, p.sem, sizeof(s));
    std::memcpy(&e, &p.err, sizeof(e));
    std::printf("%08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %016" PRIx64 " %d\n", s[0], s[1], s[2], e, p.finite ? 1 : 0);
    cases++;
  }
  std::fclose(f);
  return cases > 0 ? 0 : 3;
}
