// Host run of raytrace2_amd/csrc/temporal.h, the arithmetic of the GPU's temporal blend
// (tests/test_temporal_host.py). Reads one case from the binary file argv[1]:
//   int32 width, height, n_materials (-1: no table), 0;
//   float32 max_history, max_history_specular, min_normal_dot, sigma_p, sigma_a; float32 hist_camera[21];
//   float32 color[h][w][3], variance[h][w], length[h][w], features[h][w][16], then the history's same four,
//   then materials[n_materials][8]
// and writes float32 color'[h][w][3], variance'[h][w], length'[h][w] to the file argv[2].
#include <cstdint>
#include <cstdio>
#include <vector>

#include "temporal.h"

namespace {
bool ReadFloats(std::FILE* f, std::vector<float>& v) { return v.empty() || std::fread(v.data(), sizeof(float), v.size(), f) == v.size(); }
bool WriteFloats(std::FILE* f, const std::vector<float>& v) {
  return v.empty() || std::fwrite(v.data(), sizeof(float), v.size(), f) == v.size();
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t hdr[4];
  float par[5], cam[rt2::kTemporalCameraWords];
  if (std::fread(hdr, sizeof(hdr), 1, f) != 1 || std::fread(par, sizeof(par), 1, f) != 1 ||
      std::fread(cam, sizeof(cam), 1, f) != 1)
    return 3;
  const int w = hdr[0], h = hdr[1], n_mat = hdr[2];
  if (w <= 0 || h <= 0 || (long)w * h > (1L << 24) || n_mat < -1 || n_mat > (1 << 16)) return 3;
  const rt2::TemporalParams k{par[0], par[1], par[2], par[3], par[4]};
  if (!rt2::TemporalParamsValid(k)) return 4;
  const size_t n = (size_t)w * (size_t)h, nf = (size_t)rt2::kDenoiseFeatureFloats * n;
  std::vector<float> color(3 * n), variance(n), length(n), features(nf);
  std::vector<float> hcolor(3 * n), hvariance(n), hlength(n), hfeatures(nf);
  std::vector<float> materials(n_mat > 0 ? (size_t)n_mat * rt2::kTemporalMaterialFloats : 0);
  if (!ReadFloats(f, color) || !ReadFloats(f, variance) || !ReadFloats(f, length) || !ReadFloats(f, features) ||
      !ReadFloats(f, hcolor) || !ReadFloats(f, hvariance) || !ReadFloats(f, hlength) || !ReadFloats(f, hfeatures) ||
      !ReadFloats(f, materials))
    return 3;
  std::fclose(f);
  std::vector<rt2::TemporalPixel> hist(n);
  for (size_t i = 0; i < n; i++)
    hist[i] = rt2::TemporalPack(&hcolor[3 * i], hvariance[i], hlength[i], &hfeatures[(size_t)rt2::kDenoiseFeatureFloats * i]);
  const rt2::TemporalCamera K = rt2::TemporalCameraOf(cam);
  std::vector<float> oc(3 * n), ov(n), on(n);
  for (int y = 0; y < h; y++) {
    for (int x = 0; x < w; x++) {
      const size_t i = (size_t)y * (size_t)w + (size_t)x;
      const auto fetch = [&](int qx, int qy) { return hist.at((size_t)qy * (size_t)w + (size_t)qx); };
      const rt2::TemporalResult r = rt2::TemporalResolvePixel(
          &color[3 * i], variance[i], length[i], &features[(size_t)rt2::kDenoiseFeatureFloats * i], K, w, h,
          materials.empty() ? nullptr : materials.data(), n_mat > 0 ? n_mat : 0, false, k, fetch);
      oc[3 * i] = r.c[0], oc[3 * i + 1] = r.c[1], oc[3 * i + 2] = r.c[2];
      ov[i] = r.v;
      on[i] = r.len;
    }
  }
  std::FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 2;
  const bool ok = WriteFloats(o, oc) && WriteFloats(o, ov) && WriteFloats(o, on);
  return std::fclose(o) == 0 && ok ? 0 : 5;
}
