// Stand-alone host program for the AddressSanitizer / UBSan run of the pipelined gallery preparation (ncc_prep6.hip):
// the CPU emulation of the kernels (tests/emu) plus the library's launchers, driven through the C ABI.  The prepared
// buffers and the maps are heap allocations of exactly the sizes the ABI asks for, so a store or load outside them
// stops the program; the results of the two kernels are compared as in tests/prep6_cases.py.
//   tools/san_prep6/build.sh && tools/san_prep6/_build/san_prep6
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "shoeprint_mi355x.h"

static std::vector<unsigned char> prepare(const char* flag, const spr_ncc_shape& shape, const std::vector<float>& maps,
                                          int n) {
  setenv("SPR_PREP6", flag, 1);
  spr_ncc_plan* plan = nullptr;
  if (spr_ncc_plan_create(&shape, &plan) != 0) { std::fprintf(stderr, "plan: %s\n", spr_last_error()); std::exit(2); }
  int32_t rows = 0, cols = 0;
  spr_ncc_plan_fft_size(plan, &rows, &cols);
  if (rows != 192 || cols != 96) { std::fprintf(stderr, "grid %d x %d\n", rows, cols); std::exit(2); }
  std::vector<unsigned char> out(spr_ncc_gallery_bytes(plan, n));
  if (spr_ncc_prepare_gallery(plan, maps.data(), n, out.data(), nullptr) != 0) {
    std::fprintf(stderr, "prepare: %s\n", spr_last_error());
    std::exit(2);
  }
  spr_ncc_plan_destroy(plan);
  return out;
}

int main() {
  int failures = 0;
  const int shapes[3][2] = {{128, 64}, {124, 60}, {130, 68}};  // 130 x 68: the largest map of the six-wave layout (126 x 64)
  for (const auto& hw : shapes) {
    const int n = 2, channels = 3, h = hw[0], w = hw[1];
    std::vector<float> maps(static_cast<size_t>(n) * channels * h * w);
    uint32_t state = 12345u + h;
    for (size_t i = 0; i < maps.size(); ++i) {
      state = state * 1664525u + 1013904223u;
      const float v = static_cast<float>(state >> 8) / 16777216.0f - 0.45f;
      maps[i] = v > 0.0f ? v : 0.0f;  // post-ReLU-like
    }
    for (int i = 0; i < n; ++i)  // the last channel of every item is all zero
      std::memset(&maps[(static_cast<size_t>(i) * channels + channels - 1) * h * w], 0, sizeof(float) * h * w);
    const spr_ncc_shape shape{channels, h, w, h, w, 2, SPR_F32, SPR_NCC_FFT};
    const std::vector<unsigned char> a = prepare("0", shape, maps, n), b = prepare("1", shape, maps, n);
    const size_t spec_per_chan = 2 * 12 * 384 + 192, inv_per_chan = 6 * 384 * 4, item = a.size() / n;
    const size_t spec_bytes = channels * spec_per_chan * 8, inv_bytes = channels * inv_per_chan * 4;
    double worst = 0.0;
    for (int i = 0; i < n; ++i) {
      const unsigned char *pa = a.data() + i * item, *pb = b.data() + i * item;
      if (std::memcmp(pa, pb, spec_bytes) != 0) { std::printf("%dx%d item %d: spectra differ\n", h, w, i); ++failures; }
      if (std::memcmp(pa + spec_bytes + inv_bytes, pb + spec_bytes + inv_bytes, channels) != 0) {
        std::printf("%dx%d item %d: dead flags differ\n", h, w, i);
        ++failures;
      }
      for (size_t k = 0; k < static_cast<size_t>(channels) * inv_per_chan; ++k) {
        float x, y;
        std::memcpy(&x, pa + spec_bytes + 4 * k, 4);
        std::memcpy(&y, pb + spec_bytes + 4 * k, 4);
        if ((x == 0.0f) != (y == 0.0f)) { ++failures; continue; }
        const float big = std::fabs(x) > std::fabs(y) ? std::fabs(x) : std::fabs(y);
        const double step = std::nextafter(big, INFINITY) - big;
        const double d = std::fabs(static_cast<double>(x) - y);
        if (d > step) ++failures;
        if (step > 0 && d / step > worst) worst = d / step;
      }
    }
    std::printf("%d x %d: 1/sigma within %.2f float32 steps\n", h, w, worst);
  }
  std::printf(failures ? "FAILED (%d)\n" : "ok\n", failures);
  return failures ? 1 : 0;
}
