// Host sanitizer run of the radial reductions (test infrastructure): emu_radial.cpp -- the radial.h code the
// gfx950 kernels run -- built as ONE executable with -fsanitize=address,undefined, so no sanitizer runtime
// has to be preloaded into Python.  Runs the power spectrum, the profile gradient (shared and per channel)
// and the dense pair at 2 x 3 x 12 x 10 x 9 in both modes; checks Parseval, that bin(expand) keeps the
// shell counts and that every output is written; exits non-zero on a violation (the sanitizers abort on
// their own findings).
#include "emu_radial.cpp"

#include <cstdio>
#include <random>

int main() {
  const int B = 2, C = 3, H = 12, W = 10, D = 9, K = 8;
  const int64_t N = (int64_t)H * W * D;
  std::vector<float> x((size_t)B * C * N), g(x.size());
  std::mt19937 gen(31);
  std::normal_distribution<float> nd;
  for (auto& v : x) v = nd(gen);
  for (auto& v : g) v = nd(gen);
  const int64_t st[3] = {N, (int64_t)W * D, D};
  int fails = 0;
  for (int mode = 0; mode < 2; ++mode) {
    std::vector<float> P((size_t)B * C * K, std::nanf(""));
    if (tbemu_kspace_radial_f32(H, W, D, x.data(), st, nullptr, nullptr, P.data(), 1, K, 1.0, mode, B, C, 7, 2)) ++fails;
    for (int v = 0; v < B * C; ++v) {
      double sp = 0.0, sx = 0.0;
      for (int k = 0; k < K; ++k) sp += P[(size_t)v * K + k];
      for (int64_t i = 0; i < N; ++i) sx += (double)x[v * N + i] * x[v * N + i];
      if (!(std::fabs(sp - sx) <= 1e-5 * sx)) { std::fprintf(stderr, "parseval %d %d: %g %g\n", mode, v, sp, sx); ++fails; }
    }
    for (int Cp : {1, C}) {
      std::vector<float> dp((size_t)Cp * K, std::nanf(""));
      if (tbemu_kspace_radial_f32(H, W, D, x.data(), st, g.data(), st, dp.data(), Cp, K, 1.0, mode, B, C, 7, 2)) ++fails;
      for (float v : dp) if (!std::isfinite(v)) { std::fprintf(stderr, "dp not written\n"); ++fails; }
    }
    std::vector<float> ones(K, 1.f), M((size_t)N, std::nanf("")), q(K, std::nanf(""));
    if (tbemu_radial_mask_f32(H, W, D, ones.data(), 1, K, 1.0, mode, M.data())) ++fails;
    if (tbemu_radial_bin_f32(H, W, D, M.data(), 1, K, 1.0, mode, q.data(), 100, 3)) ++fails;
    double cnt = 0.0;
    for (float v : q) cnt += v;
    if (!(std::fabs(cnt - (double)N) <= 1e-4 * N)) { std::fprintf(stderr, "counts %g\n", cnt); ++fails; }
  }
  if (fails) return 1;
  std::printf("emu radial sanitizer run ok\n");
  return 0;
}
