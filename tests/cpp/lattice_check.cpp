#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include "lattice.hpp"
using namespace ifem;
static void box(int dim, const int *reps, const double *h, const double *lo, bool perm, std::vector<double> &vc, std::vector<int32_t> &cp, int64_t &nn) {
  int n[3] = {1, 1, 1};
  for (int d = 0; d < dim; ++d) n[d] = reps[d] + 1;
  nn = int64_t(n[0]) * n[1] * n[2];
  std::vector<int32_t> id(nn);
  std::iota(id.begin(), id.end(), 0);
  if (perm) { std::mt19937 g(5); std::shuffle(id.begin(), id.end(), g); }
  const int nv = 1 << dim;
  vc.clear(); cp.clear();
  for (int cz = 0; cz < (dim == 3 ? reps[2] : 1); ++cz)
    for (int cy = 0; cy < reps[1]; ++cy)
      for (int cx = 0; cx < reps[0]; ++cx)
        for (int v = 0; v < nv; ++v) {
          const int i[3] = {cx + (v & 1), cy + ((v >> 1) & 1), cz + ((v >> 2) & 1)};
          for (int d = 0; d < dim; ++d) vc.push_back(lo[d] + i[d] * h[d]);
          cp.push_back(id[i[0] + n[0] * (i[1] + int64_t(n[1]) * i[2])]);
        }
}
int main() {
  int fails = 0;
  const double h[3] = {0.4, 0.1, 0.35}, lo[3] = {0.3, -0.1, 0.2};
  const int shapes[][4] = {{3, 5, 3, 2}, {3, 4, 1, 3}, {3, 1, 1, 1}, {3, 70, 2, 2}, {2, 7, 4, 0}, {2, 70, 3, 0}, {3, 4, 3, 5}};
  for (auto &s : shapes) {
    for (int perm = 0; perm < 2; ++perm) {
      std::vector<double> vc; std::vector<int32_t> cp, nol, lon; int64_t nn; int n[3];
      box(s[0], s + 1, h, lo, perm, vc, cp, nn);
      const int64_t nc = int64_t(cp.size()) >> s[0];
      bool ok = lattice_map(s[0], nc, nn, vc.data(), cp.data(), h, n, nol, lon);
      for (int64_t l = 0; ok && l < nn; ++l) ok = lon[nol[l]] == l;
      for (int d = 0; d < s[0]; ++d) ok = ok && n[d] == s[1 + d] + 1;
      if (!ok) { printf("FAIL map dim %d %d x %d x %d perm %d\n", s[0], s[1], s[2], s[3], perm); ++fails; }
      // refused inputs: a moved vertex, a duplicate node, a node out of range, one node short
      std::vector<double> v2 = vc; v2[s[0]] += 1e-6;
      if (lattice_map(s[0], nc, nn, v2.data(), cp.data(), h, n, nol, lon)) { printf("FAIL moved vertex accepted\n"); ++fails; }
      std::vector<int32_t> c2 = cp; c2[0] = c2.back();
      if (nn > 2 && lattice_map(s[0], nc, nn, vc.data(), c2.data(), h, n, nol, lon)) { printf("FAIL duplicate accepted\n"); ++fails; }
      c2 = cp; c2[1] = int32_t(nn);
      if (lattice_map(s[0], nc, nn, vc.data(), c2.data(), h, n, nol, lon)) { printf("FAIL out of range accepted\n"); ++fails; }
      if (lattice_map(s[0], nc, nn - 1, vc.data(), cp.data(), h, n, nol, lon)) { printf("FAIL short node count accepted\n"); ++fails; }
      if (lattice_map(s[0], nc, nn + 1, vc.data(), cp.data(), h, n, nol, lon)) { printf("FAIL long node count accepted\n"); ++fails; }
    }
  }
  for (int n = 1; n <= 9; ++n) {
    std::vector<uint8_t> cls; std::vector<int32_t> first;
    const int k = lattice_axis_classes(n, cls, first);
    bool ok = k == (n < 5 ? n : 5) && int(cls.size()) == n && int(first.size()) == k;
    for (int i = 0; ok && i < n; ++i) {
      const int f = first[cls[i]];
      ok = cls[i] < k && std::min(f, 2) == std::min(i, 2) && std::min(n - 1 - f, 2) == std::min(n - 1 - i, 2) && f <= i;
    }
    if (!ok) { printf("FAIL axis classes n = %d\n", n); ++fails; }
  }
  printf("%s (%d failures)\n", fails ? "FAILED" : "ok", fails);
  return fails != 0;
}
