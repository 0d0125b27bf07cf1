#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include "lattice.hpp"
using namespace ifem;
// cell tables of a box of reps cells with velocity nodes of degree deg, local index x fastest; perm: node ids shuffled
static void box(int dim, int deg, const int *reps, const double *h, const double *lo, bool perm, std::vector<double> &vc, std::vector<int32_t> &cu, int64_t &nn) {
  int n[3] = {1, 1, 1};
  for (int d = 0; d < dim; ++d) n[d] = deg * reps[d] + 1;
  nn = int64_t(n[0]) * n[1] * n[2];
  std::vector<int32_t> id(nn);
  std::iota(id.begin(), id.end(), 0);
  if (perm) { std::mt19937 g(5); std::shuffle(id.begin(), id.end(), g); }
  const int nv = 1 << dim, q = deg + 1;
  vc.clear(); cu.clear();
  for (int cz = 0; cz < (dim == 3 ? reps[2] : 1); ++cz)
    for (int cy = 0; cy < reps[1]; ++cy)
      for (int cx = 0; cx < reps[0]; ++cx) {
        for (int v = 0; v < nv; ++v) {
          const int i[3] = {cx + (v & 1), cy + ((v >> 1) & 1), cz + ((v >> 2) & 1)};
          for (int d = 0; d < dim; ++d) vc.push_back(lo[d] + i[d] * h[d]);
        }
        for (int tz = 0; tz < (dim == 3 ? q : 1); ++tz)
          for (int ty = 0; ty < q; ++ty)
            for (int tx = 0; tx < q; ++tx) cu.push_back(id[(deg * cx + tx) + n[0] * ((deg * cy + ty) + int64_t(n[1]) * (deg * cz + tz))]);
      }
}
int main() {
  int fails = 0;
  const double h[3] = {0.4, 0.1, 0.35}, lo[3] = {0.3, -0.1, 0.2};
  const int shapes[][4] = {{3, 5, 3, 2}, {3, 4, 1, 3}, {3, 1, 1, 1}, {3, 70, 2, 2}, {2, 7, 4, 0}, {2, 70, 3, 0}, {2, 1, 1, 0}, {3, 4, 3, 5}};
  for (auto &s : shapes)
    for (int deg = 1; deg <= 2; ++deg)
      for (int perm = 0; perm < 2; ++perm) {
        const int dim = s[0], nloc = dim == 3 ? (deg + 1) * (deg + 1) * (deg + 1) : (deg + 1) * (deg + 1);
        std::vector<double> vc; std::vector<int32_t> cu, nol, lon; int64_t nn; int n[3];
        box(dim, deg, s + 1, h, lo, perm, vc, cu, nn);
        const int64_t nc = int64_t(cu.size()) / nloc;
        bool ok = lattice_map_u(dim, deg, nc, nn, vc.data(), cu.data(), h, n, nol, lon);
        for (int64_t l = 0; ok && l < nn; ++l) ok = lon[nol[l]] == l;
        for (int d = 0; d < dim; ++d) ok = ok && n[d] == deg * s[1 + d] + 1;
        // the node at the low corner of cell 0 is lattice point 0, the last node of the last cell the last point
        ok = ok && lon[cu[0]] == 0 && lon[cu.back()] == nn - 1;
        if (!ok) { printf("FAIL map dim %d deg %d %d x %d x %d perm %d\n", dim, deg, s[1], s[2], s[3], perm); ++fails; }
        // refused inputs: a moved vertex (a non-uniform cell), a duplicate node, a node out of range, a hole (one node short), one node too many,
        // a degree the map does not know
        std::vector<double> v2 = vc; v2[dim] += 1e-6;
        if (lattice_map_u(dim, deg, nc, nn, v2.data(), cu.data(), h, n, nol, lon)) { printf("FAIL moved vertex accepted\n"); ++fails; }
        v2 = vc; v2[(size_t(1) << dim) * dim - 1] += h[dim - 1]; // the last vertex of cell 0 one cell further: not the box of edges h
        if (lattice_map_u(dim, deg, nc, nn, v2.data(), cu.data(), h, n, nol, lon)) { printf("FAIL stretched cell accepted\n"); ++fails; }
        std::vector<int32_t> c2 = cu; c2[0] = c2.back();
        if (lattice_map_u(dim, deg, nc, nn, vc.data(), c2.data(), h, n, nol, lon)) { printf("FAIL duplicate accepted\n"); ++fails; }
        c2 = cu; c2[1] = int32_t(nn);
        if (lattice_map_u(dim, deg, nc, nn, vc.data(), c2.data(), h, n, nol, lon)) { printf("FAIL out of range accepted\n"); ++fails; }
        c2 = cu; c2[1] = -1;
        if (lattice_map_u(dim, deg, nc, nn, vc.data(), c2.data(), h, n, nol, lon)) { printf("FAIL negative node accepted\n"); ++fails; }
        if (lattice_map_u(dim, deg, nc, nn - 1, vc.data(), cu.data(), h, n, nol, lon)) { printf("FAIL short node count accepted\n"); ++fails; }
        if (lattice_map_u(dim, deg, nc, nn + 1, vc.data(), cu.data(), h, n, nol, lon)) { printf("FAIL long node count accepted\n"); ++fails; }
        if (nc > 1 && lattice_map_u(dim, deg, nc - 1, nn, vc.data(), cu.data(), h, n, nol, lon)) { printf("FAIL missing cell (a hole) accepted\n"); ++fails; }
        if (lattice_map_u(dim, 3, nc, nn, vc.data(), cu.data(), h, n, nol, lon)) { printf("FAIL degree 3 accepted\n"); ++fails; }
      }
  for (int deg = 1; deg <= 2; ++deg)
    for (int n = 1; n <= 14; ++n) {
      std::vector<uint8_t> cls; std::vector<int32_t> first;
      const int k = lattice_axis_classes_u(n, deg, cls, first), cap = 2 * deg;
      bool ok = k >= 1 && k <= 5 * deg && int(cls.size()) == n && int(first.size()) == k;
      for (int i = 0; ok && i < n; ++i) {
        const int f = first[cls[i]];
        const bool capped = std::min(i, cap) == cap && std::min(n - 1 - i, cap) == cap;
        ok = cls[i] < k && std::min(f, cap) == std::min(i, cap) && std::min(n - 1 - f, cap) == std::min(n - 1 - i, cap) && f <= i && (!capped || f % deg == i % deg);
      }
      // two points with different signatures never share an id
      for (int i = 0; ok && i < n; ++i)
        for (int j = 0; ok && j < i; ++j)
          if (cls[i] == cls[j]) ok = std::min(i, cap) == std::min(j, cap) && std::min(n - 1 - i, cap) == std::min(n - 1 - j, cap);
      if (!ok) { printf("FAIL axis classes n = %d deg %d\n", n, deg); ++fails; }
    }
  printf("%s (%d failures)\n", fails ? "FAILED" : "ok", fails);
  return fails != 0;
}
