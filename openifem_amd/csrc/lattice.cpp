// lattice.cpp -- host side of the lattice readers (mp_direct.hip; the axis classes of lattice_stencil.hpp for sm_stencil.hip and bb_stencil.hip): plain C++, no device call.
#include <algorithm>
#include <cmath>
#include "lattice.hpp"

namespace ifem {

bool lattice_map(int dim, int64_t nc, int64_t n_nodes, const double *vc, const int32_t *cp, const double *h, int n[3],
                 std::vector<int32_t> &node_of_lattice, std::vector<int32_t> &lattice_of_node) {
  const int nv = 1 << dim;
  if (nc <= 0 || n_nodes <= 0 || n_nodes >= (int64_t(1) << 31)) return false;
  double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0}, M = 0;
  for (int64_t k = 0; k < nc * nv; ++k)
    for (int d = 0; d < dim; ++d) {
      const double x = vc[k * dim + d];
      if (!std::isfinite(x)) return false;
      if (k == 0 || x < lo[d]) lo[d] = x;
      if (k == 0 || x > hi[d]) hi[d] = x;
      M = std::max(M, std::fabs(x));
    }
  const double tol = 8.0 * 2.220446049250313e-16 * M;
  // the lattice step is extent / count (how a box mesh forms its coordinates: lo + i * step); it must be the detected cell edge
  double step[3] = {1, 1, 1};
  int64_t total = 1;
  n[0] = n[1] = n[2] = 1;
  for (int d = 0; d < dim; ++d) {
    if (!(h[d] > 0)) return false;
    const double cells = std::round((hi[d] - lo[d]) / h[d]);
    if (!(cells >= 1) || cells + 1 > kLatticeMaxLine) return false;
    n[d] = int(cells) + 1;
    step[d] = (hi[d] - lo[d]) / cells;
    if (!(std::fabs(step[d] - h[d]) <= tol)) return false;
    total *= n[d];
    if (total > n_nodes) return false; // more lattice points than nodes: a hole
  }
  if (total != n_nodes) return false;
  node_of_lattice.assign(size_t(total), -1);
  lattice_of_node.assign(size_t(n_nodes), -1);
  for (int64_t k = 0; k < nc * nv; ++k) {
    const int32_t node = cp[k];
    if (node < 0 || node >= n_nodes) return false;
    int64_t lin = 0, mul = 1;
    for (int d = 0; d < dim; ++d) {
      const double x = vc[k * dim + d];
      const double fi = std::round((x - lo[d]) / step[d]);
      if (!(fi >= 0 && fi <= n[d] - 1)) return false;
      if (!(std::fabs(x - (lo[d] + fi * step[d])) <= tol)) return false;
      lin += int64_t(fi) * mul;
      mul *= n[d];
    }
    if (lattice_of_node[node] >= 0 && lattice_of_node[node] != lin) return false; // one node at two points
    lattice_of_node[node] = int32_t(lin);
    if (node_of_lattice[lin] >= 0 && node_of_lattice[lin] != node) return false; // two nodes at one point
    node_of_lattice[lin] = node;
  }
  for (int64_t l = 0; l < total; ++l)
    if (node_of_lattice[l] < 0) return false; // a lattice point no cell touches (with total == n_nodes: some node is in no cell either)
  return true;
}

bool lattice_map_u(int dim, int deg, int64_t nc, int64_t n_nodes, const double *vc, const int32_t *cu, const double *h, int n[3],
                   std::vector<int32_t> &node_of_lattice, std::vector<int32_t> &lattice_of_node) {
  const int nv = 1 << dim;
  if ((deg != 1 && deg != 2) || (dim != 2 && dim != 3) || nc <= 0 || n_nodes <= 0 || n_nodes >= (int64_t(1) << 31)) return false;
  const int nloc = dim == 3 ? (deg + 1) * (deg + 1) * (deg + 1) : (deg + 1) * (deg + 1);
  double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0}, M = 0;
  for (int64_t k = 0; k < nc * nv; ++k)
    for (int d = 0; d < dim; ++d) {
      const double x = vc[k * dim + d];
      if (!std::isfinite(x)) return false;
      if (k == 0 || x < lo[d]) lo[d] = x;
      if (k == 0 || x > hi[d]) hi[d] = x;
      M = std::max(M, std::fabs(x));
    }
  const double tol = 8.0 * 2.220446049250313e-16 * M;
  double step[3] = {1, 1, 1};
  int cells[3] = {1, 1, 1};
  int64_t total = 1;
  n[0] = n[1] = n[2] = 1;
  for (int d = 0; d < dim; ++d) {
    if (!(h[d] > 0)) return false;
    const double c = std::round((hi[d] - lo[d]) / h[d]);
    if (!(c >= 1) || deg * c + 1 > kLatticeMaxLine) return false;
    cells[d] = int(c);
    n[d] = deg * cells[d] + 1;
    step[d] = (hi[d] - lo[d]) / c;
    if (!(std::fabs(step[d] - h[d]) <= tol)) return false;
    total *= n[d];
    if (total > n_nodes) return false; // more lattice points than nodes: a hole
  }
  if (total != n_nodes) return false;
  node_of_lattice.assign(size_t(total), -1);
  lattice_of_node.assign(size_t(n_nodes), -1);
  for (int64_t c = 0; c < nc; ++c) {
    // every vertex of the cell at its lattice point: vertex v of cell (c_x, c_y, c_z) at c_d + bit d of v
    int ci[3] = {0, 0, 0};
    for (int v = 0; v < nv; ++v)
      for (int d = 0; d < dim; ++d) {
        const double x = vc[(c * nv + v) * dim + d];
        const double fi = std::round((x - lo[d]) / step[d]);
        if (!(fi >= 0 && fi <= cells[d])) return false;
        if (!(std::fabs(x - (lo[d] + fi * step[d])) <= tol)) return false;
        if (v == 0) {
          if (fi > cells[d] - 1) return false;
          ci[d] = int(fi);
        } else if (int(fi) != ci[d] + ((v >> d) & 1)) return false; // not the box of edges h at that place
      }
    for (int a = 0; a < nloc; ++a) {
      const int32_t node = cu[c * nloc + a];
      if (node < 0 || node >= n_nodes) return false;
      const int t[3] = {a % (deg + 1), (a / (deg + 1)) % (deg + 1), a / ((deg + 1) * (deg + 1))};
      int64_t lin = 0, mul = 1;
      for (int d = 0; d < dim; ++d) {
        lin += int64_t(deg * ci[d] + t[d]) * mul;
        mul *= n[d];
      }
      if (lattice_of_node[node] >= 0 && lattice_of_node[node] != lin) return false; // one node at two points
      lattice_of_node[node] = int32_t(lin);
      if (node_of_lattice[lin] >= 0 && node_of_lattice[lin] != node) return false; // two nodes at one point
      node_of_lattice[lin] = node;
    }
  }
  for (int64_t l = 0; l < total; ++l)
    if (node_of_lattice[l] < 0) return false; // a lattice point no cell touches
  return true;
}

int lattice_axis_classes(int n, std::vector<uint8_t> &cls, std::vector<int32_t> &first) {
  cls.assign(size_t(std::max(n, 0)), 0);
  first.clear();
  int id_of_code[9];
  std::fill(id_of_code, id_of_code + 9, -1);
  for (int i = 0; i < n; ++i) {
    const int code = 3 * std::min(i, 2) + std::min(n - 1 - i, 2);
    if (id_of_code[code] < 0) {
      id_of_code[code] = int(first.size());
      first.push_back(i);
    }
    cls[i] = uint8_t(id_of_code[code]);
  }
  return int(first.size());
}

} // namespace ifem

namespace ifem {

int lattice_axis_classes_u(int n, int deg, std::vector<uint8_t> &cls, std::vector<int32_t> &first) {
  cls.assign(size_t(std::max(n, 0)), 0);
  first.clear();
  if (deg != 1 && deg != 2) return 0;
  const int cap = 2 * deg, ncode = (cap + 1) * (cap + 1) * deg;
  std::vector<int> id_of_code(size_t(ncode), -1);
  for (int i = 0; i < n; ++i) {
    const int a = std::min(i, cap), b = std::min(n - 1 - i, cap);
    const int code = (a * (cap + 1) + b) * deg + (a == cap && b == cap ? i % deg : 0);
    if (id_of_code[code] < 0) {
      id_of_code[code] = int(first.size());
      first.push_back(i);
    }
    cls[i] = uint8_t(id_of_code[code]);
  }
  return int(first.size());
}

} // namespace ifem
