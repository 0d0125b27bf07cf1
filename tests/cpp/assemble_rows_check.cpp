// Stand-alone check of the index arithmetic of the row-owner assembly (csrc/assemble_rows.hpp): over all owners of a box of n_x x n_y x n_z
// Q2 cells, every (row node, cell, local index) incidence of the mesh is produced exactly once, by the owner of the node; the pairs of
// one node are adjacent; every column of a pair sits inside the owner's 5^3 neighbourhood at the lattice point the cell's local numbering
// gives it, inside the row's stencil box; and every (row, column) of the lattice pattern is produced by a pair whose cell holds both --
// once per such cell, no more.
#include <cstdio>
#include <map>
#include <set>
#include <vector>
#include "assemble_rows.hpp"

using namespace ifem::rows;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { if (++failures < 20) std::printf("FAILED %s (line %d)\n", #c, __LINE__); } } while (0)

static void run(int nx, int ny, int nz) {
  const int n[3] = {nx, ny, nz};
  const int nl[3] = {2 * nx + 1, 2 * ny + 1, 2 * nz + 1};
  const int64_t npts = int64_t(nl[0]) * nl[1] * nl[2];
  auto point = [&](int x, int y, int z) { return x + int64_t(nl[0]) * (y + int64_t(nl[1]) * z); };
  // the mesh's incidences: (lattice point, cell, local index) and the pattern (row, column) -> number of cells that hold both
  std::set<std::vector<int64_t>> want;
  std::map<std::pair<int64_t, int64_t>, int> pattern, got;
  for (int cz = 0; cz < nz; ++cz)
    for (int cy = 0; cy < ny; ++cy)
      for (int cx = 0; cx < nx; ++cx) {
        const int64_t cell = cx + int64_t(nx) * (cy + int64_t(ny) * cz);
        for (int a = 0; a < 27; ++a) {
          const int64_t pa = point(2 * cx + a % 3, 2 * cy + (a / 3) % 3, 2 * cz + a / 9);
          want.insert({pa, cell, a});
          for (int b = 0; b < 27; ++b) ++pattern[{pa, point(2 * cx + b % 3, 2 * cy + (b / 3) % 3, 2 * cz + b / 9)}];
        }
      }
  std::set<std::vector<int64_t>> seen;
  std::vector<int> owned(npts, 0);
  const int64_t no = n_owners(n);
  CHECK(no == int64_t(nx + 1) * (ny + 1) * (nz + 1));
  for (int64_t o = 0; o < no; ++o) {
    int ijk[3];
    owner_ijk(o, n, ijk);
    CHECK(ijk[0] >= 0 && ijk[0] <= nx && ijk[1] >= 0 && ijk[1] <= ny && ijk[2] >= 0 && ijk[2] <= nz);
    int last_nd = -1;
    std::set<int> nodes_done;
    for (int p = 0; p < kPairs; ++p) {
      const Pair P = pair_of(p);
      CHECK(P.nd >= 0 && P.nd < 8 && P.a >= 0 && P.a < 27 && (P.cb & P.nd) == 0);
      if (P.nd != last_nd) { CHECK(!nodes_done.count(P.nd)); nodes_done.insert(P.nd); last_nd = P.nd; } // pairs of one node are adjacent
      const int64_t row = row_point(ijk, n, P.nd);
      const int64_t cell = pair_cell(ijk, n, P);
      if (row < 0) continue;
      CHECK(row < npts);
      CHECK(row == nb_point(ijk, n, nb_of_node(P.nd)));
      if (p == kNodeFirst[0] || P.nd != pair_of(p - 1).nd) ++owned[row];
      if (cell < 0) continue;
      CHECK(cell < int64_t(nx) * ny * nz);
      CHECK(seen.insert({row, cell, P.a}).second); // exactly once
      CHECK(want.count({row, cell, P.a}) == 1);
      const int cx = int(cell % nx), cy = int((cell / nx) % ny), cz = int(cell / (int64_t(nx) * ny));
      for (int b = 0; b < 27; ++b) {
        const int t = nb_of_column(P.cb, b);
        CHECK(t >= 0 && t < 125);
        const int64_t col = nb_point(ijk, n, t);
        CHECK(col == point(2 * cx + b % 3, 2 * cy + (b / 3) % 3, 2 * cz + b / 9)); // inside the lattice, at the cell's own point
        // inside the row's stencil box: at most 2 points from the row on every axis
        const int td[3] = {t % 5, (t / 5) % 5, t / 25};
        for (int d = 0; d < 3; ++d) CHECK(td[d] - (2 + ((P.nd >> d) & 1)) >= -2 && td[d] - (2 + ((P.nd >> d) & 1)) <= 2);
        ++got[{row, col}];
      }
    }
    CHECK(nodes_done.size() == 8);
  }
  CHECK(seen.size() == want.size());
  for (int64_t i = 0; i < npts; ++i) CHECK(owned[i] == 1); // every lattice node has exactly one owner
  CHECK(got == pattern);
  std::printf("%d x %d x %d cells: %lld owners, %zu incidences, %zu pattern entries\n", nx, ny, nz, (long long)no, seen.size(), got.size());
}

int main() {
  // pair table: 8 + 4 + 4 + 4 + 2 + 2 + 2 + 1, tile 0 = pairs 0..15, tile 1 = pairs 16..26
  int cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int p = 0; p < kPairs; ++p) ++cnt[pair_of(p).nd];
  const int expect[8] = {8, 4, 4, 2, 4, 2, 2, 1};
  for (int i = 0; i < 8; ++i) CHECK(cnt[i] == expect[i]);
  run(1, 1, 1);
  run(1, 2, 3);
  run(2, 2, 2);
  run(3, 3, 3);
  run(5, 4, 3);
  std::printf("ok (%d failures)\n", failures);
  return failures != 0;
}
