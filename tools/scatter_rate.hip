// scatter_rate.hip -- how fast can one wavefront per cell add its 27 x (27 blocks of 72 bytes) to 27 rows of a 64 GB block-CSR value
// array, by kind of memory operation?  The assembly kernel's scatter (assemble3.hip) issues f64 atomics and sits on the memory-side
// atomic rate (~25 G requests of <= 64 bytes per second = 1.6 TB/s of values).  If the cells of one launch never share a row (a cell
// colouring), the same update is a plain read-modify-write.  Rates here decide whether that is worth building.
//   hipcc -O3 --offload-arch=gfx950 -munsafe-fp-atomics tools/scatter_rate.hip -o tools/scatter_rate && tools/scatter_rate
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)
typedef double d2 __attribute__((ext_vector_type(2)));

constexpr int ROW = 1125; // doubles per matrix row (125 blocks of 9)
constexpr int SPAN = 243; // doubles one cell adds to a row (27 blocks), contiguous here: the best case of the row order

__device__ inline unsigned hash32(unsigned x) { x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16; return x; }

// MODE 0: f64 atomic add, 8 bytes per lane   1: plain store 8 B / lane   2: load + add + store 8 B / lane
//      3: load + add + store 16 B / lane     4: plain store 16 B / lane  5: as 3 with the loads of the next row issued before the stores
// LOCAL: rows of a cell are neighbours (8 apart) instead of random
template <int MODE, bool LOCAL>
__global__ __launch_bounds__(128) void k_scatter(double *buf, unsigned n_rows, unsigned n_cells) {
  const unsigned cell = blockIdx.x * 2 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (cell >= n_cells) return;
  const double v = 1.0 + lane;
  d2 nxt = {0, 0};
  for (int a = 0; a < 27; ++a) {
    const unsigned h = hash32(cell * 27u + a);
    const unsigned row = LOCAL ? (hash32(cell) % (n_rows - 256) + 8u * a + (h & 7u)) : h % n_rows;
    const unsigned off = (hash32(h) % 98u) * 9u; // first block of the cell in the row
    double *p = buf + size_t(row) * ROW + off;
    if constexpr (MODE == 0) {
#pragma unroll
      for (int k = 0; k < 4; ++k) if (64 * k + lane < SPAN) unsafeAtomicAdd(p + 64 * k + lane, v);
    } else if constexpr (MODE == 1) {
#pragma unroll
      for (int k = 0; k < 4; ++k) if (64 * k + lane < SPAN) p[64 * k + lane] = v;
    } else if constexpr (MODE == 2) {
      double o[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = (64 * k + lane < SPAN) ? p[64 * k + lane] : 0.0;
#pragma unroll
      for (int k = 0; k < 4; ++k) if (64 * k + lane < SPAN) p[64 * k + lane] = o[k] + v;
    } else if constexpr (MODE == 3) {
      d2 o[2];
#pragma unroll
      for (int k = 0; k < 2; ++k) o[k] = (128 * k + 2 * lane < SPAN + 1) ? *reinterpret_cast<const d2 *>(p + 128 * k + 2 * lane) : d2{0, 0};
#pragma unroll
      for (int k = 0; k < 2; ++k) if (128 * k + 2 * lane < SPAN + 1) *reinterpret_cast<d2 *>(p + 128 * k + 2 * lane) = o[k] + d2{v, v};
    } else if constexpr (MODE == 4) {
#pragma unroll
      for (int k = 0; k < 2; ++k) if (128 * k + 2 * lane < SPAN + 1) *reinterpret_cast<d2 *>(p + 128 * k + 2 * lane) = d2{v, v};
    } else {
      // software pipeline over the rows: the values of row a + 1 are requested before the stores of row a
      d2 o[2];
      if (a == 0) {
#pragma unroll
        for (int k = 0; k < 2; ++k) o[k] = (128 * k + 2 * lane < SPAN + 1) ? *reinterpret_cast<const d2 *>(p + 128 * k + 2 * lane) : d2{0, 0};
      } else { o[0] = nxt; o[1] = d2{0, 0}; if (128 + 2 * lane < SPAN + 1) o[1] = *reinterpret_cast<const d2 *>(p + 128 + 2 * lane); }
      if (a + 1 < 27) {
        const unsigned h2 = hash32(cell * 27u + a + 1);
        const unsigned row2 = LOCAL ? (hash32(cell) % (n_rows - 256) + 8u * (a + 1) + (h2 & 7u)) : h2 % n_rows;
        const double *q = buf + size_t(row2) * ROW + (hash32(h2) % 98u) * 9u;
        nxt = *reinterpret_cast<const d2 *>(q + 2 * lane);
      }
#pragma unroll
      for (int k = 0; k < 2; ++k) if (128 * k + 2 * lane < SPAN + 1) *reinterpret_cast<d2 *>(p + 128 * k + 2 * lane) = o[k] + d2{v, v};
    }
  }
}

// The transpose of the above: one wavefront per OWNER (i, j, k) of the node lattice.  An owner has 8 nodes, (2i + {0,1}, 2j + {0,1},
// 2k + {0,1}), whose rows hold (5 or 3)^3 blocks: 125 | 75 75 75 | 45 45 45 | 27 = 512 blocks, touched by 8 | 4 4 4 | 2 2 2 | 1 = 27
// cells.  Each (row, cell) pair adds its 27 blocks into an image of the row in LDS at their (strided) positions inside the row; the
// complete image then leaves as plain contiguous stores of 16 bytes per lane and nobody else writes it.  The two nodes of one x pair
// are neighbours in memory, so one image holds both rows: 200 | 120 | 120 | 72 blocks, every one an even count of doubles.  Pair p of
// owner o lies at base[p] + o * size[p]: consecutive owners write adjacent memory, as the owners of one x line of the lattice do.
// ATOMIC: the LDS add is one ds_add_f64, otherwise a read, an add and a write.
constexpr int PAIR_MAX = 1800; // doubles in the largest image (vertex + x-edge node)

template <bool ATOMIC>
__global__ __launch_bounds__(128) void k_rows(double *buf, unsigned n_owners) {
  __shared__ __attribute__((aligned(16))) double img_all[2][PAIR_MAX];
  const unsigned w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const unsigned owner = blockIdx.x * 2 + w;
  const bool live = owner < n_owners;
  double *img = img_all[w];
  const double v = 1.0 + lane;
  // element e = 64 * k + lane of a pair's 243 values: column node (a, b, c) of the cell and component
  int ea[4], eb[4], ec[4], em[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) { const int e = 64 * k + int(lane), blk = e / 9; em[k] = e - 9 * blk; ea[k] = blk % 3; eb[k] = (blk / 3) % 3; ec[k] = blk / 9; }
  size_t base = 0;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    // extents of the column neighbourhood: 5 across an axis on which the node is a vertex, 3 where it is a cell midpoint
    const int ey = (p & 1) ? 3 : 5, ez = (p & 2) ? 3 : 5;
    const int n0 = 5 * ey * ez * 9, n1 = 3 * ey * ez * 9, n = n0 + n1; // doubles of the two rows
    for (int i = lane; i < n / 2; i += 64) reinterpret_cast<d2 *>(img)[i] = d2{0, 0};
    __syncthreads();
#pragma unroll
    for (int node = 0; node < 2; ++node) {
      const int ex = node ? 3 : 5;
      double *row = img + (node ? n0 : 0);
      // the cells of this node, one after the other: two per axis on which it is a vertex
      for (int cz = 0; cz < (ez == 5 ? 2 : 1); ++cz)
        for (int cy = 0; cy < (ey == 5 ? 2 : 1); ++cy)
          for (int cx = 0; cx < (ex == 5 ? 2 : 1); ++cx) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
              if (64 * k + int(lane) < SPAN) {
                double *q = row + 9 * ((2 * cx + ea[k]) + ex * ((2 * cy + eb[k]) + ey * (2 * cz + ec[k]))) + em[k];
                if constexpr (ATOMIC) unsafeAtomicAdd(q, v); else *q += v;
              }
            if constexpr (!ATOMIC) __syncthreads(); // the next cell of this node adds to some of the same blocks
          }
    }
    __syncthreads();
    if (live) {
      d2 *out = reinterpret_cast<d2 *>(buf + base + size_t(owner) * size_t(n));
      for (int i = lane; i < n / 2; i += 64) out[i] = reinterpret_cast<const d2 *>(img)[i];
    }
    __syncthreads();
    base += size_t(n_owners) * size_t(n);
  }
}

template <class F> float timeit(F f, int reps = 2) {
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  f(); CK(hipDeviceSynchronize());
  CK(hipEventRecord(e0)); for (int i = 0; i < reps; ++i) f(); CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
  float ms; CK(hipEventElapsedTime(&ms, e0, e1)); return ms / reps;
}

template <int MODE, bool LOCAL> void run(double *buf, unsigned n_rows, unsigned n_cells, const char *name) {
  const float ms = timeit([&] { hipLaunchKernelGGL((k_scatter<MODE, LOCAL>), dim3((n_cells + 1) / 2), dim3(128), 0, 0, buf, n_rows, n_cells); });
  const double bytes = double(n_cells) * 27 * SPAN * 8;
  printf("%-44s %-7s rows: %8.2f ms for %u cells = %6.2f TB/s of values, a 128^3 mesh (2.1 M cells) in %6.1f ms\n", name, LOCAL ? "nearby" : "random", ms, n_cells,
         bytes / ms / 1e9, ms * 2097152.0 / n_cells);
}

// one owner per cell of the mesh (a 128^3 mesh has 129^3 owners, the last plane of each axis with fewer rows): 512 blocks each
constexpr size_t OWNER = 512 * 9; // doubles one owner stores

template <bool ATOMIC> void run_rows(double *buf, unsigned n_owners, const char *name) {
  const float ms = timeit([&] { hipLaunchKernelGGL((k_rows<ATOMIC>), dim3((n_owners + 1) / 2), dim3(128), 0, 0, buf, n_owners); });
  printf("%-44s %-7s rows: %8.2f ms for %u owners = %5.2f TB/s stored, a 128^3 mesh (2.1 M cells) in %6.1f ms\n", name, "owned", ms, n_owners,
         double(n_owners) * OWNER * 8 / ms / 1e9, ms * 2097152.0 / n_owners);
}

int main() {
  const unsigned n_rows = 7000000; // x 9000 bytes = 63 GB
  double *buf; CK(hipMalloc(&buf, size_t(n_rows) * ROW * 8)); CK(hipMemset(buf, 0, size_t(n_rows) * ROW * 8));
  const unsigned n_cells = 1u << 20;
  static_assert(size_t(1u << 20) * OWNER <= size_t(7000000) * ROW, "the owners' rows fit the array");
  {
    const float ms = timeit([&] { CK(hipMemsetAsync(buf, 0, size_t(n_cells) * OWNER * 8, 0)); });
    printf("%-44s %-7s rows: %8.2f ms for %u owners = %5.2f TB/s, a 128^3 mesh (2.1 M cells) in %6.1f ms\n", "zero fill of the values the scatter adds to", "all", ms, n_cells,
           double(n_cells) * OWNER * 8 / ms / 1e9, ms * 2097152.0 / n_cells);
  }
  run_rows<true>(buf, n_cells, "27 x 27 blocks by ds_add_f64, rows stored");
  run_rows<false>(buf, n_cells, "27 x 27 blocks by LDS read-add-write, stored");
  run<0, false>(buf, n_rows, n_cells, "f64 atomics, 8 bytes per lane");
  run<1, false>(buf, n_rows, n_cells, "plain stores, 8 bytes per lane");
  run<4, false>(buf, n_rows, n_cells, "plain stores, 16 bytes per lane");
  run<2, false>(buf, n_rows, n_cells, "load + add + store, 8 bytes per lane");
  run<3, false>(buf, n_rows, n_cells, "load + add + store, 16 bytes per lane");
  run<5, false>(buf, n_rows, n_cells, "... next row's loads before the stores");
  run<0, true>(buf, n_rows, n_cells, "f64 atomics, 8 bytes per lane");
  run<1, true>(buf, n_rows, n_cells, "plain stores, 8 bytes per lane");
  run<4, true>(buf, n_rows, n_cells, "plain stores, 16 bytes per lane");
  run<2, true>(buf, n_rows, n_cells, "load + add + store, 8 bytes per lane");
  run<3, true>(buf, n_rows, n_cells, "load + add + store, 16 bytes per lane");
  run<5, true>(buf, n_rows, n_cells, "... next row's loads before the stores");
  return 0;
}
