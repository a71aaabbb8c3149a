// A point cloud in a dense grid, and sums over points in a fixed order: what the scan registrations (icp.h, gicp.h and their kernels)
// share.  Host- and device-compilable in the style of p3p.h and inertial_align.h: plain C++, nothing from HIP but the qualifiers.
//
//   PointGrid, grid_apply, grid_cell_of   the grid of one cloud; a point through a 3 x 4 transform; its cell
//   grid_visit_range                      the candidates of one range of sorted records against the best so far, by (d^2, index)
//   grid_near[_part]                      the nearest record within one cell edge: the fixed 9 ranges around the query (exact: see there)
//   grid_knn, grid_shell_nearest[_part]   the k nearest records / the nearest below a radius, through shells of cells (exact, any cell edge)
//   grid_plan, grid_build_serial          (host only) a cloud's bounding box -> its grid; the counting sort on one core
//   grid_wave_tree, grid_chunked_sums     (host only) the sums of per-point terms in the kernels' order of addition
//
// Bits.  Device and host must produce the same doubles (tests/test_gpu_register_scans*.py compare them bit for bit), so every function
// body switches floating-point contraction off (clang's pragma; a GCC build of this header passes -ffp-contract=off, which matters
// where the target has a fused multiply-add): a * b + c is two roundings on both sides, and fma() appears only where it is written.
// Division and square root are correctly rounded on both.  Sums over the points of a cloud are taken in a fixed order: points in chunks
// of kGridChunk; inside a chunk the tree of a 64-lane shuffle-down reduction per wave, the waves then in order; the chunks in order
// (grid_chunked_sums here, grid_chunk_reduce and grid_sum_partials in k_point_grid.h).  So a result depends neither on its neighbours
// in a batch nor on the launch.
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#if defined(__HIPCC__)
#define BSG_GRID_FN __host__ __device__ inline
#else
#define BSG_GRID_FN inline
#endif
#if defined(__clang__)
#define BSG_GRID_EXACT _Pragma("clang fp contract(off)")
#else
#define BSG_GRID_EXACT
#endif

namespace bsg {

constexpr int kGridChunk = 128;       // points per partial record (one workgroup); their sums: two waves' trees
constexpr int kGridWave = 64;
constexpr int kGridSub = 8;           // lanes that share one query's candidates in the kernels
constexpr double kGridEps = 2.220446049250313e-16;   // 2^-52

// The dense grid of one cloud: cell edge h, origin at the bounding box's lower corner, n cells per axis, x fastest.  The cells of all
// clouds of a call lie in one array, this cloud's from cell0; cell_end[c] is where cell c's records end in the sorted records of the
// whole call, and they begin where cell c - 1's end (at 0 for c == 0).  A record: 4 doubles (x, y, z, index within its cloud).
struct PointGrid {
  double o[3];
  double h;
  int n[3];
  int cell0;
};

// out = T p, T row-major 3 x 4.  (The only fused multiply-adds of the registration headers: written, so the same on both sides.)
BSG_GRID_FN void grid_apply(const double* T, const double* p, double* out) {
  out[0] = fma(T[0], p[0], fma(T[1], p[1], fma(T[2], p[2], T[3])));
  out[1] = fma(T[4], p[0], fma(T[5], p[1], fma(T[6], p[2], T[7])));
  out[2] = fma(T[8], p[0], fma(T[9], p[1], fma(T[10], p[2], T[11])));
}

// floor((x - o) / h) as a double: non-decreasing in x, which is all the searches below rely on
BSG_GRID_FN double grid_cell_f(double x, double o, double h) {
  BSG_GRID_EXACT
  return floor((x - o) / h);
}
BSG_GRID_FN int grid_clampi(double f, int n) { return f < 0.0 ? 0 : (f > (double)(n - 1) ? n - 1 : (int)f); }
// the cell (index into the call's cell array) of a point of the cloud; a point of the bounding box is never clamped
BSG_GRID_FN int grid_cell_of(const PointGrid& g, const double* q) {
  const int cx = grid_clampi(grid_cell_f(q[0], g.o[0], g.h), g.n[0]);
  const int cy = grid_clampi(grid_cell_f(q[1], g.o[1], g.h), g.n[1]);
  const int cz = grid_clampi(grid_cell_f(q[2], g.o[2], g.h), g.n[2]);
  return g.cell0 + (cz * g.n[1] + cy) * g.n[0] + cx;
}
// cells per axis of a bounding box [lo, hi]; as doubles, so that the product can be compared with a cap before it is an int
BSG_GRID_FN double grid_axis_cells(double lo, double hi, double h) { return grid_cell_f(hi, lo, h) + 1.0; }

// (d^2, index) is compared lexicographically, ties to the lowest index: a total order, so neither the order in which a cell was
// filled, nor the order in which candidates are visited, nor how they are dealt out to lanes can change a search's answer.
BSG_GRID_FN bool grid_better(double d2, double idx, double best, double bidx) { return d2 < best || (d2 == best && idx < bidx); }
BSG_GRID_FN double grid_dist2(const double* r, const double* x) {
  BSG_GRID_EXACT
  const double dx = r[0] - x[0], dy = r[1] - x[1], dz = r[2] - x[2];
  return dx * dx + dy * dy + dz * dz;
}
// the best record seen so far, squared distance in FP64; d2 and idx are +infinity while nothing was seen
struct GridBest {
  double d2, idx, x, y, z;
};
BSG_GRID_FN GridBest grid_no_best() {
  const double inf = std::numeric_limits<double>::infinity();
  return GridBest{inf, inf, 0.0, 0.0, 0.0};
}
// Records b + sub, b + sub + nsub, ... of the range [b, e) against m.  (A kernel gives a query to nsub neighbouring lanes, which
// read neighbouring 32-byte records, and merges their bests; on the host sub = 0, nsub = 1.)
BSG_GRID_FN void grid_visit_range(const double* rec, int b, int e, int sub, int nsub, const double* x, GridBest* m) {
  for (int p = b + sub; p < e; p += nsub) {
    const double* r = rec + 4 * (size_t)p;
    const double q[3] = {r[0], r[1], r[2]}, idx = r[3];      // (read once, before *m is written: one 32-byte load)
    const double d2 = grid_dist2(q, x);
    const bool better = grid_better(d2, idx, m->d2, m->idx);
    m->d2 = better ? d2 : m->d2; m->idx = better ? idx : m->idx;
    m->x = better ? q[0] : m->x; m->y = better ? q[1] : m->y; m->z = better ? q[2] : m->z;
  }
}

// ---- the nearest record within one cell edge: 9 ranges ------------------------------------------------------------------------------------
// The cells [lo, hi] of one axis that can hold a record within h of s; false: none.  A kept record has a COMPUTED d^2 <= h^2, hence
// |q - s| <= h up to rounding; the interval is widened by 4 ulp of (|s| + h) on each side, which covers that rounding and the one of
// s -+ h itself, and grid_cell_f is monotone.  So every record that can be kept lies in the cells searched: the search is exact, not
// approximate.  (In all but such rounding cases the interval is the three cells of the usual 3 x 3 x 3 neighbourhood.)
BSG_GRID_FN bool grid_axis_range(double s, double o, double h, int n, int* lo, int* hi) {
  BSG_GRID_EXACT
  const double pad = 4.0 * kGridEps * (fabs(s) + h);
  const double fl = grid_cell_f(s - h - pad, o, h), fh = grid_cell_f(s + h + pad, o, h);
  if (!(fh >= 0.0) || !(fl <= (double)(n - 1))) return false;
  *lo = grid_clampi(fl, n);
  *hi = grid_clampi(fh, n);
  return true;
}
// The nearest record of s among those that can lie within h = g.h of it.  A row of cells is contiguous in the sorted records: 9 ranges,
// not 27 cells.  grid_near_part is the search of one of nsub lanes and applies no threshold; grid_near keeps d^2 <= h2.
BSG_GRID_FN GridBest grid_near_part(const PointGrid& g, const int* cell_end, const double* rec, const double* s, int sub, int nsub) {
  GridBest m = grid_no_best();
  int x0 = 0, x1 = -1, y0 = 0, y1 = -1, z0 = 0, z1 = -1;
  const bool any = g.n[0] > 0 && g.n[1] > 0 && g.n[2] > 0 && grid_axis_range(s[0], g.o[0], g.h, g.n[0], &x0, &x1) &&
                   grid_axis_range(s[1], g.o[1], g.h, g.n[1], &y0, &y1) && grid_axis_range(s[2], g.o[2], g.h, g.n[2], &z0, &z1);
  if (any) {
    for (int z = z0; z <= z1; ++z) {
      for (int y = y0; y <= y1; ++y) {
        const int row = g.cell0 + (z * g.n[1] + y) * g.n[0];
        const int c0 = row + x0, c1 = row + x1;
        grid_visit_range(rec, c0 > 0 ? cell_end[c0 - 1] : 0, cell_end[c1], sub, nsub, s, &m);
      }
    }
  }
  return m;
}
BSG_GRID_FN bool grid_near(const PointGrid& g, const int* cell_end, const double* rec, const double* s, double h2, GridBest* m) {
  *m = grid_near_part(g, cell_end, rec, s, 0, 1);
  return m->d2 <= h2;
}

// ---- the shell search: any radius, any cell edge ------------------------------------------------------------------------------------------
// The query's cell, clamped into the grid per axis (a query may lie anywhere; a NaN goes to cell 0 and finds nothing).
BSG_GRID_FN int grid_query_clampi(double f, int n) { return !(f > 0.0) ? 0 : (f > (double)(n - 1) ? n - 1 : (int)f); }
BSG_GRID_FN void grid_query_cell(const PointGrid& g, const double* x, int* cx, int* cy, int* cz) {
  *cx = grid_query_clampi(grid_cell_f(x[0], g.o[0], g.h), g.n[0]);
  *cy = grid_query_clampi(grid_cell_f(x[1], g.o[1], g.h), g.n[1]);
  *cz = grid_query_clampi(grid_cell_f(x[2], g.o[2], g.h), g.n[2]);
}
// Shell r of cell (cx, cy, cz): the cells at Chebyshev distance exactly r.  Its part in row (cy + dy, cz + dz), as ranges of the
// sorted records: the whole span cx - r .. cx + r where |dy| == r or |dz| == r (one range: a row is contiguous), else the two cells
// cx - r and cx + r.  Returns the number of ranges (0 .. 2).
BSG_GRID_FN int grid_row_ranges(const PointGrid& g, const int* cell_end, int cx, int cy, int cz, int r, int dy, int dz, int* b0, int* e0, int* b1,
                                int* e1) {
  const int y = cy + dy, z = cz + dz;
  *b0 = *e0 = *b1 = *e1 = 0;
  if (y < 0 || y >= g.n[1] || z < 0 || z >= g.n[2]) return 0;
  const int row = g.cell0 + (z * g.n[1] + y) * g.n[0];
  const int xl = cx - r, xh = cx + r;
  if (dy == r || dy == -r || dz == r || dz == -r) {
    const int c0 = row + (xl < 0 ? 0 : xl), c1 = row + (xh > g.n[0] - 1 ? g.n[0] - 1 : xh);
    *b0 = c0 > 0 ? cell_end[c0 - 1] : 0; *e0 = cell_end[c1];
    return 1;
  }
  int n = 0;
  if (xl >= 0) { *b0 = row + xl > 0 ? cell_end[row + xl - 1] : 0; *e0 = cell_end[row + xl]; n = 1; }
  if (xh <= g.n[0] - 1) {
    const int b = cell_end[row + xh - 1], e = cell_end[row + xh];      // (xh >= 1 here: r >= 1)
    if (n == 0) { *b0 = b; *e0 = e; } else { *b1 = b; *e1 = e; }
    ++n;
  }
  return n;
}
// A lower bound of the distance from x to every point of the grid: the largest per-axis gap to the box of the cells.  A point of
// cell index <= m - 1 has floor(fl((q - o) / h)) < m, hence q < o + h m up to a few ulp; the pad covers that and the rounding of the
// edge itself (the rule of grid_axis_range, with a wider factor for the longer expression).
BSG_GRID_FN double grid_pad(double x, double o, double h, int m) {
  BSG_GRID_EXACT
  return 16.0 * kGridEps * (fabs(x) + fabs(o) + h * (double)(m + 1));
}
BSG_GRID_FN double grid_box_bound(const PointGrid& g, const double* x) {
  BSG_GRID_EXACT
  double D = 0.0;
  for (int a = 0; a < 3; ++a) {
    const double below = (g.o[a] - x[a]) - grid_pad(x[a], g.o[a], g.h, 0);
    const double above = (x[a] - (g.o[a] + g.h * (double)g.n[a])) - grid_pad(x[a], g.o[a], g.h, g.n[a]);
    D = below > D ? below : D;
    D = above > D ? above : D;
  }
  return D;
}
// A lower bound of the distance from x to every point of a cell outside shells 0 .. r of cell c: such a cell lies at index
// >= c + r + 1 or <= c - r - 1 on some axis.  +infinity: there is no such cell.  Never negative.
BSG_GRID_FN double grid_shell_bound(const PointGrid& g, const double* x, int cx, int cy, int cz, int r) {
  BSG_GRID_EXACT
  double D = std::numeric_limits<double>::infinity();
  const int c[3] = {cx, cy, cz};
  for (int a = 0; a < 3; ++a) {
    const int hi = c[a] + r + 1, lo = c[a] - r;
    if (hi <= g.n[a] - 1) {
      const double d = ((g.o[a] + g.h * (double)hi) - x[a]) - grid_pad(x[a], g.o[a], g.h, hi);
      D = d < D ? d : D;
    }
    if (lo >= 1) {
      const double d = (x[a] - (g.o[a] + g.h * (double)lo)) - grid_pad(x[a], g.o[a], g.h, lo);
      D = d < D ? d : D;
    }
  }
  return D < 0.0 ? 0.0 : D;
}

// The neighbour list of one query: k entries (d^2, index) in ascending lexicographic order, entry j at ld[j * stride], li[j * stride]
// (a kernel keeps the lists of a workgroup's points interleaved in LDS); +infinity where there is no entry yet.
BSG_GRID_FN void grid_list_insert(double* ld, double* li, int stride, int k, double d2, double idx) {
  if (!grid_better(d2, idx, ld[(k - 1) * stride], li[(k - 1) * stride])) return;
  int j = k - 1;
  while (j > 0 && grid_better(d2, idx, ld[(j - 1) * stride], li[(j - 1) * stride])) {
    ld[j * stride] = ld[(j - 1) * stride]; li[j * stride] = li[(j - 1) * stride];
    --j;
  }
  ld[j * stride] = d2; li[j * stride] = idx;
}
// The k nearest records of x by (d^2, index), no radius.  Shells of cells around x's cell are searched until the k-th best d^2 is
// below the squared bound of everything not yet searched: every record that could enter the list has then been seen, so the list is
// brute force's, whatever the cell edge.  Fewer than k records: the tail stays +infinity.
BSG_GRID_FN void grid_knn(const PointGrid& g, const int* cell_end, const double* rec, const double* x, int k, double* ld, double* li, int stride) {
  BSG_GRID_EXACT
  const double inf = std::numeric_limits<double>::infinity();
  for (int j = 0; j < k; ++j) { ld[j * stride] = inf; li[j * stride] = inf; }
  if (g.n[0] <= 0 || g.n[1] <= 0 || g.n[2] <= 0) return;
  int cx, cy, cz;
  grid_query_cell(g, x, &cx, &cy, &cz);
  const double box = grid_box_bound(g, x);
  for (int r = 0;; ++r) {
    const int z0 = -r < -cz ? -cz : -r, z1 = r > g.n[2] - 1 - cz ? g.n[2] - 1 - cz : r;
    const int y0 = -r < -cy ? -cy : -r, y1 = r > g.n[1] - 1 - cy ? g.n[1] - 1 - cy : r;
    for (int dz = z0; dz <= z1; ++dz) {
      for (int dy = y0; dy <= y1; ++dy) {
        int b0, e0, b1, e1;
        const int nr = grid_row_ranges(g, cell_end, cx, cy, cz, r, dy, dz, &b0, &e0, &b1, &e1);
        for (int w = 0; w < nr; ++w) {
          const int b = w == 0 ? b0 : b1, e = w == 0 ? e0 : e1;
          for (int p = b; p < e; ++p) {
            const double* q = rec + 4 * (size_t)p;
            grid_list_insert(ld, li, stride, k, grid_dist2(q, x), q[3]);
          }
        }
      }
    }
    const double shell = grid_shell_bound(g, x, cx, cy, cz, r);
    if (shell == inf) break;
    const double D = shell > box ? shell : box;
    if (ld[(k - 1) * stride] < D * D) break;
  }
}
// The nearest record of x by (d^2, index) among those with d^2 < mc2 (strict).  As grid_knn with k = 1; the search also ends when
// nothing not yet searched can lie below the threshold.  false: none (*m then holds the nearest seen, or nothing).
// grid_shell_nearest_part is the search of one of nsub lanes that share the query: after every shell `merge` leaves the best of all
// the lanes in each of them, so that they all take the same decision to go on.
struct GridNoMerge {
  BSG_GRID_FN void operator()(GridBest*) const {}
};
template <class Merge>
BSG_GRID_FN bool grid_shell_nearest_part(const PointGrid& g, const int* cell_end, const double* rec, const double* x, double mc2, int sub, int nsub,
                                         Merge merge, GridBest* out) {
  BSG_GRID_EXACT
  const double inf = std::numeric_limits<double>::infinity();
  GridBest m = grid_no_best();
  if (g.n[0] > 0 && g.n[1] > 0 && g.n[2] > 0) {
    int cx, cy, cz;
    grid_query_cell(g, x, &cx, &cy, &cz);
    const double box = grid_box_bound(g, x);
    for (int r = 0; box * box < mc2; ++r) {
      const int z0 = -r < -cz ? -cz : -r, z1 = r > g.n[2] - 1 - cz ? g.n[2] - 1 - cz : r;
      const int y0 = -r < -cy ? -cy : -r, y1 = r > g.n[1] - 1 - cy ? g.n[1] - 1 - cy : r;
      for (int dz = z0; dz <= z1; ++dz) {
        for (int dy = y0; dy <= y1; ++dy) {
          int b0, e0, b1, e1;
          const int nr = grid_row_ranges(g, cell_end, cx, cy, cz, r, dy, dz, &b0, &e0, &b1, &e1);
          for (int w = 0; w < nr; ++w) grid_visit_range(rec, w == 0 ? b0 : b1, w == 0 ? e0 : e1, sub, nsub, x, &m);
        }
      }
      merge(&m);
      const double shell = grid_shell_bound(g, x, cx, cy, cz, r);
      if (shell == inf) break;
      const double D = shell > box ? shell : box;
      if (m.d2 < D * D || !(D * D < mc2)) break;
    }
  }
  *out = m;
  return m.d2 < mc2;
}
BSG_GRID_FN bool grid_shell_nearest(const PointGrid& g, const int* cell_end, const double* rec, const double* x, double mc2, GridBest* m) {
  return grid_shell_nearest_part(g, cell_end, rec, x, mc2, 0, 1, GridNoMerge(), m);
}

// ---- host only: a cloud's grid --------------------------------------------------------------------------------------------------------------
// The grid of n points (each under the 3 x 4 transform T when one is given) with cell edge h, its cells from cell0: the bounding box,
// the cells per axis and their product *cells, by the arithmetic the device uses.  The product is compared with max_cells as a
// double, before any of it is an int; g->n is set only when the grid is accepted.  No points: no cells.
enum GridPlan { kGridOk = 0, kGridNotFinite, kGridTooManyCells };
inline GridPlan grid_plan(int n, const double* pts, const double* T, double h, int cell0, double max_cells, PointGrid* g, double* cells) {
  g->h = h; g->cell0 = cell0;
  for (int a = 0; a < 3; ++a) { g->o[a] = 0.0; g->n[a] = 0; }
  *cells = 0.0;
  if (n == 0) return kGridOk;
  double lo[3], hi[3], q[3];
  for (int i = 0; i < n; ++i) {
    const double* p = pts + 3 * (size_t)i;
    if (T) grid_apply(T, p, q);
    for (int a = 0; a < 3; ++a) {
      const double v = T ? q[a] : p[a];
      lo[a] = i == 0 || v < lo[a] ? v : lo[a]; hi[a] = i == 0 || v > hi[a] ? v : hi[a];
    }
  }
  double nc[3], here = 1.0;
  for (int a = 0; a < 3; ++a) {
    if (!std::isfinite(lo[a]) || !std::isfinite(hi[a])) return kGridNotFinite;
    nc[a] = grid_axis_cells(lo[a], hi[a], h);
    here *= nc[a];
  }
  if (!(here <= max_cells)) return kGridTooManyCells;
  *cells = here;
  for (int a = 0; a < 3; ++a) { g->o[a] = lo[a]; g->n[a] = (int)nc[a]; }
  return kGridOk;
}

struct SerialGrid {
  PointGrid g;
  std::vector<int> cell_end;
  std::vector<double> rec;
};
// The grid of one cloud (already in the frame it is searched in) by a counting sort; false: more than max_cells cells.
inline bool grid_build_serial(int n, const double* q, double h, double max_cells, SerialGrid* G) {
  PointGrid& g = G->g;
  double cells;
  G->cell_end.clear(); G->rec.assign(4 * (size_t)n, 0.0);
  if (grid_plan(n, q, nullptr, h, 0, max_cells, &g, &cells) != kGridOk) return false;
  if (n == 0) return true;
  std::vector<int>& ce = G->cell_end;
  ce.assign((size_t)(g.n[0] * g.n[1] * g.n[2]), 0);
  for (int i = 0; i < n; ++i) ++ce[grid_cell_of(g, q + 3 * i)];
  int run = 0;
  for (int& c : ce) { const int k = c; c = run; run += k; }      // starts; the scatter below turns them into ends
  for (int i = 0; i < n; ++i) {
    double* r = &G->rec[4 * (size_t)ce[grid_cell_of(g, q + 3 * i)]++];
    r[0] = q[3 * i]; r[1] = q[3 * i + 1]; r[2] = q[3 * i + 2]; r[3] = (double)i;
  }
  return true;
}

// ---- host only: the fixed-order sums --------------------------------------------------------------------------------------------------------
// lane 0's value of a shuffle-down reduction over the 64 values v[0], v[stride], ...: offsets 32, 16, .., 1
inline double grid_wave_tree(double* v, int stride) {
  BSG_GRID_EXACT
  for (int off = kGridWave / 2; off >= 1; off /= 2)
    for (int i = 0; i < off; ++i) v[i * stride] = v[i * stride] + v[(i + off) * stride];
  return v[0];
}
// sum[0 .. REC) of the terms of points 0 .. n - 1 in the order of the kernels (see "Bits"); term(i, r) writes point i's REC terms
template <int REC, class Term>
inline void grid_chunked_sums(int n, Term term, double* sum) {
  BSG_GRID_EXACT
  std::vector<double> lanes((size_t)kGridChunk * REC);
  for (int t = 0; t < REC; ++t) sum[t] = 0.0;
  for (int c = 0; c < n; c += kGridChunk) {
    for (int l = 0; l < kGridChunk; ++l) {
      double* r = &lanes[(size_t)l * REC];
      if (c + l < n) term(c + l, r);
      else for (int t = 0; t < REC; ++t) r[t] = 0.0;
    }
    for (int t = 0; t < REC; ++t) {
      double part = 0.0;
      for (int w = 0; w < kGridChunk / kGridWave; ++w) part = part + grid_wave_tree(&lanes[(size_t)w * kGridWave * REC + t], REC);
      sum[t] = sum[t] + part;
    }
  }
}

}  // namespace bsg
