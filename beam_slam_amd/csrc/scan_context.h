// Scan Context place recognition (bsgpu_scan_context_describe / bsgpu_scan_context_match, k_scan_context.hip): the descriptor and the
// search of RelocCandidateSearchScanContext::FindRelocCandidates (bs_models/src/lib/reloc/reloc_candidate_search_scan_context.cpp:117-150),
// as include/bsgpu.h pins them.  SCManager is libbeam's copy of the published Scan Context code (Kim & Kim, IROS 2018) and is not in the
// reference checkout: makeScancontext, fastAlignUsingVkey, distDirectSC and detectLoopClosureID are RECALLED, not verified.
// Host- and device-compilable in the style of icp.h: plain C++, nothing from HIP but the qualifiers.
//
// Shared by the kernels, the CPU test program (tests/plan/test_scan_context.cpp), the host stand-in's test back-end
// (tests/host/test_host_reloc.cpp) and the one-core timing (scripts/time_scan_context_cpu.cpp):
//   sc_transform, sc_sector, sc_bin      a point through a 3 x 4 transform; its sector, its bin
//   sc_key_of, sc_value_of               a bin value as an order-preserving 64-bit integer (0: empty) and back
//   sc_mean20, sc_norm20, sc_dot20       the 20-term sums: a chain in ring order
//   sc_tree64                            the 60-term sums: the tree of a 64-lane xor butterfly, positions 60..63 zero
//   sc_describe_serial, sc_match_serial  (host only) the two entry points on one core, in the kernels' order of addition
//
// Bits.  Device and host must produce the same doubles (tests/test_gpu_scan_context.py compares them bit for bit), so every function
// body switches floating-point contraction off (clang's pragma; a GCC build passes -ffp-contract=off): a * b + c is two roundings on
// both sides.  Division and square root are correctly rounded on both.  No function of libm whose last place differs between the two
// sides is called: the sector is decided by comparisons (sc_sector), never by atan.  A bin is a maximum, which has no order.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

#if defined(__HIPCC__)
#define BSG_SC_FN __host__ __device__ inline
#else
#define BSG_SC_FN inline
#endif
#if defined(__clang__)
#define BSG_SC_EXACT _Pragma("clang fp contract(off)")
#define BSG_SC_UNROLL _Pragma("unroll")
#else
#define BSG_SC_EXACT
#define BSG_SC_UNROLL
#endif

namespace bsg {

constexpr int kScRings = 20;                 // BSGPU_SC_RINGS
constexpr int kScSectors = 60;               // BSGPU_SC_SECTORS
constexpr int kScBins = kScRings * kScSectors;
constexpr int kScChunk = 4096;               // points of a member that one workgroup of sc_bin_kernel bins
constexpr int kScMaxTree = 64;               // BSGPU_SC_MAX_TREE_CANDIDATES
constexpr int kScMaxCandidates = 65536;      // BSGPU_SC_MAX_CANDIDATES
constexpr int kScMaxScanPoints = 65535 * kScChunk;   // BSGPU_SC_MAX_SCAN_POINTS: a scan's chunks are one axis of sc_bin_kernel's grid
constexpr double kScYawStep = 6.283185307179586 / 60.0;   // one sector in radians

// out = T p, T row-major 3 x 4: ((T0 x + T1 y) + T2 z) + T3 per row, every product and sum rounded
BSG_SC_FN void sc_transform(const double* T, const double* p, double* out) {
  BSG_SC_EXACT
  out[0] = ((T[0] * p[0] + T[1] * p[1]) + T[2] * p[2]) + T[3];
  out[1] = ((T[4] * p[0] + T[5] * p[1]) + T[6] * p[2]) + T[7];
  out[2] = ((T[8] * p[0] + T[9] * p[1]) + T[10] * p[2]) + T[11];
}

// tan(6 m degrees), m = 1 .. 7 (to 17 digits).  The seven boundaries above 45 degrees use the same constants through
// tan(90 - a) = 1 / tan(a), written as a comparison of the other coordinate: 14 boundaries below 90 degrees, 7 constants.
BSG_SC_FN double sc_tan6(int m) {
  switch (m) {
    case 1: return 0.10510423526567646;
    case 2: return 0.21255656167002213;
    case 3: return 0.32491969623290632;
    case 4: return 0.44522868530853616;
    case 5: return 0.57735026918962576;
    case 6: return 0.72654252800536089;
    default: return 0.90040404429783994;
  }
}

// How many of the boundaries 0, 6, .., 84 degrees lie strictly below the angle of (a, b), a >= 0 along the quadrant's first axis and
// b >= 0 along its second, not both zero: 0 on the first axis itself, 15 above 84 degrees.  Comparisons of rounded products only.
BSG_SC_FN int sc_quadrant_count(double a, double b) {
  BSG_SC_EXACT
  int c;
  if (b <= a) {                // [0, 45] degrees: 6 m degrees is below iff b > tan(6 m) a
    c = b > 0.0 ? 1 : 0;
BSG_SC_UNROLL
    for (int m = 1; m <= 7; ++m) c += b > sc_tan6(m) * a ? 1 : 0;
  } else {                     // (45, 90]: 0 .. 42 are below; 90 - 6 m degrees is below iff a < tan(6 m) b
    c = 8;
BSG_SC_UNROLL
    for (int m = 1; m <= 7; ++m) c += a < sc_tan6(m) * b ? 1 : 0;
  }
  return c;
}

// The sector of (x, y): k for an azimuth in (6 k, 6 (k + 1)] degrees, counter-clockwise from +x; azimuth 0 and the origin: sector 0.
// This function's decision is the contract at a boundary.
BSG_SC_FN int sc_sector(double x, double y) {
  const double ax = fabs(x), ay = fabs(y);
  int c;
  if (x > 0.0 && y >= 0.0) c = sc_quadrant_count(ax, ay);                // [0, 90)
  else if (x <= 0.0 && y > 0.0) c = 15 + sc_quadrant_count(ay, ax);      // [90, 180)
  else if (x < 0.0 && y <= 0.0) c = 30 + sc_quadrant_count(ax, ay);      // [180, 270)
  else if (x >= 0.0 && y < 0.0) c = 45 + sc_quadrant_count(ay, ax);      // [270, 360)
  else c = 0;                                                            // the origin
  return c > 0 ? c - 1 : 0;
}

// The bin (ring * 60 + sector) of a point, -1: dropped (r > max_radius, or r not a number: a transform took the point out of range)
BSG_SC_FN int sc_bin(double x, double y, double max_radius) {
  BSG_SC_EXACT
  const double r = sqrt(x * x + y * y);
  if (!(r <= max_radius)) return -1;
  const double f = ceil(r / max_radius * (double)kScRings);
  const int ring = f < 1.0 ? 0 : (f > (double)kScRings ? kScRings - 1 : (int)f - 1);
  return ring * kScSectors + sc_sector(x, y);
}

// A finite double as an unsigned integer of the same order; never 0, which marks the empty bin.
BSG_SC_FN unsigned long long sc_key_of(double v) {
  unsigned long long b;
  memcpy(&b, &v, 8);
  return (b >> 63) != 0 ? ~b : (b | 0x8000000000000000ull);
}
BSG_SC_FN double sc_value_of(unsigned long long k) {
  if (k == 0) return 0.0;
  const unsigned long long b = (k >> 63) != 0 ? (k & 0x7fffffffffffffffull) : ~k;
  double v;
  memcpy(&v, &b, 8);
  return v;
}
// what a point contributes to its bin (z + lidar_height); false: not finite, the point is dropped
BSG_SC_FN bool sc_point_value(double z, double lidar_height, double* v) {
  BSG_SC_EXACT
  *v = z + lidar_height;
  return *v - *v == 0.0;
}

// ---- the 20-term sums: a chain in ring order over a column (stride: distance between rings) -------------------------------------------
BSG_SC_FN double sc_mean20(const double* c, int stride) {
  BSG_SC_EXACT
  double s = 0.0;
BSG_SC_UNROLL
  for (int r = 0; r < kScRings; ++r) s = s + c[r * stride];
  return s / (double)kScRings;
}
BSG_SC_FN double sc_norm20(const double* c, int stride) {
  BSG_SC_EXACT
  double s = 0.0;
BSG_SC_UNROLL
  for (int r = 0; r < kScRings; ++r) s = s + c[r * stride] * c[r * stride];
  return sqrt(s);
}
BSG_SC_FN double sc_dot20(const double* a, int stride_a, const double* b, int stride_b) {
  BSG_SC_EXACT
  double s = 0.0;
BSG_SC_UNROLL
  for (int r = 0; r < kScRings; ++r) s = s + a[r * stride_a] * b[r * stride_b];
  return s;
}
BSG_SC_FN double sc_sq_diff(double a, double b) {
  BSG_SC_EXACT
  const double d = a - b;
  return d * d;
}
// cosine of two columns from their dot product and norms
BSG_SC_FN double sc_cosine(double dot, double na, double nb) {
  BSG_SC_EXACT
  return dot / (na * nb);
}
// the distance of one shift from the sum of the cosines of its n columns
BSG_SC_FN double sc_shift_distance(double sum, int n) {
  BSG_SC_EXACT
  return n > 0 ? 1.0 - sum / (double)n : std::numeric_limits<double>::infinity();
}
// R of the refinement window: round(0.5 search_ratio 60), 30 and above meaning all 60 shifts
BSG_SC_FN int sc_search_radius(double search_ratio) {
  BSG_SC_EXACT
  const double r = floor(0.5 * search_ratio * (double)kScSectors + 0.5);
  return r >= 30.0 ? 30 : (int)r;
}
// What is compared is never a NaN.  Finite descriptor entries near the ends of the FP64 range can make one (a sum that overflows, then
// inf - inf; a product of norms that underflows, then 0 / 0); as +infinity it takes its place in the order, the same on both sides.
BSG_SC_FN double sc_orderable(double d) { return d == d ? d : std::numeric_limits<double>::infinity(); }
BSG_SC_FN bool sc_in_window(int s, int shift0, int R) {
  int d = s - shift0;
  d = d < 0 ? d + kScSectors : d;
  d = d > kScSectors - d ? kScSectors - d : d;
  return d <= R;
}
BSG_SC_FN int sc_wrap(int j) { return j >= kScSectors ? j - kScSectors : j; }
// (d, index) pairs in lexicographic order
BSG_SC_FN bool sc_less(double da, long long ia, double db, long long ib) { return da < db || (da == db && ia < ib); }

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the 60-term sums: v[0 .. 59] the terms, v[60 .. 63] zero; the tree of the kernels' xor butterfly (32, 16, .., 1) -----------------
inline double sc_tree64(double* v) {
  BSG_SC_EXACT
  for (int off = 32; off >= 1; off >>= 1)
    for (int i = 0; i < off; ++i) v[i] = v[i] + v[i + off];
  return v[0];
}
inline double sc_tree60(const double* terms, int stride) {
  double v[64];
  for (int i = 0; i < 64; ++i) v[i] = i < kScSectors ? terms[i * stride] : 0.0;
  return sc_tree64(v);
}
// ring key (20) and sector key (60) of a descriptor (ring-major 20 x 60); either may be null
inline void sc_keys(const double* desc, double* ring_key, double* sector_key) {
  BSG_SC_EXACT
  if (ring_key) for (int r = 0; r < kScRings; ++r) ring_key[r] = sc_tree60(desc + r * kScSectors, 1) / (double)kScSectors;
  if (sector_key) for (int j = 0; j < kScSectors; ++j) sector_key[j] = sc_mean20(desc + j, kScSectors);
}

// bsgpu_scan_context_describe on one core; arguments as the entry point's, already checked; the optional outputs may be null
inline void sc_describe_serial(const int32_t* scan_start, const double* points, int32_t n_aggregates, const int32_t* member_start,
                               const int32_t* member_scan, const double* member_T, double lidar_height, double max_radius, double* desc,
                               double* ring_key, double* sector_key, int32_t* n_binned) {
  static const double eye[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  std::vector<unsigned long long> table(kScBins);
  for (int a = 0; a < n_aggregates; ++a) {
    std::fill(table.begin(), table.end(), 0ull);
    int kept = 0;
    for (int m = member_start[a]; m < member_start[a + 1]; ++m) {
      const double* T = member_T ? member_T + 12 * (size_t)m : eye;
      const int sc = member_scan[m];
      for (size_t i = (size_t)scan_start[sc]; i < (size_t)scan_start[sc + 1]; ++i) {
        double q[3], v;
        sc_transform(T, points + 3 * i, q);
        const int b = sc_bin(q[0], q[1], max_radius);
        if (b < 0 || !sc_point_value(q[2], lidar_height, &v)) continue;
        const unsigned long long k = sc_key_of(v);
        table[b] = k > table[b] ? k : table[b];
        ++kept;
      }
    }
    double* d = desc + (size_t)kScBins * a;
    for (int b = 0; b < kScBins; ++b) d[b] = sc_value_of(table[b]);
    sc_keys(d, ring_key ? ring_key + (size_t)kScRings * a : nullptr, sector_key ? sector_key + (size_t)kScSectors * a : nullptr);
    if (n_binned) n_binned[a] = kept;
  }
}

// one (query, candidate) comparison: qd / cd the descriptors, qk / ck their sector keys, qn / cn their column norms -> distance, shift.
// The tree's position i is the candidate's column i, which meets the query's column (i + s) mod 60 under shift s.
inline void sc_compare(const double* qd, const double* qk, const double* qn, const double* cd, const double* ck, const double* cn, int R,
                       double* dist, int* shift) {
  double v[64];
  double best = std::numeric_limits<double>::infinity();
  int shift0 = 0;
  for (int s = 0; s < kScSectors; ++s) {
    for (int i = 0; i < 64; ++i) v[i] = i < kScSectors ? sc_sq_diff(qk[sc_wrap(i + s)], ck[i]) : 0.0;
    const double n2 = sc_orderable(sc_tree64(v));   // the squared norm: its minimum is the norm's
    if (n2 < best) { best = n2; shift0 = s; }
  }
  double bd = std::numeric_limits<double>::infinity();
  int bs = -1;
  for (int s = 0; s < kScSectors; ++s) {
    if (!sc_in_window(s, shift0, R)) continue;
    if (bs < 0) bs = s;
    int n = 0;
    for (int i = 0; i < 64; ++i) {
      v[i] = 0.0;
      if (i >= kScSectors) continue;
      const int j = sc_wrap(i + s);
      if (qn[j] == 0.0 || cn[i] == 0.0) continue;
      v[i] = sc_cosine(sc_dot20(qd + j, kScSectors, cd + i, kScSectors), qn[j], cn[i]);
      ++n;
    }
    const double d = sc_orderable(sc_shift_distance(sc_tree64(v), n));
    if (d < bd) { bd = d; bs = s; }
  }
  *dist = bd; *shift = bs;
}

// bsgpu_scan_context_match on one core; arguments as the entry point's, already checked; yaw, dist_all and shift_all may be null
inline void sc_match_serial(int32_t n_sets, const int32_t* query_start, const double* query_desc, const int32_t* cand_start,
                            const double* cand_desc, int32_t n_tree_candidates, double search_ratio, double dist_thres, int32_t* best_cand,
                            double* best_dist, int32_t* best_shift, double* yaw, double* dist_all, int32_t* shift_all) {
  BSG_SC_EXACT
  const double inf = std::numeric_limits<double>::infinity();
  const int R = sc_search_radius(search_ratio);
  size_t pair0 = 0;
  for (int s = 0; s < n_sets; ++s) {
    const int c0 = cand_start[s], nc = cand_start[s + 1] - c0;
    std::vector<double> ck((size_t)nc * kScSectors), cn((size_t)nc * kScSectors), crk((size_t)nc * kScRings);
    for (int c = 0; c < nc; ++c) {
      const double* cd = cand_desc + (size_t)kScBins * (c0 + c);
      sc_keys(cd, &crk[(size_t)c * kScRings], &ck[(size_t)c * kScSectors]);
      for (int j = 0; j < kScSectors; ++j) cn[(size_t)c * kScSectors + j] = sc_norm20(cd + j, kScSectors);
    }
    const bool select = n_tree_candidates > 0 && n_tree_candidates < nc;
    for (int q = query_start[s]; q < query_start[s + 1]; ++q, pair0 += (size_t)nc) {
      const double* qd = query_desc + (size_t)kScBins * q;
      double qrk[kScRings], qk[kScSectors], qn[kScSectors];
      sc_keys(qd, qrk, qk);
      for (int j = 0; j < kScSectors; ++j) qn[j] = sc_norm20(qd + j, kScSectors);
      std::vector<char> take((size_t)nc, select ? 0 : 1);
      if (select) {
        std::vector<double> d2((size_t)nc);
        for (int c = 0; c < nc; ++c) {
          double acc = 0.0;
          for (int r = 0; r < kScRings; ++r) acc = acc + sc_sq_diff(qrk[r], crk[(size_t)c * kScRings + r]);
          d2[c] = sc_orderable(acc);
        }
        for (int k = 0; k < n_tree_candidates; ++k) {
          int pick = -1;
          for (int c = 0; c < nc; ++c) if (!take[c] && (pick < 0 || sc_less(d2[c], c, d2[pick], pick))) pick = c;
          take[pick] = 1;
        }
      }
      double bd = inf;
      int bc = -1, bs = 0;
      for (int c = 0; c < nc; ++c) {
        double d = inf;
        int sh = 0;
        if (take[c])
          sc_compare(qd, qk, qn, cand_desc + (size_t)kScBins * (c0 + c), &ck[(size_t)c * kScSectors], &cn[(size_t)c * kScSectors], R, &d, &sh);
        if (dist_all) dist_all[pair0 + c] = d;
        if (shift_all) shift_all[pair0 + c] = sh;
        if (take[c] && (bc < 0 || d < bd)) { bd = d; bc = c; bs = sh; }
      }
      best_cand[q] = bc >= 0 && bd < dist_thres ? bc : -1;
      best_dist[q] = bd;
      best_shift[q] = bs;
      if (yaw) yaw[q] = (double)bs * kScYawStep;
    }
  }
}
#endif  // !__HIP_DEVICE_COMPILE__

}  // namespace bsg
