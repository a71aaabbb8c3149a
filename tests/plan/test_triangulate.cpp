// Driver of beam_slam_amd/csrc/triangulate_core.h on the CPU for tests/test_triangulation_hp.py: reads commands from a file and prints
// what the header computes, one bsgpu_triangulate call per command.
//   TRACKS <n_tracks> <n_obs> <n_values> <truncate> <max_dist> <max_reproj>, followed by
//          <16 doubles: fx fy cx cy R_cam_baselink[9] t_cam_baselink[3]>, <n_values doubles: the values>,
//          <n_tracks + 1 ints: track_start>, then n_obs lines <q_offset p_offset u v>
//          -> n_tracks lines PT <case> <track> <status> <3 doubles>
#include <cstdio>
#include <cstring>
#include <vector>

#include "triangulate_core.h"

namespace {
struct Cam { double fx, fy, cx, cy, R[9], t[3]; };
struct Off { int x, y; };
struct Pix { double x, y; };
}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  char cmd[16];
  int count = 0;
  while (std::fscanf(f, "%15s", cmd) == 1) {
    if (!std::strcmp(cmd, "TRACKS")) {
      int n, n_obs, n_val, truncate;
      double max_dist, max_reproj;
      if (std::fscanf(f, "%d %d %d %d %lf %lf", &n, &n_obs, &n_val, &truncate, &max_dist, &max_reproj) != 6) return 3;
      if (n < 0 || n_obs < 0 || n_val < 0) return 3;
      Cam cam;
      double c[16];
      for (double& v : c) if (std::fscanf(f, "%lf", &v) != 1) return 3;
      cam.fx = c[0]; cam.fy = c[1]; cam.cx = c[2]; cam.cy = c[3];
      for (int i = 0; i < 9; ++i) cam.R[i] = c[4 + i];
      for (int i = 0; i < 3; ++i) cam.t[i] = c[13 + i];
      std::vector<double> x(n_val);
      for (double& v : x) if (std::fscanf(f, "%lf", &v) != 1) return 3;
      std::vector<int> start(n + 1);
      for (int& v : start) if (std::fscanf(f, "%d", &v) != 1) return 3;
      std::vector<Off> off(n_obs);
      std::vector<Pix> pix(n_obs);
      for (int o = 0; o < n_obs; ++o) {
        if (std::fscanf(f, "%d %d %lf %lf", &off[o].x, &off[o].y, &pix[o].x, &pix[o].y) != 4) return 3;
        if (off[o].x < 0 || off[o].x + 4 > n_val || off[o].y < 0 || off[o].y + 3 > n_val) return 3;
      }
      for (int l = 0; l < n; ++l) {
        if (start[l] < 0 || start[l + 1] < start[l] || start[l + 1] > n_obs) return 3;
        double P[3];
        const int st = bsg::triangulate_track(start[l], start[l + 1], off.data(), pix.data(), x.data(), cam, truncate, max_dist, max_reproj, P);
        std::printf("PT %d %d %d %.17g %.17g %.17g\n", count, l, st, P[0], P[1], P[2]);
      }
    } else {
      return 4;
    }
    ++count;
  }
  std::fclose(f);
  std::printf("DONE %d\n", count);
  return 0;
}
