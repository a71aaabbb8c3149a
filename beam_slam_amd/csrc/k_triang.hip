// Landmark triangulation for a batch of feature tracks — the factor producer that creates the Point3DLandmark
// blocks the reprojection factors attach to.  Follows the reference's call sites
//   VisualOdometry::TriangulateLandmark      bs_models/src/visual_odometry.cpp:532-610
//   SLAMInitialization::TriangulateLandmark  bs_models/src/slam_initialization.cpp:699-701
// which collect, per track, T_camera_world = (T_world_baselink * T_cam_baselink^-1)^-1 of every keyframe of the
// track that is in the graph (VisualMap::GetCameraPose, bs_models/src/lib/vision/visual_map.cpp:43-54) and the
// measured pixel truncated to integers (`m.value.cast<int>()`, visual_odometry.cpp:547), demand >= 2 views (:572)
// and call [EXT] beam_cv::Triangulation::TriangulatePoint(cam, T_cam_world, pixels, max_dist, max_reprojection).
// libbeam is not under /root/reference (un-vendored, version unpinned); its published algorithm,
// restated here: back-project each pixel to a unit bearing m, stack the two DLT rows
//      m.x * T.row(2) - m.z * T.row(0),   m.y * T.row(2) - m.z * T.row(1)
// per view into A (2V x 4), take the right singular vector of the smallest singular value, de-homogenise, and
// reject the point if in any view it is behind the camera, farther than max_dist (> 0) or re-projects more than
// max_reprojection (> 0) pixels from the measurement.  The camera is the skew-free pinhole (K of the camera table)
// the reprojection factors themselves use.
//
// One lane per track (triangulate_core.h, shared with the CPU tests): the rows of A are rotated into a 4x4 triangular factor as
// they are formed and the singular vector comes from one-sided Jacobi on that factor (all indices compile-time => registers) — not
// from the Gram matrix A^T A, whose eigenvector is only good to cond(A)^2 * 1e-16 and cond(A) grows with the distance from the world
// origin.  Streamed per view: 8 B of offsets + 16 B pixel; the keyframe poses are gathered (L2-resident: a window has a few
// hundred of them).  HBM-bound, ~24 B/view + 28 B/track out.
#include "bsgpu_device.h"
#include "triangulate_core.h"

namespace bsg {

// status: 0 = triangulated; 1 = fewer than 2 views; 2 = behind a camera; 3 = farther than max_dist;
//         4 = re-projection above max_reproj; 5 = point at infinity (homogeneous w == 0)
__global__ __launch_bounds__(256) void triangulate_kernel(int n_tracks, const int* __restrict__ track_start,
                                                          const int2* __restrict__ pose_off, const double2* __restrict__ pix,
                                                          const double* __restrict__ x, DevCamera cam, int truncate,
                                                          double max_dist, double max_reproj, double* __restrict__ points,
                                                          int* __restrict__ status) {
  const int l = blockIdx.x * 256 + threadIdx.x;
  if (l >= n_tracks) return;
  double P[3];
  const int st = triangulate_track(track_start[l], track_start[l + 1], pose_off, pix, x, cam, truncate, max_dist, max_reproj, P);
  points[3 * (size_t)l] = P[0]; points[3 * (size_t)l + 1] = P[1]; points[3 * (size_t)l + 2] = P[2];
  status[l] = st;
}

void launch_triangulate(hipStream_t s, int n_tracks, const int* track_start, const int2* pose_off, const double2* pix, const double* x,
                        const DevCamera& cam, bool truncate, double max_dist, double max_reproj, double* points, int* status) {
  if (n_tracks <= 0) return;
  hipLaunchKernelGGL(triangulate_kernel, dim3((n_tracks + 255) / 256), dim3(256), 0, s, n_tracks, track_start, pose_off, pix, x, cam,
                     truncate ? 1 : 0, max_dist, max_reproj, points, status);
}

}  // namespace bsg
