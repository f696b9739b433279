// pose_covariance.h — host-side types of the pose covariance (include/vo_hip.h: vo_gn_pose_information_*,
// vo_svo_set_pose_covariance, vo_mvo_set_pose_covariance). Row-major 6x6 doubles, order xi = [rho; phi].
#ifndef VO_AMD_POSE_COVARIANCE_H_
#define VO_AMD_POSE_COVARIANCE_H_

#include <array>
#include <cstddef>

namespace vo {

using Mat66d = std::array<double, 36>;

// of a pose-only BA's result: H = sum w J J^T, Sigma = s2 H^-1 (T10_true ~ exp(eps) T10_est, eps ~ N(0, Sigma))
struct PoseInformation {
  Mat66d H{}, Sigma{};
  double s2 = 0.0;
  bool valid = false;
};

// of a driver's pose: P_k = Ad(T10,k) P_k-1 Ad(T10,k)^T + Sigma_xi,k (T_wc_true ~ T_wc_est exp(-e), e ~ N(0, P))
struct PoseCovariance {
  Mat66d P{}, Sigma_xi{};
  double s2 = 0.0;
  bool valid = false;
  int n_points = 0, n_unknown_steps = 0;
};

// nav_msgs::Odometry::pose.covariance: C = B P B^T, B = blkdiag(R_wc, R_wc); order (x, y, z, rot x, rot y, rot z), row-major.
// T_wc: row-major 4x4.
template <typename Pose>
inline std::array<double, 36> poseCovarianceRos(const Mat66d &P, const Pose &T_wc) {
  double B[6][6] = {}, T[6][6] = {};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) B[i][j] = B[3 + i][3 + j] = (double)T_wc[(std::size_t)(i * 4 + j)];
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) {
      double s = 0.0;
      for (int m = 0; m < 6; ++m) s += B[i][m] * P[(std::size_t)(m * 6 + j)];
      T[i][j] = s;
    }
  std::array<double, 36> C{};
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) {
      double a = 0.0, b = 0.0;  // both halves from the same two sums: exactly symmetric
      for (int m = 0; m < 6; ++m) {
        a += T[i][m] * B[j][m];
        b += T[j][m] * B[i][m];
      }
      C[(std::size_t)(i * 6 + j)] = C[(std::size_t)(j * 6 + i)] = 0.5 * (a + b);
    }
  return C;
}

}  // namespace vo
#endif
