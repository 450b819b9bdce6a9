// plane_shim.cpp -- extern "C" view of pvio_amd/host/plane_ransac.{h,cpp} for tests/test_plane_ransac.py and tests/prof_plane_ransac.py (built
// by them with g++ -O2 -ffp-contract=off next to plane_ransac.cpp; no device, no other product source).
#include <cstdint>
#include <cstring>

#include "../../pvio_amd/host/plane_ransac.h"

extern "C" {

// ints: n_inliers, iterations, best_iteration, refit_valid; doubles: normal[3] distance refit_normal[3] refit_distance reference_point[3]
void host_plane_ransac(int n, const double *points, double threshold, double confidence, int max_iterations, uint32_t seed, uint8_t *mask, int32_t ints[4],
                       double doubles[11]) {
    const pvio::PlaneRansacResult r = pvio::plane_ransac(n, points, threshold, confidence, max_iterations, seed);
    if (n > 0) std::memcpy(mask, r.inlier_mask.data(), (size_t)n);
    ints[0] = r.n_inliers, ints[1] = r.iterations, ints[2] = r.best_iteration, ints[3] = r.refit_valid ? 1 : 0;
    std::memcpy(doubles, r.normal, 3 * sizeof(double));
    doubles[3] = r.distance;
    std::memcpy(doubles + 4, r.refit_normal, 3 * sizeof(double));
    doubles[7] = r.refit_distance;
    std::memcpy(doubles + 8, r.reference_point, 3 * sizeof(double));
}

// returns found; n_inliers and the inlier indices (room for n), doubles: normal[3] distance reference_point[3]
int host_extract_plane(int n, const double *points, int min_inliers, int32_t *n_inliers, int64_t *inliers, double doubles[7]) {
    const pvio::ExtractedPlane e = pvio::extract_plane(n, points, 0.03, 0.999, 1000, 0, min_inliers);
    *n_inliers = (int32_t)e.inliers.size();
    for (size_t k = 0; k < e.inliers.size(); ++k) inliers[k] = (int64_t)e.inliers[k];
    std::memcpy(doubles, e.normal, 3 * sizeof(double));
    doubles[3] = e.distance;
    std::memcpy(doubles + 4, e.reference_point, 3 * sizeof(double));
    return e.found ? 1 : 0;
}
}
