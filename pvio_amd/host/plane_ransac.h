// plane_ransac.h -- the plane extraction of PlaneExtractor::work (core/plane_extractor.cpp:40-81), host only: the 3-point plane RANSAC
// Ransac<3, PlaneState, PlaneSolver, PlaneEvaluator> (utility/ransac.h; threshold 0.03, confidence 0.999, 1000 iterations, seed 0) over the
// landmark points and the least-squares refit of the winner's inliers.  The arithmetic -- model, error, sampler, stopping rule, the refit's
// eigenvector and its sign -- is pvio_amd/csrc/pv_plane.h, shared with the batched device form (pvio_hip_plane_ransac); this
// sequential form is what the tests hold the device form against (identical masks and models) and the CPU timing baseline.
//   * the sampler, the `strictly more inliers` rule and the ^5 stopping rule are the reference's (tests/test_plane_ransac.py pins them against
//     the reference's own template);
//   * a degenerate sample has a zero normal and every finite point as an inlier, as in the reference;
//   * the refit is computed whenever the winner has >= 3 inliers; extract_plane applies the reference's `> 30` rule on top.
// A product PlaneExtractor above this -- in the drop-in or the stand-in headless driver -- is the follow-up.
#pragma once
#include "host_namespace.h"
#include <cstddef>
#include <cstdint>
#include <vector>

namespace pvio {

struct PlaneRansacResult {
    int n_inliers = 0, iterations = 0, best_iteration = -1;
    bool refit_valid = false;
    std::vector<uint8_t> inlier_mask;               // [n]
    double normal[3] = {0, 0, 0}, distance = 0;     // the RANSAC model (ransac.solve's return)
    double refit_normal[3] = {0, 0, 0}, refit_distance = 0, reference_point[3] = {0, 0, 0}; // plane_extractor.cpp:59-77
};

// points: [n][3].  n < 3: the empty result (the reference returns an uninitialised model there).
PlaneRansacResult plane_ransac(int n, const double *points, double threshold = 0.03, double confidence = 0.999, int max_iterations = 1000, uint32_t seed = 0);

// what PlaneExtractor::work puts into a PlaneRecord
struct ExtractedPlane {
    bool found = false;                // ransac.inlier_count > min_inliers
    std::vector<size_t> inliers;       // indices into `points`, rising (the caller maps them to track ids)
    double normal[3] = {0, 0, 0}, distance = 0, reference_point[3] = {0, 0, 0}; // the refit's parameters
};
ExtractedPlane extract_plane(int n, const double *points, double threshold = 0.03, double confidence = 0.999, int max_iterations = 1000, uint32_t seed = 0,
                             int min_inliers = 30);

} // namespace pvio
