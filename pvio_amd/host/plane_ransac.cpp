// plane_ransac.cpp -- see plane_ransac.h.  The host-only form of the plane RANSAC: sequential hypothesise-and-verify, every hypothesis scored
// over all points like the reference does, then the refit.  The arithmetic is pvio_amd/csrc/pv_plane.h, shared with the device form.
#include "plane_ransac.h"

#include <algorithm>
#include <cmath>

#include "../csrc/pv_plane.h"

#if !defined(__clang__) && defined(__GNUC__)
#pragma GCC optimize("fp-contract=off") // the sums of the refit below, like the header's functions
#endif

namespace pvio {
namespace {

// cog, scatter, smallest eigenvector of the inliers (plane_extractor.cpp:59-77), sums in index order
void refit(int n, const double *points, PlaneRansacResult &r) {
    PV_NO_CONTRACT
    double sp[3] = {0, 0, 0}, sc[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < n; ++i)
        if (r.inlier_mask[(size_t)i]) sp[0] += points[3 * i], sp[1] += points[3 * i + 1], sp[2] += points[3 * i + 2];
    const double count = (double)r.n_inliers, cog[3] = {sp[0] / count, sp[1] / count, sp[2] / count};
    for (int i = 0; i < n; ++i)
        if (r.inlier_mask[(size_t)i]) {
            const double dx = points[3 * i] - cog[0], dy = points[3 * i + 1] - cog[1], dz = points[3 * i + 2] - cog[2];
            sc[0] += dx * dx, sc[1] += dx * dy, sc[2] += dx * dz, sc[3] += dy * dy, sc[4] += dy * dz, sc[5] += dz * dz;
        }
    (void)pvpl::pl_smallest_eigvec(sc, r.refit_normal);
    pvpl::pl_orient(r.refit_normal, r.normal);
    r.refit_distance = pvpl::pl_dot(r.refit_normal, cog);
    std::copy(cog, cog + 3, r.reference_point);
    r.refit_valid = true;
}

} // namespace

PlaneRansacResult plane_ransac(int n, const double *points, double threshold, double confidence, int max_iterations, uint32_t seed) {
    PlaneRansacResult r;
    r.inlier_mask.assign((size_t)std::max(n, 0), 0);
    if (n < 3) return r;
    pvpl::PlSampler sampler(n, seed);
    pvpl::PlBest run(confidence, max_iterations);
    std::vector<uint8_t> cur((size_t)n);
    int iter = 0;
    for (; iter < run.iter_max; ++iter) {
        int32_t s[3];
        sampler.sample(s);
        double m[4];
        pvpl::pl_model(points + 3 * (size_t)s[0], points + 3 * (size_t)s[1], points + 3 * (size_t)s[2], m);
        int good = 0;
        for (int i = 0; i < n; ++i) {
            const uint8_t in = pvpl::pl_error(m, points + 3 * (size_t)i) <= threshold ? 1 : 0;
            cur[(size_t)i] = in, good += in;
        }
        if (run.offer(good, iter, n)) {
            std::swap(cur, r.inlier_mask);
            std::copy(m, m + 3, r.normal);
            r.distance = m[3];
        }
    }
    r.iterations = iter, r.n_inliers = run.count, r.best_iteration = run.best_iter;
    if (r.n_inliers >= 3) refit(n, points, r);
    return r;
}

ExtractedPlane extract_plane(int n, const double *points, double threshold, double confidence, int max_iterations, uint32_t seed, int min_inliers) {
    ExtractedPlane e;
    const PlaneRansacResult r = plane_ransac(n, points, threshold, confidence, max_iterations, seed);
    if (!(r.n_inliers > min_inliers) || !r.refit_valid) return e;
    e.found = true;
    for (size_t i = 0; i < r.inlier_mask.size(); ++i)
        if (r.inlier_mask[i]) e.inliers.push_back(i);
    std::copy(r.refit_normal, r.refit_normal + 3, e.normal);
    e.distance = r.refit_distance;
    std::copy(r.reference_point, r.reference_point + 3, e.reference_point);
    return e;
}

} // namespace pvio
