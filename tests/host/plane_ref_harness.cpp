// plane_ref_harness.cpp -- the reference's OWN plane RANSAC over a file of points: pvio::Ransac<3, PlaneState, PlaneExtractor::PlaneSolver,
// PlaneExtractor::PlaneEvaluator> instantiated from the reference's headers, read in place (header-only: nothing of the reference is linked).
// tests/test_plane_ransac.py builds it into its temporary directory -- include paths: the reference's pvio/src, the mini-Eigen of
// oracle/ref/eigen, a generated pvio/version.h -- and compares pv_plane.h's restatement of sampler, model and bookkeeping with what it returns.
//   plane_ref_harness points.f64 out.bin threshold confidence max_iterations seed
//   points.f64: n x 3 doubles;  out.bin: five doubles (inlier_count, normal[3], distance), then n mask bytes
#include <cstdio>
#include <cstdlib>
#include <vector>

#include <pvio/core/plane_extractor.h>
#include <pvio/utility/ransac.h>

int main(int argc, char **argv) {
    if (argc != 7) return 2;
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    std::vector<double> raw;
    double buf[3];
    while (std::fread(buf, sizeof(double), 3, f) == 3) raw.insert(raw.end(), buf, buf + 3);
    std::fclose(f);
    std::vector<pvio::vector<3>> points(raw.size() / 3);
    for (size_t i = 0; i < points.size(); ++i) points[i] = pvio::vector<3>(raw[3 * i], raw[3 * i + 1], raw[3 * i + 2]);

    pvio::Ransac<3, pvio::PlaneState, pvio::PlaneExtractor::PlaneSolver, pvio::PlaneExtractor::PlaneEvaluator> ransac(
        std::atof(argv[3]), std::atof(argv[4]), (size_t)std::atol(argv[5]), std::atoi(argv[6]));
    const pvio::PlaneState model = ransac.solve(points);

    const double head[5] = {(double)ransac.inlier_count, model.normal(0), model.normal(1), model.normal(2), model.distance};
    f = std::fopen(argv[2], "wb");
    if (!f) return 4;
    std::fwrite(head, sizeof(double), 5, f);
    if (!ransac.inlier_mask.empty()) std::fwrite(ransac.inlier_mask.data(), 1, ransac.inlier_mask.size(), f);
    std::fclose(f);
    return 0;
}
