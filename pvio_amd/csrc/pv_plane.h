// pv_plane.h -- the arithmetic of the plane RANSAC over landmark points, shared by the device kernels (ba_plane.hip: k_plane_hypotheses,
// k_plane_refit), the host orchestration around them (BASolver::plane_ransac) and the host-only implementation the tests hold them against
// (pvio_amd/host/plane_ransac.cpp).
//
// Reference: PlaneExtractor::work (core/plane_extractor.cpp:40-81) -- Ransac<3, PlaneState, PlaneSolver, PlaneEvaluator> (utility/ransac.h,
// core/plane_extractor.h:47-65) over the landmark points, then a least-squares refit of the winner's inliers.  The pieces:
//   pl_dot / pl_model / pl_error   plane through a 3-point sample, distance of a point to it                              [host + device]
//   pl_smallest_eigvec / pl_orient the refit's eigenvector (cyclic Jacobi on the 3 x 3) and its DEFINED sign               [host + device]
//   PlMinstd / pl_uniform          std::default_random_engine and std::uniform_int_distribution<size_t>, restated          [host only]
//   PlSampler                      LotBox: three draws without replacement from a permutation that PERSISTS over iterations [host only]
//   PlBest                         the loop's bookkeeping: strictly more inliers replace the best, iter_max shrinks         [host only]
//
// DEFINED ARITHMETIC.  An inlier count decides which hypothesis wins and a point whose error sits on the threshold moves a count by one, so a
// model and an error are ONE sequence of IEEE operations wherever this header is compiled: FP64, no FMA contraction (PV_NO_CONTRACT; hipcc
// contracts by default), no libm beyond sqrt and fabs (correctly rounded / exact on both sides).  A dot product is (x0 y0 + x1 y1) + x2 y2 --
// Eigen's order for a 3-vector, also that of the sum of squares in stableNormalize.
//
// QUIRKS KEPT.  A degenerate sample (collinear or duplicate points) has a zero cross product: w = 0, z = NaN, the normal stays zero, the
// distance is 0 and EVERY finite point is an inlier (error 0 <= threshold) -- the reference does the same.  A sample with a non-finite
// coordinate gives a non-finite normal: every error is NaN (or infinite) and `error <= threshold` holds for no point.
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

#include "pv_math.h" // PV_HD, PV_NO_CONTRACT

#if !defined(__clang__) && defined(__GNUC__)
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off") // g++ contracts by default unless the build says otherwise: the functions below must not
#endif

namespace pvpl {

constexpr int kPlaneJacobiSweeps = 30; // bound of the refit's Jacobi loop for any input; a covariance of real points needs 3 to 6

PV_HD double pl_dot(const double *x, const double *y) {
    PV_NO_CONTRACT
    return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2];
}

// m = normal[3] | distance of the plane through p0, p1, p2 (plane_extractor.h:47-55): normal = (p2 - p0) x (p1 - p0), Eigen's stableNormalize
// (w = max |c|; z = sum (c / w)^2; divided by sqrt(z) w only if z > 0), distance = p0 . normal
PV_HD void pl_model(const double *p0, const double *p1, const double *p2, double m[4]) {
    PV_NO_CONTRACT
    const double a[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]}, b[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
    double c[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
    double w = fabs(c[0]);
    if (fabs(c[1]) > w) w = fabs(c[1]);
    if (fabs(c[2]) > w) w = fabs(c[2]);
    const double s[3] = {c[0] / w, c[1] / w, c[2] / w};
    const double z = pl_dot(s, s);
    if (z > 0) {
        const double d = sqrt(z) * w;
        c[0] /= d, c[1] /= d, c[2] /= d;
    }
    m[0] = c[0], m[1] = c[1], m[2] = c[2];
    m[3] = pl_dot(p0, c);
}

// |p . normal - distance| (plane_extractor.h:57-65); a point is an inlier iff pl_error(...) <= threshold, which NaN fails
PV_HD double pl_error(const double m[4], const double *p) {
    PV_NO_CONTRACT
    return fabs(pl_dot(p, m) - m[3]);
}

// Unit eigenvector of the smallest eigenvalue of the symmetric 3 x 3 (xx, xy, xz, yy, yz, zz): cyclic Jacobi, pairs (0,1) (0,2) (1,2), a pair
// rotated while |a_pq| > eps sqrt(|a_pp a_qq|) -- false for NaN, so a NaN matrix ends the loop at once; kPlaneJacobiSweeps bounds it for every
// other input.  Ties take the first of the equal diagonal entries.  Returns the sweeps taken (the last, rotation-free one included).
PV_HD int pl_smallest_eigvec(const double cov[6], double v[3]) {
    PV_NO_CONTRACT
    double A[3][3] = {{cov[0], cov[1], cov[2]}, {cov[1], cov[3], cov[4]}, {cov[2], cov[4], cov[5]}};
    double V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    int sweeps = 0;
    for (; sweeps < kPlaneJacobiSweeps;) {
        ++sweeps;
        bool rotated = false;
#pragma unroll
        for (int pair = 0; pair < 3; ++pair) { // (unrolled: p, q, r are constants, the matrices stay in registers)
            const int p = pair == 2 ? 1 : 0, q = pair == 0 ? 1 : 2, r = 3 - p - q;
            const double apq = A[p][q];
            if (!(fabs(apq) > 2.220446049250313e-16 * sqrt(fabs(A[p][p] * A[q][q])))) continue;
            rotated = true;
            const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
            const double t = (theta < 0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
            const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
            A[p][p] -= t * apq, A[q][q] += t * apq;
            A[p][q] = A[q][p] = 0.0;
            const double arp = A[r][p], arq = A[r][q];
            A[r][p] = A[p][r] = c * arp - s * arq;
            A[r][q] = A[q][r] = s * arp + c * arq;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double vp = V[k][p], vq = V[k][q];
                V[k][p] = c * vp - s * vq, V[k][q] = s * vp + c * vq;
            }
        }
        if (!rotated) break;
    }
    double lmin = A[0][0], e[3] = {V[0][0], V[1][0], V[2][0]};
    if (A[1][1] < lmin) lmin = A[1][1], e[0] = V[0][1], e[1] = V[1][1], e[2] = V[2][1];
    if (A[2][2] < lmin) lmin = A[2][2], e[0] = V[0][2], e[1] = V[1][2], e[2] = V[2][2];
    const double len = sqrt(pl_dot(e, e)); // 1 up to the rounding of the rotations
    v[0] = e[0] / len, v[1] = e[1] / len, v[2] = e[2] / len;
    return sweeps;
}

// the sign the reference leaves to Eigen, DEFINED: v . toward >= 0; if that is exactly 0 (the zero normal of a degenerate sample), the first
// non-zero component of v is positive
PV_HD void pl_orient(double v[3], const double *toward) {
    PV_NO_CONTRACT
    const double d = pl_dot(v, toward);
    const bool neg = d < 0.0 || (d == 0.0 && (v[0] < 0.0 || (v[0] == 0.0 && (v[1] < 0.0 || (v[1] == 0.0 && v[2] < 0.0)))));
    if (neg) v[0] = -v[0], v[1] = -v[1], v[2] = -v[2];
}

// ---- host only --------------------------------------------------------------------------------------------------------------------

// std::default_random_engine as libstdc++ defines it (minstd_rand0) -- the library the reference's results in this project come from:
// x <- 16807 x mod (2^31 - 1); seed s -> s mod (2^31 - 1), 0 replaced by 1.  Restated so that the samples do not depend on the library the
// product is built with (libc++ picks another engine and another distribution algorithm); tests/host/plane_sampler_check.cpp compares with the
// std classes of the machine it is built on.
struct PlMinstd {
    uint32_t x;
    explicit PlMinstd(uint32_t seed) : x(seed % 2147483647u ? seed % 2147483647u : 1u) {}
    uint32_t next() { return x = (uint32_t)((uint64_t)x * 16807u % 2147483647u); } // in [1, 2^31 - 2]
};

// std::uniform_int_distribution<size_t>(a, b) over that engine, libstdc++'s downscaling branch: the engine's range is 2^31 - 3, the bucket
// size range / m, values past m buckets are redrawn.  Holds for m - 1 < 2^31 - 3 (pvio_hip_plane_ransac admits n <= 2^24).
inline uint32_t pl_uniform(PlMinstd &g, uint32_t a, uint32_t b) {
    const uint32_t range = 2147483645u, m = b - a + 1u, scaling = range / m, past = m * scaling;
    uint32_t r;
    do r = g.next() - 1u;
    while (r >= past);
    return a + r / scaling;
}

// LotBox (utility/random.h:108-163) as Ransac::solve uses it: refill_all only resets `cap`, the swaps of earlier iterations stay; three
// draw_without_replacement per iteration; when one lot remains (n = 3, third draw) no number is drawn and the LAST lot is returned.
struct PlSampler {
    std::vector<uint32_t> lots;
    PlMinstd rng;
    PlSampler(int n, uint32_t seed) : lots((size_t)(n > 0 ? n : 0)), rng(seed) {
        for (size_t i = 0; i < lots.size(); ++i) lots[i] = (uint32_t)i;
    }
    void sample(int32_t idx[3]) { // lots.size() >= 3
        const uint32_t n = (uint32_t)lots.size();
        for (uint32_t cap = 0; cap < 3; ++cap) {
            if (n - cap > 1) {
                const uint32_t j = pl_uniform(rng, cap, n - 1);
                const uint32_t t = lots[cap];
                lots[cap] = lots[j], lots[j] = t;
                idx[cap] = (int32_t)lots[cap];
            } else {
                idx[cap] = (int32_t)lots[n - 1];
            }
        }
    }
};

// The bookkeeping of Ransac::solve (ransac.h:49-92), the ONE definition of its acceptance and stopping rule: a hypothesis replaces the best only
// with STRICTLY more inliers (the best starts at 0), and then N = K / log(1 - (count / n)^5), K = log(max(1 - confidence, 1e-5)), shrinks
// iter_max to ceil(N) when N < iter_max.  A ratio of 1 gives N = -0: the run ends after that iteration.  Two cases the reference leaves to an
// out-of-range conversion are defined: a ratio so small that 1 - ratio^5 rounds to 1 (log = 0; N would be K / 0) changes nothing -- the
// limit of the formula --, and a negative N (a confidence <= 0) is taken as 0.  The sequential host form offers every hypothesis as it scores
// it, the device form replays the counts in the order of the draws.  libm is used here: host only, one implementation.
struct PlBest {
    double K;
    int iter_max, count = 0, best_iter = -1;
    PlBest(double confidence, int max_iterations) : K(log(1 - confidence > 1.0e-5 ? 1 - confidence : 1.0e-5)), iter_max(max_iterations) {}
    bool offer(int good, int iter, int n) { // true: the hypothesis is the best now
        if (good <= count) return false;
        count = good, best_iter = iter;
        const double ratio = good / (double)n, den = log(1 - pow(ratio, 5));
        if (den != 0) {
            const double N = K / den;
            if (N < (double)iter_max) iter_max = N > 0 ? (int)ceil(N) : 0;
        }
        return true;
    }
};

} // namespace pvpl

#if !defined(__clang__) && defined(__GNUC__)
#pragma GCC pop_options
#endif
