// marg_prior.h -- the dense host algebra of BundleAdjustor::marginalize_frame (bundle_adjustor.cpp:536-590) as pure functions over plain arrays:
// assemble_information -> eliminate_victim -> sqrt_information.  No HIP call, no solver, no pool: BASolver::marginalize (ba_solver.cpp) hands them what
// it read back from the device and owns the large work arrays; tests/hipemu/marg_prior_check.cpp calls them alone.  Header-only, so that no list of
// sources changes.  Every loop nest keeps the iteration order and the accumulation variables its results were verified with.
#pragma once
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "sym_eig.h"

namespace pvba {

inline bool lu_inverse15(const double *Ain, double *inv) { // Eigen's .inverse() for a 15 x 15 block is PartialPivLU based
    const int n = 15;
    double A[225];
    int piv[15];
    std::memcpy(A, Ain, sizeof A);
    for (int i = 0; i < n; ++i) piv[i] = i;
    for (int k = 0; k < n; ++k) {
        int p = k;
        double best = std::fabs(A[k * n + k]);
        for (int i = k + 1; i < n; ++i)
            if (std::fabs(A[i * n + k]) > best) best = std::fabs(A[i * n + k]), p = i;
        if (best == 0.0) return false;
        if (p != k) {
            for (int j = 0; j < n; ++j) std::swap(A[k * n + j], A[p * n + j]);
            std::swap(piv[k], piv[p]);
        }
        for (int i = k + 1; i < n; ++i) {
            const double f = A[i * n + k] / A[k * n + k];
            A[i * n + k] = f;
            for (int j = k + 1; j < n; ++j) A[i * n + j] -= f * A[k * n + j];
        }
    }
    for (int col = 0; col < n; ++col) {
        double x[15];
        for (int i = 0; i < n; ++i) x[i] = piv[i] == col ? 1.0 : 0.0;
        for (int i = 0; i < n; ++i)
            for (int k = 0; k < i; ++k) x[i] -= A[i * n + k] * x[k];
        for (int i = n - 1; i >= 0; --i) {
            for (int k = i + 1; k < n; ++k) x[i] -= A[i * n + k] * x[k];
            x[i] /= A[i * n + i];
        }
        for (int i = 0; i < n; ++i) inv[i * n + col] = x[i];
    }
    return true;
}

// What one marginalization pass (k_linearize in MODE_MARG + k_reduce) leaves on the device, on the host: the segments of BASolver's gather.
struct MargSegments {
    const double *red;                 // [9 n_tasks] 3 x 3 tiles, element-major | [6N] J^T r | [6N] sum_l W_l^T b_l / H_ll | ...
    const double *pre_H, *pre_g;       // [N][30][30], [N][30]: IMU factor j over frames j - 1, j
    const double *prior_H, *prior_g;   // [15 prior_n][15 prior_n], [15 prior_n]: the old prior in its own coordinates
    const double *rot_H, *rot_g;       // [N][3][3], [N][3]: rotation priors (zero where a frame has none)
    const int32_t *task_desc;          // [n_tasks] fi | fj << 8 | si << 16 | sj << 17
};

// The 15N information matrix H (both halves) and vector b of everything the victim touches.  preint_valid may be null (no IMU factors).
inline void assemble_information(const MargSegments &g, const uint8_t *preint_valid, const int32_t *prior_frames, int prior_n, int N, int victim, int n_tasks,
                                 int P6, std::vector<double> &H, std::vector<double> &b) {
    const int D = 15 * N;
    const size_t nS = (size_t)n_tasks * 9, Dp = 15 * (size_t)prior_n;
    b.assign(D, 0.0);
    H.assign((size_t)D * D, 0.0);
    for (int t = 0; t < n_tasks; ++t) {
        const int fi = g.task_desc[t] & 255, fj = (g.task_desc[t] >> 8) & 255, si = (g.task_desc[t] >> 16) & 1, sj = (g.task_desc[t] >> 17) & 1;
        for (int el = 0; el < 9; ++el) {
            const int r = 15 * fi + 3 * si + el / 3, c = 15 * fj + 3 * sj + el % 3;
            const double val = g.red[(size_t)el * n_tasks + t];
            if (fi != fj) H[(size_t)r * D + c] = H[(size_t)c * D + r] = val;
            else if (r >= c) H[(size_t)r * D + c] = H[(size_t)c * D + r] = val; // only the lower half of a diagonal block is complete
        }
    }
    for (int f = 0; f < N; ++f)
        for (int k = 0; k < 6; ++k) b[15 * f + k] = g.red[nS + 6 * f + k] - g.red[nS + P6 + 6 * f + k]; // J^T r - sum_l W_l^T b_l / H_ll
    for (int j = victim; j <= victim + 1; ++j) {
        if (j == 0 || j >= N || !(preint_valid && preint_valid[j])) continue;
        for (int a = 0; a < 30; ++a) {
            b[15 * (j - 1) + a] += g.pre_g[(size_t)j * 30 + a];
            for (int c = 0; c < 30; ++c) H[(size_t)(15 * (j - 1) + a) * D + 15 * (j - 1) + c] += g.pre_H[(size_t)j * 900 + a * 30 + c];
        }
    }
    for (int a = 0; a < 3; ++a) { // the victim's rotation prior (evaluated un-gated in MODE_MARG; zero when it has none)
        b[15 * victim + a] += g.rot_g[(size_t)victim * 3 + a];
        for (int c = 0; c < 3; ++c) H[(size_t)(15 * victim + a) * D + 15 * victim + c] += g.rot_H[(size_t)victim * 9 + 3 * a + c];
    }
    std::vector<int> gprior(Dp); // prior coordinate -> window coordinate (a division per ELEMENT of the 135 x 135 block cost 40 us here)
    for (size_t a = 0; a < Dp; ++a) gprior[a] = 15 * prior_frames[a / 15] + (int)(a % 15);
    for (size_t a = 0; a < Dp; ++a) {
        const int ga = gprior[a];
        b[ga] += g.prior_g[a];
        double *hrow = &H[(size_t)ga * D];
        const double *prow = &g.prior_H[a * Dp];
        for (size_t c = 0; c < Dp; ++c) hrow[gprior[c]] += prow[c];
    }
}

// Eliminates the victim's 15 x 15 block (:547-581): C = H_rr - H_rv H_vv^-1 H_vr, cv = b_r - H_rv H_vv^-1 b_v over the other 15 (N - 1) coordinates.
// false: the victim's block is singular; C and cv are then left as they were.
inline bool eliminate_victim(const std::vector<double> &H, const std::vector<double> &b, int N, int victim, std::vector<double> &C, std::vector<double> &cv) {
    const int D = 15 * N, R = D - 15;
    double Hvv[225], Hinv[225];
    for (int x = 0; x < 15; ++x)
        for (int y = 0; y < 15; ++y) Hvv[x * 15 + y] = H[(size_t)(15 * victim + x) * D + 15 * victim + y];
    if (!lu_inverse15(Hvv, Hinv)) return false;
    auto gidx = [&](int k) { return k < 15 * victim ? k : k + 15; };
    std::vector<double> T((size_t)R * 15);
    cv.assign(R, 0.0);
    C.assign((size_t)R * R, 0.0);
    for (int i = 0; i < R; ++i) { // T = H_rv Hvv^-1: fifteen independent sums per row, each still taken over x in ascending order
        const double *hiv = &H[(size_t)gidx(i) * D + 15 * victim];
        double trow[15] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int x = 0; x < 15; ++x) {
            const double hx = hiv[x];
            for (int y = 0; y < 15; ++y) trow[y] += hx * Hinv[x * 15 + y];
        }
        for (int y = 0; y < 15; ++y) T[(size_t)i * 15 + y] = trow[y];
    }
    const int split = 15 * victim;
    // the victim's rows with the victim's own columns removed, so that the inner loops below run over contiguous memory (the sums are
    // taken in the same order as a loop over y per element would take them; that form cost 100 us per marginalization)
    std::vector<double> Hv((size_t)15 * R), acc(R);
    for (int y = 0; y < 15; ++y)
        for (int j = 0; j < R; ++j) Hv[(size_t)y * R + j] = H[(size_t)(15 * victim + y) * D + gidx(j)];
    for (int i = 0; i < R; ++i) {
        double s = 0;
        for (int y = 0; y < 15; ++y) s += T[(size_t)i * 15 + y] * b[15 * victim + y];
        cv[i] = b[gidx(i)] - s;
        const int j0 = i >= split ? split : 0; // lower-left = transpose of upper-right (:572-576), filled in below
        for (int j = j0; j < R; ++j) acc[j] = 0;
        for (int y = 0; y < 15; ++y) {
            const double ty = T[(size_t)i * 15 + y];
            const double *hv = &Hv[(size_t)y * R];
            for (int j = j0; j < R; ++j) acc[j] += ty * hv[j];
        }
        const double *hi = &H[(size_t)gidx(i) * D];
        double *ci = &C[(size_t)i * R];
        for (int j = j0; j < split; ++j) ci[j] = hi[j] - acc[j];
        for (int j = j0 > split ? j0 : split; j < R; ++j) ci[j] = hi[j + 15] - acc[j];
    }
    for (int i = split; i < R; ++i)
        for (int j = 0; j < split; ++j) C[(size_t)i * R + j] = C[(size_t)j * R + i];
    return true;
}

struct SqrtInfoStats { // diagnostics of one sqrt_information (the PVIO_HIP_TIMING line of marginalize)
    int Rk = 0;        // order of the eigen-problem: the coordinates that carry information
    std::chrono::steady_clock::time_point eig_begin, eig_end;
};

// Square-root information (:583-590): S = sqrt(L) V^T [R x R] and s = L^-1/2 V^T cv [R] of C = V L V^T, eigenvalues <= 1e-8 zeroed.  C (R x R) is
// used up: the coordinates that stay in the eigen-problem are compressed to the front of its storage.  V is work space.
// Coordinates without any information -- an exactly zero row and column: velocity / biases of a frame no IMU factor or prior reaches --
// are eigenvectors of eigenvalue 0 by themselves and stay out of the eigen-problem: a backward-stable solver would hand them back with
// an eigenvalue of a few eps |C| and a few eps of every other coordinate mixed in, which the 1e-8 cut then keeps or drops as the rounding
// falls (profiles/NOTES_r1_r3.md section 2a).  Their rows of S are zero (they come first, like the zero eigenvalues of the full problem).
inline SqrtInfoStats sqrt_information(std::vector<double> &C, const std::vector<double> &cv, int R, std::vector<double> &V, double *S, double *s) {
    SqrtInfoStats stats;
    std::vector<int> keep;
    keep.reserve(R);
    for (int i = 0; i < R; ++i) {
        bool zero = true;
        for (int j = 0; j < R && zero; ++j) zero = C[(size_t)i * R + j] == 0.0 && C[(size_t)j * R + i] == 0.0;
        if (!zero) keep.push_back(i);
    }
    const int Rk = stats.Rk = (int)keep.size(), nz = R - Rk;
    std::vector<double> w(std::max(Rk, 1));
    V.resize((size_t)std::max(Rk, 1) * std::max(Rk, 1));
    stats.eig_begin = std::chrono::steady_clock::now();
    if (nz > 0) { // compress the kept coordinates to the front of C's storage (the caller has made its copies)
        for (int a = 0; a < Rk; ++a)
            for (int b = 0; b < Rk; ++b) C[(size_t)a * Rk + b] = C[(size_t)keep[a] * R + keep[b]];
    }
    if (Rk > 0) sym_eig(C.data(), Rk, w.data(), V.data());
    stats.eig_end = std::chrono::steady_clock::now();
    std::fill(S, S + (size_t)R * R, 0.0);
    std::fill(s, s + R, 0.0);
    for (int k = 0; k < Rk; ++k) {
        const double lam = w[k] > 1.0e-8 ? w[k] : 0.0, lam_inv = w[k] > 1.0e-8 ? 1.0 / w[k] : 0.0;
        const double sl = std::sqrt(lam), sli = std::sqrt(lam_inv);
        double acc = 0;
        double *Srow = S + (size_t)(nz + k) * R;
        for (int i = 0; i < Rk; ++i) {
            Srow[keep[i]] = sl * V[(size_t)k * Rk + i];
            acc += V[(size_t)k * Rk + i] * cv[keep[i]];
        }
        s[nz + k] = sli * acc;
    }
    return stats;
}

} // namespace pvba
