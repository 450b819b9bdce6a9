// ba_triangulate.hip -- batched multi-view DLT triangulation on the device (pvio_hip_triangulate).
//
// Reference: Track::triangulate / try_triangulate (map/track.cpp:61-106) build the 2K x 4 system u P_2 - P_0, v P_2 - P_1 of a track's K
// observations, triangulate_point_scored (geometry/stereo.h:67-74,104-128) takes its last right singular vector q and applies the
// in-front-of-every-camera and depth < 100 gates.  Here one launch does that for every track of a call.
//
//   k_triangulate<G>   a track takes a group of G lanes (64, or 32 when no track of the call has more than 16 observations), lane r < 2K holds
//                      row r of the system as four doubles, the other lanes hold zero rows.  One-sided (Hestenes) Jacobi on the rows
//                      themselves -- A^T A is never formed, the condition number is not squared: a sweep is three rounds of two disjoint
//                      column pairs, (0,1)(2,3), (0,2)(1,3), (0,3)(1,2); the six sums of a round (both squared column norms and the inner
//                      product, for both pairs) go through one xor butterfly over the group, after which every lane holds the same bits and
//                      applies the same rotation to its row and to its own copy of the 4 x 4 V.  No LDS, no barriers, no polling.
//                      A pair is rotated while |a_i . a_j| > 2K eps |a_i| |a_j| (the sqrt(rows) eps of dgesvj is not enough for the sums of
//                      64 products to settle under; the residual coupling moves q by at most K eps sigma_3 / (sigma_3 - sigma_4)).  The
//                      comparison is false for NaN, so a NaN row ends the loop at once; kTriMaxSweeps bounds it for every other input.
//                      q is the column of V whose rotated column of A is the shortest; each observation's even lane then evaluates
//                      y = P q, the gates and its reprojection term; `ok` comes from a ballot, `score` from one more butterfly.
// The loop's exit is wave-uniform (a ballot over the rotation flags): the lanes of a wave stay together around every shuffle, also when two
// tracks share the wave.  A track that has converged is not changed by the further sweeps its neighbour needs: none of its pairs is rotated.
// Every sum is taken in a fixed order: two calls on the same input give the same bits.
// Not an object of its own: the last line of ba_solver.cpp includes this file, so every build of the solver (product, emulator, variants) has it.
#include <hip/hip_runtime.h>

#include <cmath>

#include "ba_triangulate.h"

namespace pvba {

template <int G>
__device__ __forceinline__ void tri_group_sum(double (&s)[6]) { // every lane of the group ends with the same six sums, bit for bit
#pragma unroll
    for (int m = 1; m < G; m <<= 1) {
        double o[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) o[k] = __shfl_xor(s[k], m);
#pragma unroll
        for (int k = 0; k < 6; ++k) s[k] += o[k];
    }
}
template <int G>
__device__ __forceinline__ double tri_group_sum(double x) {
#pragma unroll
    for (int m = 1; m < G; m <<= 1) x += __shfl_xor(x, m);
    return x;
}

// the plane rotation that makes columns i and j orthogonal, from alpha = |a_i|^2, beta = |a_j|^2, gamma = a_i . a_j; applied to the row and to V
template <int I, int J>
__device__ __forceinline__ bool tri_rotate(double alpha, double beta, double gamma, double tol2, double (&row)[4], double (&V)[4][4]) {
    if (!(gamma * gamma > tol2 * alpha * beta)) return false; // orthogonal enough, a zero column, or NaN
    const double zeta = (beta - alpha) / (2.0 * gamma);
    const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
    const double ri = row[I], rj = row[J];
    row[I] = c * ri - s * rj, row[J] = s * ri + c * rj;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double vi = V[k][I], vj = V[k][J];
        V[k][I] = c * vi - s * vj, V[k][J] = s * vi + c * vj;
    }
    return true;
}

// one round: the disjoint pairs (I, J) and (K, L)
template <int G, int I, int J, int K, int L>
__device__ __forceinline__ bool tri_round(double tol2, double (&row)[4], double (&V)[4][4]) {
    double s[6] = {row[I] * row[I], row[J] * row[J], row[I] * row[J], row[K] * row[K], row[L] * row[L], row[K] * row[L]};
    tri_group_sum<G>(s);
    const bool a = tri_rotate<I, J>(s[0], s[1], s[2], tol2, row, V);
    const bool b = tri_rotate<K, L>(s[3], s[4], s[5], tol2, row, V);
    return a || b;
}

template <int G>
__global__ void __launch_bounds__(kTriThreads) k_triangulate(TriArgs a) {
    const int track = (int)blockIdx.x * (kTriThreads / G) + (int)threadIdx.x / G, r = (int)threadIdx.x % G;
    const bool live = track < a.n_tracks;              // the lanes behind the last track hold zero rows and go through every shuffle
    const int t = live ? track : a.n_tracks - 1;       // (n_tracks > 0: launch_triangulate)
    const int o0 = a.track_ptr[t];
    const int K = live ? a.track_ptr[t + 1] - o0 : 0;  // <= G / 2: BASolver::triangulate
    const bool solvable = K >= 2;
    const int xy = r & 1;
    const bool has_row = solvable && r < 2 * K;
    double row[4] = {0.0, 0.0, 0.0, 0.0}, z[2] = {0.0, 0.0};
    const double *P = a.view_P;
    if (has_row) {
        const int o = o0 + (r >> 1);
        P += 12 * a.obs_view[o];
        z[0] = a.obs_z[2 * o], z[1] = a.obs_z[2 * o + 1];
#pragma unroll
        for (int c = 0; c < 4; ++c) row[c] = z[xy] * P[8 + c] - P[4 * xy + c];
    }
    double V[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    const double tol = 2.0 * (double)K * 2.220446049250313e-16, tol2 = tol * tol; // 2K eps

    int my_sweeps = 0; // sweeps until this track's first one without a rotation (that one included)
    bool converged = false;
    for (int sweep = 0; sweep < kTriMaxSweeps; ++sweep) {
        bool rotated = tri_round<G, 0, 1, 2, 3>(tol2, row, V);
        rotated = tri_round<G, 0, 2, 1, 3>(tol2, row, V) || rotated;
        rotated = tri_round<G, 0, 3, 1, 2>(tol2, row, V) || rotated;
        if (!converged) my_sweeps = sweep + 1, converged = !rotated;
        if (__ballot(rotated) == 0ull) break; // wave-uniform
    }

    // q: the column of V that belongs to the shortest column of A V
    double n[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) n[c] = tri_group_sum<G>(row[c] * row[c]);
    int best = 0;
    double nb = n[0];
#pragma unroll
    for (int c = 1; c < 4; ++c)
        if (n[c] < nb) nb = n[c], best = c;
    double q[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = best == 0 ? V[k][0] : best == 1 ? V[k][1] : best == 2 ? V[k][2] : V[k][3];
    {
        const double len = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]); // 1 up to the rounding of the rotations
        const bool neg = q[3] < 0.0 || (q[3] == 0.0 && (q[0] < 0.0 || (q[0] == 0.0 && (q[1] < 0.0 || (q[1] == 0.0 && q[2] < 0.0)))));
        const double f = (neg ? -1.0 : 1.0) / len;
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] *= f;
    }

    // gates and reprojection term of observation r / 2 on its even lane (stereo.h:111-119: the negated comparisons, NaN fails them)
    bool bad = false;
    double err = 0.0;
    if (has_row && xy == 0) {
        double y[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) y[k] = P[4 * k] * q[0] + P[4 * k + 1] * q[1] + P[4 * k + 2] * q[2] + P[4 * k + 3] * q[3];
        bad = !(y[2] * q[3] > 0.0) || !(y[2] / q[3] < 100.0);
        const double du = y[0] / y[2] - z[0], dv = y[1] / y[2] - z[1];
        err = du * du + dv * dv;
    }
    const unsigned long long ballot = __ballot(bad);
    const unsigned long long mine = G == 64 ? ballot : (ballot >> (threadIdx.x & 32u)) & 0xffffffffull;
    const double score = tri_group_sum<G>(err) / (double)K;

    if (r == 0 && live) {
        double *out = a.result + (size_t)track * kTriRecord;
        if (!solvable) { // the reference asserts here
            for (int k = 0; k < 7; ++k) out[k] = 0.0;
            out[7] = INFINITY, out[8] = 0.0;
        } else {
            const bool ok = mine == 0ull;
            const double len3 = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
            const double div = ok ? q[3] : len3 > 0.0 ? len3 : 1.0; // hnormalized() / normalized(), which leaves a zero vector as it is
            for (int k = 0; k < 4; ++k) out[k] = q[k];
            for (int k = 0; k < 3; ++k) out[4 + k] = q[k] / div;
            out[7] = score, out[8] = ok ? 1.0 : 0.0;
            atomicMax(a.max_sweeps, my_sweeps);
        }
    }
}

hipError_t launch_triangulate(const TriArgs &a, int group_lanes, hipStream_t st) {
    if (a.n_tracks <= 0) return hipSuccess;
    const unsigned per_block = (unsigned)(kTriThreads / group_lanes);
    const dim3 grid(((unsigned)a.n_tracks + per_block - 1) / per_block);
    if (group_lanes == 32) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_triangulate<32>), grid, dim3(kTriThreads), 0, st, a);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_triangulate<64>), grid, dim3(kTriThreads), 0, st, a);
    return hipGetLastError();
}

} // namespace pvba
