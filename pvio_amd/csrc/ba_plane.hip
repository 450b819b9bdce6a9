// ba_plane.hip -- plane RANSAC over landmark points on the device (pvio_hip_plane_ransac).
//
// Reference: PlaneExtractor::work (core/plane_extractor.cpp:40-81): Ransac<3, PlaneState, PlaneSolver, PlaneEvaluator> over the landmark
// points, then cog / covariance / smallest eigenvector of the winner's inliers.  The arithmetic of a model and of an error is pv_plane.h, the
// same sequence of IEEE operations here, in the host-only form and in the tests' restatement.
//
//   k_plane_hypotheses   a wave per hypothesis and chunk of points, four hypotheses to a workgroup, blockIdx.y the chunk.  The samples of ALL
//                        hypotheses are drawn on the host up front (they depend on nothing the device computes); every lane turns the wave's
//                        sample into its model -- the same arithmetic on the same numbers --, the lanes stride over the chunk's points, one
//                        ballot per 64 points counts the inliers, lane 0 adds the wave's share to the hypothesis' count (an integer atomic:
//                        any order gives the same sum).  Up to kPlaneChunk points a hypothesis is ONE wave; above, a wave that walked all n
//                        points alone on its SIMD waited out one memory round trip per 64 points (363 us at 50 000 points against
//                        73 us), so the points are spread over more waves.  Counts and models are written, masks are NOT:
//                        only the winner's is ever used, and k_plane_refit writes that one.  No LDS, no barriers; the loop bounds are
//                        wave-uniform, so every lane reaches every ballot.
//   k_plane_refit        ONE workgroup, for the winning model: thread t takes the points t, t + 1024, ... in rising order; re-scores them
//                        (mask and count), then two passes like the reference -- sum p -> cog = sum / count, sum (p - cog)(p - cog)^T -- and
//                        thread 0 takes the eigenvector of the smallest eigenvalue (cyclic Jacobi, pv_plane.h), orients it toward the RANSAC
//                        normal and writes normal, distance = normal . cog and cog.  Every sum is a thread's own points in index order, then
//                        an xor butterfly over the wave, then the sixteen wave sums in wave order: a fixed tree, two calls give the same
//                        bits.  The refit is computed whenever count >= 3; the reference's `> 30` rule is the caller's.
// Not an object of its own: the last lines of ba_solver.cpp include this file, so every build of the solver (product, emulator, variants) has it.
#include <hip/hip_runtime.h>

#include "ba_plane.h"
#include "pv_plane.h"

namespace pvba {

__global__ void __launch_bounds__(kPlaneHypThreads) k_plane_hypotheses(PlaneArgs a) {
    PV_NO_CONTRACT
    const int lane = (int)threadIdx.x & 63;
    const int h = (int)blockIdx.x * (kPlaneHypThreads / 64) + ((int)threadIdx.x >> 6); // wave-uniform
    if (h >= a.n_hyp) return;                                                           // the whole wave leaves
    const int32_t *s = a.samples + 3 * (size_t)h; // indices in [0, n): drawn by PlSampler
    double m[4];
    pvpl::pl_model(a.points + 3 * (size_t)s[0], a.points + 3 * (size_t)s[1], a.points + 3 * (size_t)s[2], m);
    const int begin = (int)blockIdx.y * a.chunk, end = min(a.n, begin + a.chunk); // (grid.y = ceil(n / chunk): begin < n)
    int count = 0;
    for (int i0 = begin; i0 < end; i0 += 64) {
        const int i = i0 + lane;
        int in = 0;
        if (i < end) in = pvpl::pl_error(m, a.points + 3 * (size_t)i) <= a.threshold ? 1 : 0;
        count += __popcll(__ballot(in));
    }
    if (lane == 0 && count != 0) atomicAdd(a.counts + h, count);
    if (blockIdx.y == 0 && lane < 4) a.models[4 * (size_t)h + lane] = m[lane];
}

// every thread of the workgroup ends with the same K sums, bit for bit: butterfly over the wave, then the wave sums in wave order
template <int K>
__device__ __forceinline__ void plane_block_sum(double (&s)[K], double (*red)[6]) {
    PV_NO_CONTRACT
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        double o[K];
#pragma unroll
        for (int k = 0; k < K; ++k) o[k] = __shfl_xor(s[k], m);
#pragma unroll
        for (int k = 0; k < K; ++k) s[k] += o[k];
    }
    const int wave = (int)threadIdx.x >> 6;
    __syncthreads(); // the previous use of `red` has been read
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < K; ++k) red[wave][k] = s[k];
    __syncthreads();
    for (int k = 0; k < K; ++k) {
        double t = red[0][k];
        for (int w = 1; w < kPlaneRefitThreads / 64; ++w) t += red[w][k];
        s[k] = t;
    }
}

__global__ void __launch_bounds__(kPlaneRefitThreads) k_plane_refit(PlaneArgs a) {
    PV_NO_CONTRACT
    __shared__ double red[kPlaneRefitThreads / 64][6];
    const int t = (int)threadIdx.x;
    // inliers of the winning model: the mask, the count
    double cnt[1] = {0.0};
    for (int i = t; i < a.n; i += kPlaneRefitThreads) {
        const uint8_t in = pvpl::pl_error(a.model, a.points + 3 * (size_t)i) <= a.threshold ? 1 : 0;
        a.mask[i] = in, cnt[0] += in; // (a thread reads back only what it wrote itself)
    }
    plane_block_sum<1>(cnt, red); // whole numbers below 2^24: exact
    const double count = cnt[0];
    // first pass: the centre of gravity
    double sp[3] = {0.0, 0.0, 0.0};
    for (int i = t; i < a.n; i += kPlaneRefitThreads)
        if (a.mask[i]) {
            const double *p = a.points + 3 * (size_t)i;
            sp[0] += p[0], sp[1] += p[1], sp[2] += p[2];
        }
    plane_block_sum<3>(sp, red);
    const double cog[3] = {sp[0] / count, sp[1] / count, sp[2] / count};
    // second pass: the scatter about it
    double sc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = t; i < a.n; i += kPlaneRefitThreads)
        if (a.mask[i]) {
            const double *p = a.points + 3 * (size_t)i;
            const double dx = p[0] - cog[0], dy = p[1] - cog[1], dz = p[2] - cog[2];
            sc[0] += dx * dx, sc[1] += dx * dy, sc[2] += dx * dz, sc[3] += dy * dy, sc[4] += dy * dz, sc[5] += dz * dz;
        }
    plane_block_sum<6>(sc, red);
    if (t != 0) return;
    double *out = a.record;
    for (int k = 0; k < kPlaneRecord; ++k) out[k] = 0.0;
    out[0] = count;
    if (count >= 3.0) {
        double v[3];
        const int sweeps = pvpl::pl_smallest_eigvec(sc, v);
        pvpl::pl_orient(v, a.model);
        out[1] = 1.0;
        out[2] = v[0], out[3] = v[1], out[4] = v[2];
        out[5] = pvpl::pl_dot(v, cog);
        out[6] = cog[0], out[7] = cog[1], out[8] = cog[2];
        out[9] = (double)sweeps;
    }
}

hipError_t launch_plane_hypotheses(const PlaneArgs &args, hipStream_t st) {
    if (args.n_hyp <= 0) return hipSuccess;
    if (args.n <= 0 || args.chunk < 64 || args.chunk % 64 != 0) return hipErrorInvalidValue;
    PlaneArgs a = args;
    while (((unsigned)a.n + (unsigned)a.chunk - 1) / (unsigned)a.chunk > 65535u) a.chunk *= 2; // the grid's y limit (n <= 2^24: at most 256 points per wave)
    const unsigned per_block = kPlaneHypThreads / 64, chunks = ((unsigned)a.n + (unsigned)a.chunk - 1) / (unsigned)a.chunk;
    hipLaunchKernelGGL(k_plane_hypotheses, dim3(((unsigned)a.n_hyp + per_block - 1) / per_block, chunks), dim3(kPlaneHypThreads), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_plane_refit(const PlaneArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(k_plane_refit, dim3(1), dim3(kPlaneRefitThreads), 0, st, a);
    return hipGetLastError();
}

} // namespace pvba
