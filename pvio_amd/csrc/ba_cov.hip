// ba_cov.hip -- marginal covariances of a window on the device (pvio_hip_ba_covariance, NO REFERENCE COUNTERPART).
//
// Runs behind one undamped MODE_INIT linearization (Ctrl::mu = 0: the Schur weight is 1 / H_ll) and k_reduce phase 0:
//   k_cov_assemble   S = H_pp - sum_l W_l^T W_l / H_ll in window coordinates 15 f + k from `red`, pre_H, prior_H and rot_H (the device form of
//                    BASolver::marginalize's host loop, over the whole window); the free coordinates; the unit-diagonal S^ = C S C as 16 x 16 tiles
//   k_cov_invert     one workgroup: blocked Cholesky S^ = L L^T with the pivot rule of include/pvio_hip.h, L^-1 in place, Sigma^ = L^-T L^-1 in
//                    place (the three steps of a LAPACK potrf / trtri / lauum), all tile products on v_mfma_f64_16x16x4_f64; C Sigma^ C scattered
//                    into joint_cov / frame_cov.  Tiles in LDS up to kCovLdsMaxCoords free coordinates, else the same code on global memory.
//   k_cov_landmarks  one thread per landmark: 1 / H_ll + W_l Sigma W_l^T / H_ll^2
// Every sum is taken in a fixed order and there are no atomics: two calls on the same input give the same bits.
// Not an object of its own: the last line of ba_solver.cpp includes this file, so every build of the solver (product, emulator, variants) has it.
// The helpers restated from ba_kernels.hip (task_index, the entry terms of the reduced system) are copies on purpose: that file is not touched.
#include <hip/hip_runtime.h>

#include "ba_cov.h"

namespace pvba {

typedef double cov_d4 __attribute__((vector_size(32))); // the accumulator of one v_mfma_f64_16x16x4_f64

// index of the 3x3 tile task (fi <= fj, si, sj) in upload()'s enumeration (fi-major, fj, then 2 si + sj), as in ba_kernels.hip
__device__ __forceinline__ int cov_task_index(int N, int fi, int fj, int si, int sj) {
    return 4 * (fi * N - ((fi * (fi - 1)) >> 1) + (fj - fi)) + 2 * si + sj;
}
__device__ __forceinline__ bool cov_block_active(const View &v, int f, int k) { return (k < 6 ? v.pose_active[f] : v.motion_active[f]) != 0; }

// Element (r, c) of a 16 x 16 tile.  Rows are rotated by their index: lanes that walk a column (the A operand of a product with the tile itself)
// and lanes that walk a row both touch sixteen different bank pairs.
__device__ __forceinline__ int cov_at(int r, int c) { return (r << 4) + ((c + r) & 15); }
__device__ __forceinline__ double *cov_tile(double *A, int bi, int bk) { return A + ((size_t)(((bi * (bi + 1)) >> 1) + bk) << 8); }

// ------------------------------------------------------------------------------------------------------
// k_cov_assemble, phase 0: one thread per entry (i, k <= i) of S.  Terms in the order the solver's own assembly adds them
// (apply_entry_terms in ba_kernels.hip): landmark / plane tile, rotation prior, the two IMU factors (odd factor first), prior.
//                 phase 1: one wave per row: is the coordinate's block active and its row not exactly zero?
//                 phase 2: one workgroup per tile of the scaled system in free-coordinate order (+ scale vector, coord_free, free list)
// ------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kCovThreads) k_cov_assemble(View v, CovArgs a, int phase) {
    const int D = a.D, N = v.dm.N, tid = threadIdx.x;
    if (phase == 0) {
        const size_t e = (size_t)blockIdx.x * kCovThreads + tid;
        if (e >= (size_t)D * D) return;
        const int i = (int)(e / D), k = (int)(e - (size_t)i * D);
        if (k > i) return;
        const int fa = i / 15, ka = i - 15 * fa, fb = k / 15, kb = k - 15 * fb; // fb <= fa
        double val = 0.0;
        if (cov_block_active(v, fa, ka) && cov_block_active(v, fb, kb)) {
            if (ka < 6 && kb < 6) {
                // off-diagonal frame pairs once (the smaller frame is the row of the task); diagonal blocks are complete in their lower half only
                const int n_tasks = v.dm.n_tasks;
                const int t = fa != fb ? cov_task_index(N, fb, fa, kb / 3, ka / 3) : cov_task_index(N, fa, fa, ka / 3, kb / 3);
                const int el = fa != fb ? 3 * (kb % 3) + (ka % 3) : 3 * (ka % 3) + (kb % 3);
                const int want = fa != fb ? (fb | fa << 8 | (kb / 3) << 16 | (ka / 3) << 17) : (fa | fa << 8 | (ka / 3) << 16 | (kb / 3) << 17);
                if (v.task_desc[t] != want) a.hdr->layout_error = 1; // the task table is not in the order this file assumes: the host refuses the result
                val = v.red[(size_t)el * n_tasks + t];
            }
            if (v.dm.n_rot > 0 && fa == fb && ka < 3 && kb < 3) val += v.rot_H[9 * fa + 3 * ka + kb];
            if (v.dm.d == 15) {
                if (v.dm.G_pre) { // factor j couples frames j - 1 (local 0..14) and j (local 15..29)
                    const bool same = fa == fb, adj = fa == fb + 1;
                    double hA = 0.0, hB = 0.0;
                    if (fa >= 1 && (same || adj) && v.pre_valid[fa]) hA = v.pre_H[(size_t)fa * 900 + (15 + ka) * 30 + (same ? 15 : 0) + kb];
                    if (same && fa + 1 < N && v.pre_valid[fa + 1]) hB = v.pre_H[(size_t)(fa + 1) * 900 + ka * 30 + kb];
                    val = (fa & 1) ? (val + hA) + hB : (val + hB) + hA;
                }
                if (v.dm.prior_n > 0) {
                    const int pa = v.prior_slot[fa], pb = v.prior_slot[fb];
                    if (pa >= 0 && pb >= 0) val += v.prior_H[(size_t)(15 * pa + ka) * (15 * v.dm.prior_n) + 15 * pb + kb];
                }
            }
        }
        a.Sfull[(size_t)i * D + k] = val;
        a.Sfull[(size_t)k * D + i] = val;
        return;
    }
    if (phase == 1) { // 4 rows per workgroup
        const int i = blockIdx.x * (kCovThreads / 64) + (tid >> 6), lane = tid & 63;
        if (i >= D) return; // (whole waves)
        int any = 0;
        for (int k = lane; k < D; k += 64) any |= a.Sfull[(size_t)i * D + k] != 0.0; // (a NaN is not a zero)
        const unsigned long long m = __ballot(any);
        if (lane == 0) a.row_nz[i] = (m != 0ull && cov_block_active(v, i / 15, i % 15)) ? 1 : 0;
        return;
    }
    // ---- phase 2 ----
    __shared__ int s_free[15 * kMaxFrames];
    __shared__ int s_n;
    if (tid == 0) {
        int n = 0;
        for (int i = 0; i < D; ++i)
            if (a.row_nz[i]) s_free[n++] = i;
        s_n = n;
    }
    __syncthreads();
    const int n = s_n, nb = (n + 15) >> 4;
    int bi = 0;
    while ((((bi + 1) * (bi + 2)) >> 1) <= (int)blockIdx.x) ++bi;
    const int bk = (int)blockIdx.x - ((bi * (bi + 1)) >> 1);
    if (blockIdx.x == 0) {
        for (int i = tid; i < D; i += kCovThreads) {
            const int fr = a.row_nz[i];
            const double sii = a.Sfull[(size_t)i * D + i];
            a.coord_free[i] = (uint8_t)fr;
            a.scale[i] = fr ? (sii > 0.0 ? 1.0 / sqrt(sii) : __builtin_nan("")) : 0.0;
            if (i < n) a.free_coord[i] = s_free[i];
        }
        if (tid == 0) a.hdr->n_free = n;
    }
    if (bi >= nb) return;
    const int r = tid >> 4, c = tid & 15, aa = 16 * bi + r, bb = 16 * bk + c;
    double val = 0.0;
    if (aa < n && bb <= aa) {
        const int gi = s_free[aa], gk = s_free[bb];
        const double sii = a.Sfull[(size_t)gi * D + gi], skk = a.Sfull[(size_t)gk * D + gk];
        const double ci = sii > 0.0 ? 1.0 / sqrt(sii) : __builtin_nan(""), ck = skk > 0.0 ? 1.0 / sqrt(skk) : __builtin_nan("");
        val = (a.Sfull[(size_t)gi * D + gk] * ci) * ck;
    } else if (aa == bb) {
        val = 1.0; // padding up to whole tiles: an identity block, factored and inverted along with the rest
    }
    cov_tile(a.tiles, bi, bk)[cov_at(r, c)] = val; // (the upper half of a diagonal tile is zero and stays zero)
}

// ------------------------------------------------------------------------------------------------------
// k_cov_invert
// ------------------------------------------------------------------------------------------------------
// Operand of one v_mfma_f64_16x16x4_f64 step kk of a product over a tile T.  Lane l supplies A[l & 15][l >> 4] and B[l >> 4][l & 15]:
// ROW = false reads T[l & 15][4 kk + (l >> 4)] (T as the left factor, or T^T as the right one), ROW = true reads T[4 kk + (l >> 4)][l & 15]
// (T as the right factor, or T^T as the left one).
template <bool ROW>
__device__ __forceinline__ double cov_operand(const double *T, int kk, int lane) {
    const int x = lane & 15, y = 4 * kk + (lane >> 4);
    return ROW ? T[cov_at(y, x)] : T[cov_at(x, y)];
}
// acc (+/-)= op(Ta) op(Tb), sixteen inner products of length 16 per lane group, in the order kk = 0..3
template <bool ROW_A, bool ROW_B, bool NEG>
__device__ __forceinline__ cov_d4 cov_mm(cov_d4 acc, const double *Ta, const double *Tb, int lane) {
    double av[4], bv[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) av[kk] = cov_operand<ROW_A>(Ta, kk, lane), bv[kk] = cov_operand<ROW_B>(Tb, kk, lane);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(NEG ? -av[kk] : av[kk], bv[kk], acc, 0, 0, 0);
    return acc;
}
// accumulator layout: element q of lane l is entry ((l >> 4) + 4 q, l & 15)
__device__ __forceinline__ cov_d4 cov_load(const double *T, int lane) {
    cov_d4 acc;
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = T[cov_at((lane >> 4) + 4 * q, lane & 15)];
    return acc;
}
__device__ __forceinline__ void cov_store(double *T, cov_d4 acc, int lane, bool lower_only) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int r = (lane >> 4) + 4 * q, c = lane & 15;
        if (!lower_only || r >= c) T[cov_at(r, c)] = acc[q];
    }
}

constexpr int kCovAccTiles = 8; // tiles a wave holds between the two barriers of a step: (15 * kMaxFrames / 16) tile rows over four waves

template <bool LDSMAT>
__global__ void __launch_bounds__(kCovThreads) k_cov_invert(View v, CovArgs a) {
    HIP_DYNAMIC_SHARED(double, lds)
    static_assert((15 * kMaxFrames + 15) / 16 <= 4 * kCovAccTiles, "accumulators per wave");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int D = a.D, n = a.hdr->n_free, nb = (n + 15) >> 4;
    if (n > a.max_coords) return; // (cannot happen: the host counted every block that can be free; the header then still says "not positive definite")
    double *A = LDSMAT ? lds : a.tiles;
    if (LDSMAT) {
        const int total = ((nb * (nb + 1)) >> 1) << 8;
        for (int e = tid; e < total; e += kCovThreads) lds[e] = a.tiles[e];
    }
    __syncthreads();

    // ---- S^ = L L^T, right-looking over tile columns ----
    for (int k = 0; k < nb; ++k) {
        double *Tkk = cov_tile(A, k, k);
        { // the diagonal tile, one thread per entry (r, c <= r); two barriers per column
            const int r = tid >> 4, c = tid & 15;
            for (int j = 0; j < 16; ++j) {
                __syncthreads();
                const double piv = Tkk[cov_at(j, j)]; // every thread reads the same value: the branch is uniform
                if (!(piv > kCovMinPivot)) {          // (a NaN fails too)
                    if (tid == 0) a.hdr->positive_definite = 0, a.hdr->first_bad_coord = a.free_coord[16 * k + j]; // (padding pivots are 1)
                    return;
                }
                const double ljj = sqrt(piv);
                const double lrj = r > j ? Tkk[cov_at(r, j)] / ljj : 0.0, lcj = c > j ? Tkk[cov_at(c, j)] / ljj : 0.0;
                __syncthreads();
                if (c == j && r > j) Tkk[cov_at(r, j)] = lrj;
                if (c == j && r == j) Tkk[cov_at(j, j)] = ljj;
                if (c > j && r >= c) Tkk[cov_at(r, c)] -= lrj * lcj;
            }
        }
        __syncthreads();
        // the panel below it: A_ik <- A_ik L_kk^-T, one thread per row
        for (int rr = tid; rr < (nb - 1 - k) * 16; rr += kCovThreads) {
            double *T = cov_tile(A, k + 1 + (rr >> 4), k);
            const int r = rr & 15;
            double x[16];
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                double s = T[cov_at(r, c)];
#pragma unroll
                for (int m = 0; m < c; ++m) s -= x[m] * Tkk[cov_at(c, m)];
                x[c] = s / Tkk[cov_at(c, c)];
            }
#pragma unroll
            for (int c = 0; c < 16; ++c) T[cov_at(r, c)] = x[c];
        }
        __syncthreads();
        // trailing tiles (i, j), k < j <= i: A_ij -= A_ik A_jk^T, dealt to the waves in turn
        const int rem = nb - 1 - k, n_upd = (rem * (rem + 1)) >> 1;
        for (int t = wave; t < n_upd; t += kCovThreads / 64) {
            int ii = 0;
            while ((((ii + 1) * (ii + 2)) >> 1) <= t) ++ii;
            const int i = k + 1 + ii, j = k + 1 + t - ((ii * (ii + 1)) >> 1);
            double *T = cov_tile(A, i, j);
            cov_d4 acc = cov_load(T, lane);
            acc = cov_mm<false, false, true>(acc, cov_tile(A, i, k), cov_tile(A, j, k), lane);
            cov_store(T, acc, lane, i == j);
        }
        // (the first barrier of the next tile column separates these stores from its reads)
    }
    __syncthreads();

    // ---- X = L^-1 in place, tile columns from the last to the first: column j needs the inverse of everything to its right ----
    for (int j = nb - 1; j >= 0; --j) {
        double *Tjj = cov_tile(A, j, j);
        double x[16];
        if (tid < 16) { // the diagonal tile: thread c solves L x = e_c
            const int c = tid;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                double s = r == c ? 1.0 : 0.0;
#pragma unroll
                for (int m = 0; m < r; ++m) s -= Tjj[cov_at(r, m)] * x[m];
                x[r] = r < c ? 0.0 : s / Tjj[cov_at(r, r)];
            }
        }
        __syncthreads();
        if (tid < 16) {
#pragma unroll
            for (int r = 0; r < 16; ++r) Tjj[cov_at(r, tid)] = x[r];
        }
        __syncthreads();
        // T_i = sum_{m = j+1..i} X_im L_mj for every tile row below, held in registers until every wave has read column j
        cov_d4 acc[kCovAccTiles];
#pragma unroll
        for (int q = 0; q < kCovAccTiles; ++q) {
            const int i = j + 1 + wave + 4 * q;
            if (i < nb) {
                cov_d4 z = {0.0, 0.0, 0.0, 0.0};
                for (int m = j + 1; m <= i; ++m) z = cov_mm<false, true, false>(z, cov_tile(A, i, m), cov_tile(A, m, j), lane);
                acc[q] = z;
            }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kCovAccTiles; ++q) {
            const int i = j + 1 + wave + 4 * q;
            if (i < nb) cov_store(cov_tile(A, i, j), acc[q], lane, false);
        }
        __syncthreads();
        // X_ij = - T_i X_jj (a wave reads and rewrites its own tiles only)
#pragma unroll
        for (int q = 0; q < kCovAccTiles; ++q) {
            const int i = j + 1 + wave + 4 * q;
            if (i < nb) {
                cov_d4 z = {0.0, 0.0, 0.0, 0.0};
                z = cov_mm<false, true, true>(z, cov_tile(A, i, j), Tjj, lane);
                cov_store(cov_tile(A, i, j), z, lane, false);
            }
        }
    }
    __syncthreads();

    // ---- Sigma^ = X^T X in place, tile rows from the first to the last: row i reads rows >= i and is read by rows <= i ----
    for (int i = 0; i < nb; ++i) {
        cov_d4 acc[kCovAccTiles];
#pragma unroll
        for (int q = 0; q < kCovAccTiles; ++q) {
            const int j = wave + 4 * q;
            if (j <= i) {
                cov_d4 z = {0.0, 0.0, 0.0, 0.0};
                for (int m = i; m < nb; ++m) z = cov_mm<true, true, false>(z, cov_tile(A, m, i), cov_tile(A, m, j), lane);
                acc[q] = z;
            }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kCovAccTiles; ++q) {
            const int j = wave + 4 * q;
            if (j <= i) cov_store(cov_tile(A, i, j), acc[q], lane, false);
        }
        __syncthreads();
    }

    // ---- Sigma = C Sigma^ C into window coordinates: the lower half is computed, the upper half is its copy ----
    const int r = tid >> 4, c = tid & 15, P6 = v.dm.P6;
    for (int bi = 0; bi < nb; ++bi)
        for (int bk = 0; bk <= bi; ++bk) {
            const int aa = 16 * bi + r, bb = 16 * bk + c;
            if (aa >= n || bb > aa) continue;
            const int gi = a.free_coord[aa], gk = a.free_coord[bb];
            const double val = (cov_tile(A, bi, bk)[cov_at(r, c)] * a.scale[gi]) * a.scale[gk];
            a.joint_cov[(size_t)gi * D + gk] = val;
            a.joint_cov[(size_t)gk * D + gi] = val;
            const int fi = gi / 15, ki = gi - 15 * fi, fk = gk / 15, kk = gk - 15 * fk;
            if (fi == fk) a.frame_cov[fi * 225 + ki * 15 + kk] = val, a.frame_cov[fi * 225 + kk * 15 + ki] = val;
            if (ki < 6 && kk < 6) a.sig6[(size_t)(6 * fi + ki) * P6 + 6 * fk + kk] = val, a.sig6[(size_t)(6 * fk + kk) * P6 + 6 * fi + ki] = val;
        }
    if (tid == 0) a.hdr->positive_definite = 1, a.hdr->first_bad_coord = -1;
}

// ------------------------------------------------------------------------------------------------------
// k_cov_landmarks: lm_var[l] = 1 / H_ll + W_l Sigma W_l^T / H_ll^2 over the landmark's anchor and target blocks (a frame listed twice is two
// blocks: the quadratic form sums them).  Blocks p >= q once, off-diagonal pairs doubled; a fixed frame's W block and Sigma rows are zero.
// ------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kCovThreads) k_cov_landmarks(View v, CovArgs a) {
    const int l = blockIdx.x * kCovThreads + threadIdx.x, M = v.dm.M, P6 = v.dm.P6;
    if (l >= M || !a.hdr->positive_definite) return;
    const int lin = v.ctrl->lin;
    const size_t Ms = (size_t)M, Fs = (size_t)v.dm.F;
    const double Hll = v.Hll[lin * Ms + l];
    const double *Wa = v.Wa + lin * Ms * 6 + (size_t)l * 6, *Wt = v.Wt + lin * Fs * 6;
    const int o0 = v.lm_ptr[l], o1 = v.lm_ptr[l + 1], anchor = v.lm_anchor[l];
    if (o1 == o0 || !(Hll > 0.0) || !isfinite(Hll)) {
        a.lm_var[l] = __builtin_huge_val();
        return;
    }
    double diag = 0.0, off = 0.0;
    for (int p = 0; p <= o1 - o0; ++p) {
        const int fp = p == 0 ? anchor : v.obs_frame[o0 + p - 1];
        const double *wp = p == 0 ? Wa : Wt + (size_t)(o0 + p - 1) * 6;
        double w[6];
#pragma unroll
        for (int x = 0; x < 6; ++x) w[x] = wp[x];
        for (int q = 0; q <= p; ++q) {
            const int fq = q == 0 ? anchor : v.obs_frame[o0 + q - 1];
            const double *wq = q == 0 ? Wa : Wt + (size_t)(o0 + q - 1) * 6;
            const double *Sg = a.sig6 + (size_t)(6 * fp) * P6 + 6 * fq;
            double s = 0.0;
#pragma unroll
            for (int x = 0; x < 6; ++x) {
                double t = 0.0;
#pragma unroll
                for (int y = 0; y < 6; ++y) t += Sg[(size_t)x * P6 + y] * wq[y];
                s += w[x] * t;
            }
            if (q == p) diag += s;
            else off += s;
        }
    }
    a.lm_var[l] = 1.0 / Hll + (diag + 2.0 * off) / (Hll * Hll);
}

// ------------------------------------------------------------------------------------------------------
hipError_t launch_cov_assemble(const View &v, const CovArgs &a, hipStream_t st) {
    const size_t D = (size_t)a.D;
    hipLaunchKernelGGL(k_cov_assemble, dim3((unsigned)((D * D + kCovThreads - 1) / kCovThreads)), dim3(kCovThreads), 0, st, v, a, 0);
    hipLaunchKernelGGL(k_cov_assemble, dim3((unsigned)((D + 3) / 4)), dim3(kCovThreads), 0, st, v, a, 1);
    const size_t nbm = cov_tile_rows((size_t)a.max_coords);
    if (nbm > 0) hipLaunchKernelGGL(k_cov_assemble, dim3((unsigned)(nbm * (nbm + 1) / 2)), dim3(kCovThreads), 0, st, v, a, 2);
    return hipGetLastError();
}

hipError_t launch_cov_invert(const View &v, const CovArgs &a, hipStream_t st) {
    if (a.max_coords <= kCovLdsMaxCoords) {
        const size_t lds = cov_tile_doubles((size_t)a.max_coords) * sizeof(double);
        static size_t configured = 0;
        if (lds > configured) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_cov_invert<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
            configured = lds;
        }
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cov_invert<true>), dim3(1), dim3(kCovThreads), lds, st, v, a);
    } else {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cov_invert<false>), dim3(1), dim3(kCovThreads), 0, st, v, a);
    }
    return hipGetLastError();
}

hipError_t launch_cov_landmarks(const View &v, const CovArgs &a, hipStream_t st) {
    if (v.dm.M <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_cov_landmarks, dim3((unsigned)((v.dm.M + kCovThreads - 1) / kCovThreads)), dim3(kCovThreads), 0, st, v, a);
    return hipGetLastError();
}

} // namespace pvba
