// ba_cov.h -- marginal covariances of a window (pvio_hip_ba_covariance): buffers and launchers of the kernels of ba_cov.hip.
//
// The kernels run behind one undamped MODE_INIT linearization (k_linearize + k_reduce phase 0) and read what it left on the device:
// `red`, pre_H, prior_H, rot_H and the per-landmark Hll / Wa / Wt of linearization set Ctrl::lin.
#pragma once
#include <hip/hip_runtime.h>

#include "ba_types.h"

namespace pvba {

constexpr int kCovThreads = 256;       // workgroup size of every kernel of ba_cov.hip
constexpr double kCovMinPivot = 1e-10; // PVIO_COV_MIN_PIVOT: smallest pivot of the unit-diagonal reduced system that counts as observable
// k_cov_invert keeps the lower block triangle of the scaled system (16 x 16 tiles) in LDS while it fits the 160 KiB a workgroup may take:
// 12 tile rows = 78 tiles = 159 744 bytes, i.e. up to 192 free coordinates.  Larger systems run the same code on the tiles in global memory.
constexpr int kCovLdsMaxTileRows = 12;
constexpr int kCovLdsMaxCoords = 16 * kCovLdsMaxTileRows;

inline size_t cov_tile_rows(size_t coords) { return (coords + 15) / 16; }
inline size_t cov_tile_doubles(size_t coords) { return cov_tile_rows(coords) * (cov_tile_rows(coords) + 1) / 2 * 256; }

struct CovHdr { // first bytes of the result buffer
    int32_t n_free, positive_definite, first_bad_coord, layout_error;
};

struct CovArgs { // passed by value
    int32_t D;           // 15 N window coordinates
    int32_t max_coords;  // upper bound of the free coordinates the host sized the tiles for
    // work
    double *Sfull;       // [D][D] the reduced information matrix S in window coordinates (symmetric, both halves)
    double *scale;       // [D] c_i = 1 / sqrt(S_ii) of a free coordinate
    double *tiles;       // scaled lower block triangle in free-coordinate order: tile (bi, bk <= bi) at (bi (bi + 1) / 2 + bk) * 256
    double *sig6;        // [6N][6N] pose part of the joint covariance (what k_cov_landmarks reads)
    int32_t *row_nz;     // [D] the coordinate's block is active and its row of S is not exactly zero
    int32_t *free_coord; // [D] free index -> window coordinate
    // results (one buffer: header | coord_free | frame_cov | lm_var | joint_cov)
    CovHdr *hdr;
    uint8_t *coord_free; // [D]
    double *frame_cov;   // [N][15][15]
    double *lm_var;      // [M]
    double *joint_cov;   // [D][D]
};

hipError_t launch_cov_assemble(const View &v, const CovArgs &a, hipStream_t st); // three phases: entries, zero rows, scaled tiles
hipError_t launch_cov_invert(const View &v, const CovArgs &a, hipStream_t st);
hipError_t launch_cov_landmarks(const View &v, const CovArgs &a, hipStream_t st);

} // namespace pvba
