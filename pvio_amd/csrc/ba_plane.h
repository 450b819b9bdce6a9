// ba_plane.h -- plane RANSAC over landmark points (pvio_hip_plane_ransac): buffers and launchers of the kernels of ba_plane.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pvba {

constexpr int kPlaneHypThreads = 256;    // k_plane_hypotheses: four waves, a hypothesis each
constexpr int kPlaneRefitThreads = 1024; // k_plane_refit: ONE workgroup of sixteen waves
constexpr int kPlaneChunk = 4096;        // points a wave of k_plane_hypotheses scores: n above it spreads a hypothesis over ceil(n / chunk) waves
constexpr int kPlaneMaxIterations = 4096;
constexpr int kPlaneMaxPoints = 1 << 24;
constexpr int kPlaneRecord = 12; // doubles of the refit's record: count | refit_valid | refit_normal[3] | refit_distance | cog[3] | sweeps | 2 spare

struct PlaneArgs { // passed by value; every pointer into the one device buffer of a call
    int32_t n, n_hyp;
    int32_t chunk;          // k_plane_hypotheses: points per wave, a multiple of 64
    double threshold;
    const double *points;   // [n][3]
    const int32_t *samples; // [n_hyp][3] point indices, drawn on the host
    int32_t *counts;        // [n_hyp], zeroed by the upload: the waves of a hypothesis add their shares
    double *models;         // [n_hyp][4] normal | distance
    double model[4];        // k_plane_refit: the winner, as k_plane_hypotheses wrote it
    double *record;         // [kPlaneRecord]
    uint8_t *mask;          // [n]
};

hipError_t launch_plane_hypotheses(const PlaneArgs &a, hipStream_t st);
hipError_t launch_plane_refit(const PlaneArgs &a, hipStream_t st);

} // namespace pvba
