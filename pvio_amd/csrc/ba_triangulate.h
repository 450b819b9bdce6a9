// ba_triangulate.h -- batched multi-view DLT triangulation (pvio_hip_triangulate): buffers and launcher of the kernel of ba_triangulate.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pvba {

constexpr int kTriThreads = 256;  // workgroup size: four waves
constexpr int kTriMaxObs = 32;    // PVIO_TRI_MAX_OBS: a track's 2K rows fit the 64 lanes of a wave
constexpr int kTriSmallObs = 16;  // every track of a call has K <= 16: a track takes 32 lanes, two tracks share a wave
constexpr int kTriMaxSweeps = 30; // bound of the Jacobi loop for any input (LAPACK's dgesvj allows 30 as well); converged tracks need 4 to 7
constexpr int kTriRecord = 9;     // doubles of one track's result: q[4] | point[3] | score | ok (0.0 or 1.0)

inline int tri_group_lanes(int max_obs) { return max_obs <= kTriSmallObs ? 32 : 64; }

struct TriArgs { // passed by value; every pointer into the one device buffer of a call
    int32_t n_tracks;
    const double *view_P;     // [V][12]
    const int32_t *track_ptr; // [T+1]
    const int32_t *obs_view;  // [n_obs]
    const double *obs_z;      // [n_obs][2]
    int32_t *max_sweeps;      // one int, zeroed by the upload
    double *result;           // [T][kTriRecord]
};

hipError_t launch_triangulate(const TriArgs &a, int group_lanes, hipStream_t st);

} // namespace pvba
