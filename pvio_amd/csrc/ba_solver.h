// ba_solver.h -- host orchestration of the on-device bundle adjustment (one instance per pvio_hip_ctx).
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <string>
#include <vector>

#include "../../include/pvio_hip.h"
#include "ba_types.h"
#include "hip_buffer.h"

namespace pvba {

struct Comm; // RCCL communicator wrapper (ba_comm.cpp)
int comm_unique_id(uint8_t id[128]);
int comm_init(Comm **out, const uint8_t id[128], int rank, int world, int device);
int comm_allreduce(Comm *c, double *buf, size_t n, int op_max, hipStream_t st);
void comm_destroy(Comm *c);

class DevicePool { // grow-only device allocations keyed by name
  public:
    ~DevicePool();
    void *get(const char *name, size_t bytes, bool *grew = nullptr);
    void release();
    size_t total_bytes() const { return total_; }

  private:
    struct Slot {
        std::string name;
        void *ptr = nullptr;
        size_t bytes = 0;
    };
    std::vector<Slot> slots_;
    size_t total_ = 0;
};

struct UploadPlan; // what an upload derives on the host
struct UploadWork; // the View an upload is building
struct SolvePack;  // layout of a solve's packed read-back
struct MargGather; // layout of a marginalization's gathered read-back
struct TriLayout;  // layout of a triangulation call's device buffer
struct PlaneLayout; // layout of a plane RANSAC call's device buffer

class BASolver {
  public:
    BASolver(int device, int rank, int world, bool use_graph);
    void set_force_sharded(bool on) { sharded_ = world_ > 1 || on; }
    void set_fault_injection(int fail_factorizations, int invalid_steps) { dbg_fail_ = fail_factorizations, dbg_invalid_ = invalid_steps; }
    void set_linearize_mode(int m) { lin_mode_ = m; }
    void set_reuse_candidates(bool on) { reuse_cand_ = on; }
    int last_candidate_repeats() const { return last_repeats_; }
    int graph_replays() const { return graph_replays_; }
    ~BASolver();
    int upload(const pvio_ba_problem *pb, const pvio_ba_state *st, bool may_return_early = false);   // H2D of the flat problem + initial state
    // runs from the uploaded initial state; `read_back`: the accepted iterate + quality pass land in the caller's arrays as part of the same
    // stream round (what upload + solve + download cost as three round trips before)
    int solve(pvio_ba_summary *sum, pvio_ba_kernel_times *prof = nullptr, pvio_ba_state *read_back = nullptr);
    int download(pvio_ba_state *st);                                   // D2H of the accepted iterate (+ quality pass)
    int reprojection_error(double *out);
    int marginalize(const pvio_ba_problem *pb, const pvio_ba_state *st, int victim, pvio_ba_prior *out);
    int covariance(const pvio_ba_problem *pb, const pvio_ba_state *st, pvio_ba_covariance *out); // marginal covariances of the window (ba_cov.hip)
    const double *last_covariance_kernel_ms() const { return cov_ms_; } // k_cov_assemble, k_cov_invert, k_cov_landmarks of the last call (PVIO_HIP_TIMING)
    int triangulate(const pvio_tri_problem *pb, pvio_tri_result *out); // batched DLT triangulation (ba_triangulate.hip); leaves an uploaded window alone
    int last_triangulate_sweeps() const { return tri_sweeps_; }        // most Jacobi sweeps a track of the last call took
    double last_triangulate_kernel_ms() const { return tri_ms_; }      // k_triangulate of the last call (PVIO_HIP_TIMING)
    int plane_ransac(const pvio_plane_problem *pb, pvio_plane_result *out); // plane RANSAC + refit over points (ba_plane.hip); leaves an uploaded window alone
    int last_plane_hypotheses() const { return plane_scored_; }             // hypotheses k_plane_hypotheses scored in the last call
    const double *last_plane_kernel_ms() const { return plane_ms_; }        // k_plane_hypotheses, k_plane_refit of the last call (PVIO_HIP_TIMING)
    void set_comm(Comm *c) { comm_ = c; }
    const std::string &error() const { return err_; }
    hipStream_t stream() const { return stream_; }

  private:
    int fail(int code, const std::string &msg);
    int check(hipError_t e, const char *what);
    int run_slots(int n_slots);
    int enqueue_slot(hipEvent_t *ev = nullptr);
    void invalidate_graph();
    // the steps of solve() (ba_solver.cpp)
    class ProfileScope; // what solve(prof != nullptr) sets up, undone on every way out
    int request_solve_buffers(const SolvePack &pack, bool read_back, bool want_states, double **d_pack);
    int reset_for_solve(); // the control block's template (sent when it changes) + k_reset
    int profiled_slot(hipEvent_t *pev, pvio_ba_kernel_times *prof); // one eager slot, its events -> prof
    int time_limit_reached(std::chrono::steady_clock::time_point t0, bool *timed_out); // max_solver_time, agreed on by all ranks
    int fill_summary(pvio_ba_summary *sum, bool want_states, std::chrono::steady_clock::time_point t0);
    void unpack_results(const SolvePack &pack, pvio_ba_state *read_back) const; // the packed read-back -> the caller's arrays
    void dump_ctrl(const char *after); // PVIO_HIP_DEBUG_CTRL
    // shared by marginalize() and covariance()
    int linearize_once(int mode, int victim); // k_reset, control block, k_linearize, k_reduce on the window just uploaded
    int read_back_marg(const MargGather &lay, const double **h_back); // k_gather + one D2H copy + synchronize
    // the steps of triangulate() (ba_solver.cpp)
    int validate_tracks(const pvio_tri_problem *pb, const pvio_tri_result *out, TriLayout &lay);
    int stage_tracks(const pvio_tri_problem *pb, const TriLayout &lay);
    int launch_tracks(const TriLayout &lay);
    int fetch_tracks(const TriLayout &lay, pvio_tri_result *out);
    // the steps of plane_ransac() (ba_solver.cpp)
    int validate_points(const pvio_plane_problem *pb, const pvio_plane_result *out);
    int stage_points(const pvio_plane_problem *pb, const PlaneLayout &lay);
    int score_hypotheses(const PlaneLayout &lay, double threshold);
    int refit_winner(const PlaneLayout &lay, double threshold, const double *model);
    // the steps of upload() behind its argument checks (ba_solver.cpp)
    void plan_upload(const pvio_ba_problem *pb, UploadPlan &plan) const;
    int allocate(UploadWork &w);
    int stage_inputs(const pvio_ba_problem *pb, const pvio_ba_state *st, const UploadPlan &plan, UploadWork &w);
    int commit(const pvio_ba_problem *pb, const UploadWork &w, bool may_return_early);

    int device_, rank_, world_;
    bool sharded_; // world_ > 1, or forced for tests: eager launches + all-reduces + assembly from the reduced buffer
    bool use_graph_;
    int lin_mode_ = 0; // pvio_hip_opts::linearize_mode
    bool reuse_cand_ = false; // pvio_hip_opts::reuse_identical_candidates
    int last_repeats_ = 0;    // Ctrl::cand_repeats of the last solve
    int graph_replays_ = 0;   // hipGraphLaunch calls so far (diagnostics: pvio_hip_ba_graph_replays)
    int dbg_fail_ = 0, dbg_invalid_ = 0; // tests only: forced factorization failures / invalid steps per solve
    hipStream_t stream_ = nullptr;
    hipEvent_t ev0_ = nullptr, ev1_ = nullptr;
    DevicePool pool_;
    View v_{};
    pvhip::PinnedBuffer ctrl_pin_;
    Ctrl *h_ctrl_ = nullptr; // the one Ctrl in ctrl_pin_ (pinned, allocated once by the constructor)
    bool uploaded_ = false;
    int solves_since_upload_ = 0;
    int cus_ = 0;
    pvhip::PinnedBuffer h_stage_; // pinned staging of one upload's inputs
    bool stage_in_flight_ = false; // upload(may_return_early) left its staged copy queued; cleared by the next stream synchronization
    pvhip::PinnedBuffer h_back_; // pinned read-back of one marginalization pass (doubles)
    std::vector<double> marg_H_, marg_C_, marg_V_; // host work arrays of a marginalization (15N x 15N, twice 15(N-1) x 15(N-1))
    pvhip::PinnedBuffer h_cov_;  // pinned read-back of one covariance call
    hipEvent_t cov_ev_[4] = {nullptr, nullptr, nullptr, nullptr}; // around the three kernels of a covariance call, created on first use (PVIO_HIP_TIMING)
    double cov_ms_[3] = {0.0, 0.0, 0.0};
    pvhip::DeviceBuffer d_tri_;  // a triangulation call's inputs and results (its own: the window's buffers are not touched)
    pvhip::PinnedBuffer h_tri_;  // pinned staging of those inputs and read-back of those results
    hipEvent_t tri_ev_[2] = {nullptr, nullptr}; // around k_triangulate, created on first use (PVIO_HIP_TIMING)
    int tri_sweeps_ = 0;
    double tri_ms_ = 0.0;
    pvhip::DeviceBuffer d_plane_; // a plane RANSAC call's points, samples, counts, models, record and mask (its own: the window's buffers are not touched)
    pvhip::PinnedBuffer h_plane_; // pinned staging and read-back of the same layout
    hipEvent_t plane_ev_[4] = {nullptr, nullptr, nullptr, nullptr}; // around the two kernels, created on first use (PVIO_HIP_TIMING)
    int plane_scored_ = 0;
    double plane_ms_[2] = {0.0, 0.0};
    pvhip::PinnedBuffer h_pack_; // pinned: a solve's packed results (k_quality `pack`, doubles)
    const double *fs_init_ = nullptr, *rho_init_ = nullptr; // initial state inside the inputs slab
    Ctrl h_ctrl_tmpl_{};                                    // what a solve's control block starts from (k_reset copies the device copy)
    Ctrl *d_ctrl_tmpl_ = nullptr;
    int trace_cap_ = 0;
    hipGraph_t graph_ = nullptr;
    hipGraphExec_t graph_exec_ = nullptr;
    int graph_slots_ = 0;
    double max_solver_time_ = 0.0; // seconds; checked between graph replays
    bool sharded_graph_failed_ = false; // capturing the collectives failed once: eager launches from then on
    Comm *comm_ = nullptr;
    std::string err_;
    std::vector<double> h_init_fs_, h_init_rho_;
};

} // namespace pvba
