// ba_solver.cpp -- host side of the device-resident bundle adjustment.
//
// Replaces the ceres::Problem assembly + ceres::Solve call of BundleAdjustorSolver::solve
// (pvio/src/pvio/estimation/bundle_adjustor.cpp:63-299): the flat problem is uploaded once, the whole
// trust-region loop runs on the device (kernels in ba_kernels.hip), the host only replays a graph of
// "slots" (linearize -> reduce -> dense -> backsub) until the device-side state machine reports done.
//
// In order: upload in its five steps; the read-back layouts (SolvePack, MargGather, CovSlabs); solve in its steps (enqueue_slot, run_slots,
// request_solve_buffers, reset_for_solve, ProfileScope, profiled_slot, time_limit_reached, fill_summary, unpack_results); the one-shot calls
// marginalize and covariance above linearize_once; triangulate and plane_ransac in their steps.  The marginalization's dense host algebra is marg_prior.h.
#include "ba_solver.h"

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>

#include "ba_cov.h"
#include "ba_kernels.h"
#include "ba_plane.h"
#include "ba_triangulate.h"
#include "marg_prior.h"
#include "pv_plane.h"

namespace pvba {
constexpr bool kDenseLookAheadDefault = true; // same-box A/B (profiles/r3_ab_lookahead.txt): 12 076 -> 12 678 iterations/s
constexpr size_t kLinLdsBudget = 112 * 1024;  // bytes of LDS the chunks of k_linearize's plane and register-tile roles are sized for


DevicePool::~DevicePool() { release(); }
void DevicePool::release() {
    for (auto &s : slots_)
        if (s.ptr) (void)hipFree(s.ptr);
    slots_.clear();
    total_ = 0;
}
void *DevicePool::get(const char *name, size_t bytes, bool *grew) {
    if (bytes == 0) bytes = 8;
    for (auto &s : slots_)
        if (s.name == name) {
            if (s.bytes >= bytes) return s.ptr;
            (void)hipFree(s.ptr);
            total_ -= s.bytes;
            s.ptr = nullptr;
            const size_t nb = bytes + bytes / 2;
            if (hipMalloc(&s.ptr, nb) != hipSuccess) return nullptr;
            s.bytes = nb;
            total_ += nb;
            if (grew) *grew = true;
            return s.ptr;
        }
    // Headroom from the first allocation on: the windows of a sequence change shape with every keyframe (landmarks +-30 %), and a slot that is
    // sized exactly is freed and allocated again -- ~40 slots x (hipFree + hipMalloc) showed up as 0.3-0.4 ms on individual keyframe solves of the
    // rendered sequence (profiles/r4_prof_sequence_solves.txt).  288 GB of HBM: 50 % slack on the largest window (30 x 50 000: 0.4 GB) is nothing.
    Slot s;
    s.name = name;
    bytes = bytes + bytes / 2 < 4096 ? 4096 : bytes + bytes / 2;
    if (hipMalloc(&s.ptr, bytes) != hipSuccess) return nullptr;
    s.bytes = bytes;
    total_ += bytes;
    slots_.push_back(s);
    if (grew) *grew = true;
    return s.ptr;
}

BASolver::BASolver(int device, int rank, int world, bool use_graph) : device_(device), rank_(rank), world_(world), sharded_(world > 1), use_graph_(use_graph) {
    (void)hipSetDevice(device_);
    (void)hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking);
    (void)hipEventCreate(&ev0_);
    (void)hipEventCreate(&ev1_);
    h_ctrl_ = static_cast<Ctrl *>(ctrl_pin_.reserve(sizeof(Ctrl), sizeof(Ctrl)));
}
BASolver::~BASolver() {
    invalidate_graph();
    if (ev0_) (void)hipEventDestroy(ev0_);
    if (ev1_) (void)hipEventDestroy(ev1_);
    for (hipEvent_t ev : cov_ev_)
        if (ev) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : tri_ev_)
        if (ev) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : plane_ev_)
        if (ev) (void)hipEventDestroy(ev);
    if (stream_) (void)hipStreamDestroy(stream_);
}
int BASolver::fail(int code, const std::string &msg) {
    err_ = msg;
    return code;
}
int BASolver::check(hipError_t e, const char *what) {
    if (e == hipSuccess) return PVIO_OK;
    return fail(PVIO_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
void BASolver::invalidate_graph() {
    if (graph_exec_) (void)hipGraphExecDestroy(graph_exec_);
    if (graph_) (void)hipGraphDestroy(graph_);
    graph_exec_ = nullptr;
    graph_ = nullptr;
    graph_slots_ = 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// upload = validate -> plan -> allocate -> stage -> commit.  validate and plan touch neither the device nor the solver;
// from allocate's first pool request until commit the context is between windows (upload() itself says what that means).
// ---------------------------------------------------------------------------------------------------------------------

struct Reject { // a failed argument check: what upload() returns and reports
    int code = PVIO_OK;
    const char *msg = "";
    int group = -1; // check_landmarks only: the run of upload's order of checks the failing one belongs to
};

// The checks of the landmark and observation arrays, shared with marg_subset.  validate_upload makes the other arrays' checks between them, in the
// order upload() has always made them (the first failing check decides code and message), so a failure names its run: 0 the counts, 1 null arrays and
// CSR ends, 2 the walk over the landmarks, 3 the multiplicities.  lm_seen[l], bit f: landmark l is observed in frame f (what the duplicate check
// builds; View::lm_seen).  Needs pb and st only.
static Reject check_landmarks(const pvio_ba_problem *pb, const pvio_ba_state *st, std::vector<uint32_t> &lm_seen) {
    const int N = pb->n_frames, M = pb->n_landmarks, F = pb->n_obs;
    if (N < 1 || N > kMaxFrames) return {PVIO_ERR_UNSUPPORTED, "n_frames must be in [1, 32]", 0};
    if (M < 0 || F < 0 || (M > 0 && !st->lm_inv_depth)) return {PVIO_ERR_INVALID_ARGUMENT, "bad landmark arrays", 0};
    if (M > 0 && (!pb->lm_anchor_frame || !pb->lm_anchor_z || !pb->lm_obs_ptr)) return {PVIO_ERR_INVALID_ARGUMENT, "null landmark array", 1};
    if (F > 0 && (!pb->obs_frame || !pb->obs_z)) return {PVIO_ERR_INVALID_ARGUMENT, "null observation array", 1};
    if (M > 0 && (pb->lm_obs_ptr[0] != 0 || pb->lm_obs_ptr[M] != F)) return {PVIO_ERR_INVALID_ARGUMENT, "lm_obs_ptr must start at 0 and end at n_obs", 1};
    lm_seen.assign((size_t)std::max(M, 1), 0u);
    int maxK = 1;
    for (int l = 0; l < M; ++l) {
        const int b = pb->lm_obs_ptr[l], e = pb->lm_obs_ptr[l + 1];
        if (b < 0 || e < b || e > F) return {PVIO_ERR_INVALID_ARGUMENT, "lm_obs_ptr is not a valid CSR", 2};
        const int a = pb->lm_anchor_frame[l];
        if (a < 0 || a >= N) return {PVIO_ERR_INVALID_ARGUMENT, "anchor frame out of range", 2};
        maxK = std::max(maxK, e - b);
        uint32_t seen = 0;
        for (int o = b; o < e; ++o) {
            const int t = pb->obs_frame[o];
            if (t < 0 || t >= N || t == a) return {PVIO_ERR_INVALID_ARGUMENT, "observation frame out of range or equal to the anchor", 2};
            if (seen & (1u << t)) return {PVIO_ERR_UNSUPPORTED, "a landmark lists the same target frame twice", 2};
            seen |= 1u << t;
        }
        lm_seen[(size_t)l] = seen;
    }
    if (maxK > kLinThreads) return {PVIO_ERR_UNSUPPORTED, "too many observations per landmark", 2};
    if (pb->lm_multiplicity)
        for (int l = 0; l < M; ++l)
            if (pb->lm_multiplicity[l] < 1) return {PVIO_ERR_INVALID_ARGUMENT, "lm_multiplicity must be >= 1", 3};
    return {};
}

// validate: every argument check of an upload.  No HIP call, nothing of the solver read or written.
static Reject validate_upload(const pvio_ba_problem *pb, const pvio_ba_state *st, std::vector<uint32_t> &lm_seen) {
    if (!pb || !st || !st->frame_state) return {PVIO_ERR_INVALID_ARGUMENT, "null problem/state"};
    const Reject lm = check_landmarks(pb, st, lm_seen);
    if (lm.group == 0) return lm;
    const int N = pb->n_frames;
    if (!pb->frame_fixed || !pb->cam_extrinsic || !pb->imu_extrinsic || !pb->sqrt_inv_cov || !pb->intrinsics) return {PVIO_ERR_INVALID_ARGUMENT, "null per-frame array"};
    if (lm.group == 1) return lm;
    if (pb->prior_n < 0 || pb->prior_n > N || pb->max_iterations < 0 || pb->n_plane_factors < 0) return {PVIO_ERR_INVALID_ARGUMENT, "negative count / prior_n > n_frames"};
    if (pb->prior_n > 0 && (!pb->prior_frames || !pb->prior_S || !pb->prior_s || !pb->prior_lin_state)) return {PVIO_ERR_INVALID_ARGUMENT, "null prior array"};
    if (pb->use_inertial && (!pb->preint_valid || !pb->preint_delta || !pb->preint_sqrt_inv_cov || !pb->preint_jacobian)) return {PVIO_ERR_INVALID_ARGUMENT, "null pre-integration array"};
    if (pb->n_plane_factors > 0) {
        if (!pb->plane_obs_ptr || !pb->plane_obs_frame || !pb->plane_obs_z || !pb->plane_normal || !pb->plane_distance) return {PVIO_ERR_INVALID_ARGUMENT, "null plane array"};
        if (pb->plane_obs_ptr[0] != 0) return {PVIO_ERR_INVALID_ARGUMENT, "plane_obs_ptr must start at 0"};
        for (int f = 0; f < pb->n_plane_factors; ++f) {
            if (pb->plane_obs_ptr[f + 1] < pb->plane_obs_ptr[f]) return {PVIO_ERR_INVALID_ARGUMENT, "plane_obs_ptr is not a valid CSR"};
            for (int o = pb->plane_obs_ptr[f]; o < pb->plane_obs_ptr[f + 1]; ++o)
                if (pb->plane_obs_frame[o] < 0 || pb->plane_obs_frame[o] >= N) return {PVIO_ERR_INVALID_ARGUMENT, "plane observation frame out of range"};
        }
    }
    if (lm.group == 2) return lm;
    for (int i = 0; i < pb->prior_n; ++i)
        if (pb->prior_frames[i] < 0 || pb->prior_frames[i] >= N) return {PVIO_ERR_INVALID_ARGUMENT, "prior frame out of range"};
    if (pb->n_rot_priors < 0 || (pb->n_rot_priors > 0 && (!pb->rot_prior_frame || !pb->rot_prior_q0 || !pb->rot_prior_sqrt_info)))
        return {PVIO_ERR_INVALID_ARGUMENT, "bad rotation prior arrays"};
    uint32_t has_rot = 0;
    for (int i = 0; i < pb->n_rot_priors; ++i) {
        const int f = pb->rot_prior_frame[i];
        if (f < 0 || f >= N) return {PVIO_ERR_INVALID_ARGUMENT, "rotation prior frame out of range"};
        if (has_rot & (1u << f)) return {PVIO_ERR_UNSUPPORTED, "more than one rotation prior on a frame"};
        has_rot |= 1u << f;
    }
    return lm; // the multiplicities' failure, or none
}

// Experiment switches of the planning (unsupported).  Read once per process, at the first upload that gets as far as its plan.
struct UploadSwitches {
    int lm_wgs;          // PVIO_HIP_LM_WGS=n caps the landmark workgroups of k_linearize (>= 1; the plan clamps it to 4 x CUs -- the partial-row buffers are sized
                         // from the resulting grid, so any value in the range is safe; anything else is ignored)
    bool fuse_off;       // PVIO_HIP_FUSE_BACKSUB=0: tests -- small windows through the separate k_backsub launch, i.e. the split-finalize form
    int fuse_max;        // PVIO_HIP_FUSE_BACKSUB_MAX: experiments -- the landmark count up to which the back-substitution stays inside k_dense; clamped to 16 .. 4096
    bool split_off;      // PVIO_HIP_SPLIT_FIN=0 keeps everything in k_dense (A/B timing, tests of both forms)
    int dense_la;        // PVIO_HIP_DENSE_LA=0 / 1 overrides the default form of the register-resident factorization; -1: not set
    bool img_scaled_off; // PVIO_HIP_IMG_SCALED=0: k_dense scales the image every time
};
static const UploadSwitches &upload_switches() {
    static const UploadSwitches sw = [] {
        auto env = [](const char *name, int unset) {
            const char *s = std::getenv(name);
            return s ? std::atoi(s) : unset;
        };
        UploadSwitches s;
        s.lm_wgs = env("PVIO_HIP_LM_WGS", 0);
        s.fuse_off = env("PVIO_HIP_FUSE_BACKSUB", 1) == 0;
        s.fuse_max = std::min(4096, std::max(16, env("PVIO_HIP_FUSE_BACKSUB_MAX", 256)));
        s.split_off = env("PVIO_HIP_SPLIT_FIN", 1) == 0;
        s.dense_la = env("PVIO_HIP_DENSE_LA", -1);
        s.img_scaled_off = env("PVIO_HIP_IMG_SCALED", 1) == 0;
        return s;
    }();
    return sw;
}

// Diagnostic and test switches of the calls behind an upload.  Read once per process, at the first call that asks.
struct SolverSwitches {
    bool debug_ctrl;    // PVIO_HIP_DEBUG_CTRL=1 (plain launches only): the control block as each kernel of a slot leaves it (dump_ctrl)
    bool sharded_graph; // PVIO_HIP_SHARDED_GRAPH=0 turns the capture of landmark-sharded slots off (run_slots)
    bool timing;        // PVIO_HIP_TIMING=1: where the host's time of a solve and of a marginalization goes; hipEvents around the kernels of a covariance call
    int timeout_rank;   // PVIO_HIP_DEBUG_TIMEOUT_RANK, tests: only this rank sees its clock run out (the ranks must still leave in the same round); -1: not set
};
static const SolverSwitches &solver_switches() {
    static const SolverSwitches sw = [] {
        const char *sg = std::getenv("PVIO_HIP_SHARDED_GRAPH"), *tr = std::getenv("PVIO_HIP_DEBUG_TIMEOUT_RANK");
        return SolverSwitches{std::getenv("PVIO_HIP_DEBUG_CTRL") != nullptr, !(sg != nullptr && std::atoi(sg) == 0), std::getenv("PVIO_HIP_TIMING") != nullptr, tr ? std::atoi(tr) : -1};
    }();
    return sw;
}

using Clock = std::chrono::steady_clock;
static double us(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::micro>(b - a).count(); }

// Everything an upload derives on the host.  Owns the derived arrays until the DMA has left: staging sends the large ones from where they lie.
struct UploadPlan {
    Dims dm{}; // complete (compared with memcmp, passed to every kernel)
    std::vector<uint8_t> pose_active, motion_active, pre_valid, chunk_perm;
    std::vector<int32_t> obs_lm, prior_slot, rot_slot, plane_chunk, chunk_lm, chunk_tptr, chunk_geo, tp_tile_dst, task_desc;
    std::vector<uint32_t> lm_seen; // (validate's by-product)
    std::vector<double> lm_mult;   // duplicate residual blocks (bundle_adjustor.cpp:165-179); empty: no landmark counts twice
};

// landmark ranges of <= lm_slots landmarks and <= 256 factors (one thread per factor), cut where the anchor frame changes if `one_anchor`
static std::vector<int32_t> cut_chunks(const pvio_ba_problem *pb, int lm_slots, bool one_anchor) {
    const int M = pb->n_landmarks;
    std::vector<int32_t> chunk_lm(1, 0);
    int cnt = 0, fac = 0;
    for (int l = 0; l < M; ++l) {
        const int k = pb->lm_obs_ptr[l + 1] - pb->lm_obs_ptr[l];
        if (cnt > 0 && (cnt + 1 > lm_slots || fac + k > kLinThreads || (one_anchor && pb->lm_anchor_frame[l] != pb->lm_anchor_frame[l - 1]))) {
            chunk_lm.push_back(l);
            cnt = 0, fac = 0;
        }
        ++cnt, fac += k;
    }
    if (M > 0) chunk_lm.push_back(M);
    return chunk_lm;
}

// Register-tile role.  A small window is latency-bound per workgroup, so chunks are sized to put one chunk on every CU (256 on MI355X) rather than to
// fill the LDS; a larger one falls back to LDS-filling chunks that each workgroup walks in a grid-stride loop.
// One workgroup fits on a CU (registers, LDS) and the IMU / prior workgroups are the longest: the landmark chunks get the CUs that are left, so that
// the whole grid is resident at once instead of queueing a second round behind it.  One landmark chunk per free CU.  Round 5 measured the alternative
// the 22x traffic of the partial rows suggests -- fewer, fatter workgroups, i.e. fewer rows for k_reduce to sum (PVIO_HIP_LM_WGS;
// profiles/r5_ab_partials.txt): the traffic falls with the count and the iteration rate with it, because a workgroup's chain grows with the landmarks
// it holds (the per-landmark sums and the tile accumulation walk them one after another): 48 rows = 12 161 against 14 112 iterations/s, k_linearize
// 18.4 -> 29.2 us for 0.4 us less in k_reduce.
static void plan_register_tile_chunks(const pvio_ba_problem *pb, int cus, int lm_wgs_cap, UploadPlan &pl) {
    Dims &dm = pl.dm;
    // (the cap may exceed the free CUs: more than one workgroup per CU where registers and LDS allow)
    const int lm_cus = lm_wgs_cap > 0 ? lm_wgs_cap : std::max(1, cus - dm.G_plane - dm.G_pre - dm.G_prior);
    const int slots_lds = (int)std::max<size_t>(1, std::min<size_t>(kLinLdsBudget / 8 / (40 * dm.N + 46), (size_t)kLinThreads));
    dm.lm_slots = std::min(slots_lds, std::max(1, (dm.M + lm_cus - 1) / lm_cus));
    pl.chunk_lm = cut_chunks(pb, dm.lm_slots, false);
    dm.n_chunks = (int)pl.chunk_lm.size() - 1;
    dm.G_lm = std::max(1, std::min(dm.n_chunks, lm_cus));
}

// scatter table of the Schur tiles' accumulator entries into the element-major 3 x 3-task partial row (the flush of ba_lin_tp.h): entry r of lane l of
// tile (bi, bj) is element (16 bi + (l >> 4) + 4 r, 16 bj + (l & 15)) of the lower triangle
static std::vector<int32_t> tp_tile_dst_table(int N, int P6) {
    std::vector<int32_t> table;
    const int nbt = tp_u_stride(P6) >> 4;
    auto task_index = [&](int fi, int fj, int si, int sj) { return 4 * (fi * N - ((fi * (fi - 1)) >> 1) + (fj - fi)) + 2 * si + sj; };
    for (int bi = 0; bi < nbt; ++bi)
        for (int bj = 0; bj <= bi; ++bj)
            for (int l = 0; l < 64; ++l)
                for (int r = 0; r < 4; ++r) {
                    const int I = 16 * bi + (l >> 4) + 4 * r, J = 16 * bj + (l & 15);
                    int32_t dst = -1;
                    if (I < P6 && J <= I) {
                        const int fI = I / 6, iI = I % 6, fJ = J / 6, jJ = J % 6; // fJ <= fI
                        // partial_entry(N, fI, iI, fJ, jJ) of ba_kernels.hip: off-diagonal blocks once (smaller frame = row of the task)
                        const int el = fI == fJ ? 3 * (iI % 3) + (jJ % 3) : 3 * (jJ % 3) + (iI % 3);
                        const int t = fI == fJ ? task_index(fI, fI, iI / 3, jJ / 3) : task_index(fJ, fI, jJ / 3, iI / 3);
                        dst = (el << 24) | t;
                    }
                    table.push_back(dst);
                }
    return table;
}

// Large-window role (ba_lin_tp.h): chunks of <= 256 factors whose landmarks share ONE anchor frame (a chunk is cut where the anchor changes: the
// reference's block order is anchor-sorted, any other order only makes more chunks), as many landmarks as the LDS holds U rows for; every chunk's
// factors sorted by target frame (the direct part of J^T J is accumulated per target).  Needs dm.lm_mm and the other roles' grids.
static void plan_large_window_chunks(const pvio_ba_problem *pb, int cus, int lm_wgs_cap, UploadPlan &pl) {
    Dims &dm = pl.dm;
    const int N = dm.N, M = dm.M, F = dm.F;
    pl.tp_tile_dst = tp_tile_dst_table(N, dm.P6);
    dm.lm_slots = tp_landmark_slots(dm, F > 0 ? (int)(((long long)kLinThreads * M + F - 1) / F) : 64);
    pl.chunk_lm = cut_chunks(pb, dm.lm_slots, true);
    const std::vector<int32_t> &chunk_lm = pl.chunk_lm;
    dm.n_chunks = (int)chunk_lm.size() - 1;
    // two workgroups per CU where their LDS allows (tp_landmark_slots) and the kernel is held to 256 registers (k_linearize<T <= 2, true>)
    const int per_cu = (linearize_lds_bytes(dm) <= 80 * 1024 && tiles_per_thread(dm) <= 2) ? 2 : 1;
    dm.G_lm = std::max(1, std::min(dm.n_chunks, lm_wgs_cap > 0 ? lm_wgs_cap : per_cu * cus - (dm.G_plane + dm.G_pre + dm.G_prior)));
    if (dm.n_chunks > 0) { // contiguous chunk ranges (a range mostly shares one anchor frame): no more workgroups than ranges
        const int per_wg = (dm.n_chunks + dm.G_lm - 1) / dm.G_lm;
        dm.G_lm = std::max(1, (dm.n_chunks + per_wg - 1) / per_wg);
    }
    pl.chunk_geo.assign((size_t)dm.n_chunks * 8, 0);
    pl.chunk_tptr.assign((size_t)dm.n_chunks * (N + 1), 0);
    pl.chunk_perm.assign((size_t)std::max(F, 1), 0);
    for (int c = 0; c < dm.n_chunks; ++c) {
        const int o0 = pb->lm_obs_ptr[chunk_lm[c]], o1 = pb->lm_obs_ptr[chunk_lm[c + 1]];
        int32_t *g = pl.chunk_geo.data() + (size_t)c * 8;
        g[0] = chunk_lm[c], g[1] = chunk_lm[c + 1] - chunk_lm[c], g[2] = o0, g[3] = o1 - o0;
        g[4] = pb->lm_anchor_frame[chunk_lm[c]];
        int32_t *tp = pl.chunk_tptr.data() + (size_t)c * (N + 1);
        for (int o = o0; o < o1; ++o) ++tp[pb->obs_frame[o] + 1];
        for (int t = 0; t < N; ++t) tp[t + 1] += tp[t];
        int fill[kMaxFrames] = {0};
        for (int o = o0; o < o1; ++o) { // counting sort, stable: a target's factors in landmark order
            const int t = pb->obs_frame[o];
            pl.chunk_perm[(size_t)o0 + tp[t] + fill[t]++] = (uint8_t)(o - o0);
        }
    }
}

// plan: the validated problem + the solver's configuration -> what the kernels are configured by.  No HIP call, no member written.
void BASolver::plan_upload(const pvio_ba_problem *pb, UploadPlan &pl) const {
    const UploadSwitches &sw = upload_switches();
    const int N = pb->n_frames, M = pb->n_landmarks, F = pb->n_obs, cus = cus_;
    Dims &dm = pl.dm;
    dm.N = N, dm.M = M, dm.F = F;
    dm.use_inertial = pb->use_inertial ? 1 : 0;
    dm.prior_n = pb->prior_n;
    dm.d = (dm.use_inertial || dm.prior_n > 0) ? 15 : 6;
    dm.P = dm.d * N, dm.P6 = 6 * N;
    dm.n_tasks = 4 * N * (N + 1) / 2;
    dm.max_iter = pb->max_iterations;
    dm.world = world_, dm.rank = rank_;
    dm.n_plane = pb->n_plane_factors;
    dm.n_rot = pb->n_rot_priors;

    // ---- block usage (Ceres removes constant and unreferenced parameter blocks from the reduced program) ----
    std::vector<uint8_t> pose_used(N, 0), motion_used(N, 0);
    pl.pre_valid.assign(N, 0);
    pl.obs_lm.assign(F, 0);
    uint32_t seen_any = 0; // bit f: frame f is some landmark's target
    for (int l = 0; l < M; ++l) {
        const int b = pb->lm_obs_ptr[l], e = pb->lm_obs_ptr[l + 1];
        if (e > b) pose_used[pb->lm_anchor_frame[l]] = 1;
        std::fill(pl.obs_lm.begin() + b, pl.obs_lm.begin() + e, l);
        seen_any |= pl.lm_seen[(size_t)l];
    }
    for (int f = 0; f < N; ++f)
        if ((seen_any >> f) & 1u) pose_used[f] = 1;
    if (dm.use_inertial)
        for (int j = 1; j < N; ++j)
            if (pb->preint_valid[j]) {
                pl.pre_valid[j] = 1;
                pose_used[j - 1] = pose_used[j] = motion_used[j - 1] = motion_used[j] = 1;
            }
    pl.prior_slot.assign(N, -1); // frame -> slot of the prior (the last one that names it, like the kernels' old search)
    for (int i = 0; i < dm.prior_n; ++i) {
        const int f = pb->prior_frames[i];
        pose_used[f] = motion_used[f] = 1;
        pl.prior_slot[f] = i;
    }
    pl.rot_slot.assign(N, -1); // rotation priors: at most one per frame; one on a fixed frame is a constant block and is dropped
    for (int i = 0; i < dm.n_rot; ++i) {
        pl.rot_slot[pb->rot_prior_frame[i]] = i;
        pose_used[pb->rot_prior_frame[i]] = 1;
    }
    for (int f = 0; f < dm.n_plane; ++f) {
        bool any_free = false;
        for (int o = pb->plane_obs_ptr[f]; o < pb->plane_obs_ptr[f + 1]; ++o) any_free |= !pb->frame_fixed[pb->plane_obs_frame[o]];
        if (any_free)
            for (int o = pb->plane_obs_ptr[f]; o < pb->plane_obs_ptr[f + 1]; ++o) pose_used[pb->plane_obs_frame[o]] = 1;
    }
    pl.pose_active.assign(N, 0), pl.motion_active.assign(N, 0);
    for (int i = 0; i < N; ++i) {
        pl.pose_active[i] = pose_used[i] && !pb->frame_fixed[i];
        pl.motion_active[i] = (dm.d == 15) && motion_used[i];
    }
    if (pb->lm_multiplicity && std::any_of(pb->lm_multiplicity, pb->lm_multiplicity + M, [](int32_t m) { return m != 1; }))
        pl.lm_mult.assign(pb->lm_multiplicity, pb->lm_multiplicity + M);

    // ---- the roles of k_linearize: plane chunks, one workgroup per IMU factor and per prior frame, landmark chunks ----
    dm.plane_slots = (int)std::max<size_t>(1, std::min<size_t>(kLinLdsBudget / 8 / (dm.P6 + 2), (size_t)kLinThreads));
    for (int f = 0; f <= dm.n_plane; f += dm.plane_slots) pl.plane_chunk.push_back(f);
    if (pl.plane_chunk.back() != dm.n_plane) pl.plane_chunk.push_back(dm.n_plane);
    dm.n_plane_chunks = (int)pl.plane_chunk.size() - 1;
    dm.G_plane = dm.n_plane > 0 ? std::max(1, std::min(dm.n_plane_chunks, std::max(1, cus / 4))) : 0;
    dm.G_pre = dm.use_inertial ? N - 1 : 0;
    dm.G_prior = dm.prior_n; // one workgroup per prior frame
    // Large windows take the throughput role (ba_lin_tp.h: chunks of 256 factors walked by workgroups that keep their accumulators, Schur complement on the
    // matrix cores); its prologue + flush + first chunk cost ~30 us whatever the window, the register-tile role's time grows with the landmarks per workgroup:
    // same-box A/B over 6 .. 24 frames (profiles/r6_lin_mode_ab.txt): they cross at ~40 000 factors (10 x 5000: 35.7 -> 32.4 us, 10 x 10 000: 66.7 -> 40.2 us,
    // 16 x 3000: 48.4 -> 41.0 us; 10 x 3000: 28.1 against 31.3 us, 6 x 3000: 24.5 against 34.5 us)
    // (a window without landmarks has no chunks: the register-tile role's empty walk handles it)
    dm.lm_mm = ((lin_mode_ == 2 && M > 0) || (lin_mode_ == 0 && F >= 40000)) ? 1 : 0;
    const int lm_wgs_cap = sw.lm_wgs >= 1 ? std::min(sw.lm_wgs, 4 * cus) : 0;
    if (dm.lm_mm) plan_large_window_chunks(pb, cus, lm_wgs_cap, pl);
    else plan_register_tile_chunks(pb, cus, lm_wgs_cap, pl);
    // pvio_hip_opts::reuse_identical_candidates.  Not on landmark shards: their k_reduce feeds an all-reduce that sums IN PLACE, a skipped slot
    // would add the last slot's sums to themselves.
    dm.reuse_cand = (reuse_cand_ && !sharded_) ? 1 : 0;

    // ---- back-substitution: 16 landmarks per workgroup pass (16 lanes each); <= 64 partial rows (one per lane of the wave that sums them) until a
    // large window needs the whole chip ----
    dm.G_back = M <= 4096 ? std::max(1, std::min(64, (M + 15) / 16)) : std::min(cus, (M + 63) / 64);
    dm.fuse_backsub = (!sharded_ && M <= sw.fuse_max && !sw.fuse_off) ? 1 : 0; // beyond one landmark per thread the separate launch is faster
    dm.n_back_rows = (sharded_ || dm.fuse_backsub) ? 1 : dm.G_back;
    for (int fi = 0; fi < N; ++fi) // 3x3 tile tasks over the upper block triangle
        for (int fj = fi; fj < N; ++fj)
            for (int s = 0; s < 4; ++s) pl.task_desc.push_back(fi | (fj << 8) | ((s >> 1) << 16) | ((s & 1) << 17));

    // ---- k_dense.  Tile image: k_reduce also assembles the reduced system entry by entry where the dense kernel's tile owners load it from (single
    // GPU, system resident in LDS/registers; landmark-sharded runs build it from the all-reduced `red`: k_reduce phase 2) ----
    int lds_matrix = 0;
    dense_lds_bytes(dm, &lds_matrix);
    dm.use_img = 1;
    dm.img_sz = (int)dense_tile_doubles(dm);
    // split finalize: with a separate k_backsub launch on one GPU, k_dense leaves the gradient max-norm, the state / trace copies and
    // (register-resident factorization: the image is what it factors) the pose part of v^T H v to that launch.
    // (landmark shards: every rank runs the same finalize workgroup on the same all-reduced data; the pose part of v^T H v is formed by
    // rank 0's k_backsub alone -- the exchange step behind it sums the ranks' rows)
    dm.split_fin = (!dm.fuse_backsub && !sw.split_off) ? 1 : 0;
    dm.qvv_back = (dm.split_fin && lds_matrix) ? 1 : 0;
    // look-ahead form of the register-resident factorization
    dm.dense_la = (lds_matrix && (sw.dense_la < 0 ? kDenseLookAheadDefault : sw.dense_la != 0)) ? 1 : 0;
    // the image in the form the accumulators hold once the scaling exists
    dm.img_scaled = (dm.dense_la && dm.split_fin && dm.qvv_back && !sw.img_scaled_off) ? 1 : 0;
}

// What allocate and stage hand to commit.
struct UploadWork {
    View v{};
    const double *fs_init = nullptr, *rho_init = nullptr; // initial state inside the inputs slab
    bool grew = false;          // a pool slot was allocated or moved: the captured graph holds stale addresses
    bool sent_directly = false; // an array went from where it lay, asynchronously: the stream must drain before upload() returns
};

template <typename T>
static bool dev(DevicePool &pool, const char *name, size_t n, T **dst, bool *grew) {
    T *p = static_cast<T *>(pool.get(name, n * sizeof(T), grew));
    *dst = p;
    return p != nullptr;
}

// allocate: state and work buffers of a window of w.v.dm's shape, zeroed where the kernels expect it.
int BASolver::allocate(UploadWork &w) {
    View &v = w.v;
    const Dims &dm = v.dm;
    bool *grew = &w.grew, ok = true;
    const size_t Ns = dm.N, Ms = std::max(dm.M, 1), Fs = std::max(dm.F, 1), Dp = 15 * (size_t)dm.prior_n, P = dm.P;
    double *Lambda = nullptr, *eta = nullptr, *ST = nullptr; // written by k_prior_prep (stage), read-only from then on
    ok &= dev(pool_, "prior_Lambda", Dp * Dp, &Lambda, grew);
    ok &= dev(pool_, "prior_eta", Dp, &eta, grew);
    ok &= dev(pool_, "prior_ST", Dp * Dp, &ST, grew);
    v.prior_Lambda = Lambda, v.prior_eta = eta, v.prior_ST = ST;
    ok &= dev(pool_, "ctrl", 1, &v.ctrl, grew);
    ok &= dev(pool_, "cand_rec", 24, &v.cand_rec, grew);
    ok &= dev(pool_, "fs", 2 * Ns * 16, &v.fs, grew);
    ok &= dev(pool_, "fs_user", Ns * 16, &v.fs_user, grew);
    ok &= dev(pool_, "bias0_lin", Ns * 6, &v.bias0_lin, grew);
    ok &= dev(pool_, "rho", 2 * Ms, &v.rho, grew);
    ok &= dev(pool_, "cl", Ms, &v.cl, grew);
    ok &= dev(pool_, "Hll", 2 * Ms, &v.Hll, grew);
    ok &= dev(pool_, "bl", 2 * Ms, &v.bl, grew);
    ok &= dev(pool_, "Dl", 2 * Ms, &v.Dl, grew);
    ok &= dev(pool_, "ghl", 2 * Ms, &v.ghl, grew);
    ok &= dev(pool_, "gnl", 2 * Ms, &v.gnl, grew);
    ok &= dev(pool_, "Wa", 2 * Ms * 6, &v.Wa, grew);
    ok &= dev(pool_, "Wt", 2 * Fs * 6, &v.Wt, grew);
    const size_t G = (size_t)dm.G_lm + dm.G_plane, nS = (size_t)dm.n_tasks * 9, nV = (size_t)kNumPoseVec * dm.P6;
    ok &= dev(pool_, "part_S", G * nS, &v.part_S, grew);
    ok &= dev(pool_, "part_vec", G * nV, &v.part_vec, grew);
    ok &= dev(pool_, "part_scal", G * kNumLinScal, &v.part_scal, grew);
    ok &= dev(pool_, "red", nS + nV + kNumLinScal + (size_t)world_, &v.red, grew); // + one max slot per rank
    ok &= dev(pool_, "back_part", (size_t)std::max(dm.G_back, 1) * kNumBackScal, &v.back_part, grew);
    ok &= dev(pool_, "back_red", kNumBackScal, &v.back_red, grew);
    ok &= dev(pool_, "pre_H", Ns * 900, &v.pre_H, grew);
    ok &= dev(pool_, "pre_g", Ns * 30, &v.pre_g, grew);
    ok &= dev(pool_, "pre_cost", Ns, &v.pre_cost, grew);
    ok &= dev(pool_, "prior_H", Dp * Dp, &v.prior_H, grew);
    ok &= dev(pool_, "prior_g", Dp, &v.prior_g, grew);
    ok &= dev(pool_, "prior_cost", (size_t)std::max(dm.prior_n, 1), &v.prior_cost, grew);
    {
        // arrays the kernels read for every frame whether the window has the factor or not: the prior's gradient / diagonal by frame
        // (k_dense's vector assembly; frames without a prior slot stay zero) and the rotation-prior blocks (k_reduce / k_dense; zero
        // when the window has none).  One block, one memset.
        double *zb = nullptr;
        ok &= dev(pool_, "zero_block", Ns * 42 + 1, &zb, grew);
        v.prior_gd = zb, v.rot_H = zb + Ns * 30, v.rot_g = v.rot_H + Ns * 9, v.rot_cost = v.rot_g + Ns * 3;
        if (ok && check(hipMemsetAsync(zb, 0, (dm.n_rot == 0 ? Ns * 42 + 1 : Ns * 30) * sizeof(double), stream_), "memset zero block")) return PVIO_ERR_HIP;
    }
    ok &= dev(pool_, "Smat", dense_tile_doubles(dm), &v.Smat, grew);
    // the tile image is zero wherever nothing is ever written (+ one tile of zeros behind it: what k_dense's waves load into the accumulator
    // slots they do not own)
    ok &= dev(pool_, "img", (size_t)dm.img_sz + 256, &v.img, grew);
    if (ok && dm.use_img && check(hipMemsetAsync(v.img, 0, ((size_t)dm.img_sz + 256) * sizeof(double), stream_), "memset img")) return PVIO_ERR_HIP;
    ok &= dev(pool_, "cp", P, &v.cp, grew);
    ok &= dev(pool_, "cpl", P, &v.cpl, grew);
    ok &= dev(pool_, "vraw", P, &v.vraw, grew);
    ok &= dev(pool_, "Dp", P, &v.Dp, grew);
    ok &= dev(pool_, "gtot", P, &v.gtot, grew);
    ok &= dev(pool_, "ghp", P, &v.ghp, grew);
    ok &= dev(pool_, "vstep", P, &v.vstep, grew);
    ok &= dev(pool_, "ystep", P, &v.ystep, grew);
    ok &= dev(pool_, "lm_quality", Ms, &v.lm_quality, grew);
    ok &= dev(pool_, "lm_valid", Ms, &v.lm_valid, grew);
    ok &= dev(pool_, "trace", (size_t)dm.max_iter + 2, &v.trace, grew);
    if (!ok) return fail(PVIO_ERR_OUT_OF_MEMORY, "device allocation / upload failed");
    return PVIO_OK;
}

// Host inputs of one upload: gathered in ONE pinned staging buffer and sent with ONE DMA into one device slab (a window is
// ~35 small arrays; a pageable hipMemcpyAsync each cost more than the solve's first iterations).  Offsets are 256-byte
// aligned; an array that is not given (null) keeps its place uninitialized, like the separate allocations it replaces.
struct StagedUpload {
    struct Item {
        const void *src;
        size_t bytes, off;
        const void **dst;
    };
    std::vector<Item> items; // offsets are assigned when the upload is flushed
    template <typename T>
    void add(const T *src, size_t n, const T **dst) {
        const size_t bytes = n * sizeof(T);
        items.push_back({(n && src) ? static_cast<const void *>(src) : nullptr, bytes, 0, reinterpret_cast<const void **>(dst)});
    }
    template <typename T>
    void add(const std::vector<T> &src, const T **dst) { add(src.data(), src.size(), dst); } // (an empty vector: no source)
};

// stage: the caller's arrays, the plan's and the initial state -> the inputs slab, queued on the stream; then the prior's derived forms.
// The items point into `pl`, `pb`, `st` and h_init_*: all of them stay where they are until the stream has drained.
int BASolver::stage_inputs(const pvio_ba_problem *pb, const pvio_ba_state *st, const UploadPlan &pl, UploadWork &w) {
    View &v = w.v;
    const Dims &dm = v.dm;
    const size_t Ns = dm.N, M = dm.M, F = dm.F, Dp = 15 * (size_t)dm.prior_n;
    StagedUpload stage;
    stage.add(pb->frame_fixed, Ns, &v.frame_fixed);
    stage.add(pl.pose_active, &v.pose_active);
    stage.add(pl.motion_active, &v.motion_active);
    stage.add(pb->cam_extrinsic, Ns * 7, &v.cam_ext);
    stage.add(pb->imu_extrinsic, Ns * 7, &v.imu_ext);
    stage.add(pb->sqrt_inv_cov, Ns * 4, &v.sic);
    stage.add(pb->intrinsics, Ns * 4, &v.intr);
    stage.add(pb->lm_anchor_frame, M, &v.lm_anchor);
    stage.add(pb->lm_obs_ptr, M + 1, &v.lm_ptr);
    stage.add(pb->lm_anchor_z, M * 2, &v.lm_zref);
    stage.add(pl.lm_mult, &v.lm_mult);
    stage.add(pb->obs_frame, F, &v.obs_frame);
    stage.add(pb->obs_z, F * 2, &v.obs_z);
    stage.add(pl.obs_lm, &v.obs_lm);
    stage.add(pl.lm_seen.data(), M, &v.lm_seen);
    stage.add(pl.chunk_lm, &v.chunk_lm);
    stage.add(pl.chunk_tptr, &v.chunk_tptr);
    stage.add(pl.chunk_geo, &v.chunk_geo);
    stage.add(pl.chunk_perm, &v.chunk_perm);
    stage.add(pl.tp_tile_dst, &v.tp_tile_dst);
    stage.add(pl.task_desc, &v.task_desc);
    stage.add(pl.pre_valid, &v.pre_valid);
    stage.add(dm.use_inertial ? pb->preint_delta : nullptr, Ns * 11, &v.pre_delta);
    stage.add(dm.use_inertial ? pb->preint_sqrt_inv_cov : nullptr, Ns * 225, &v.pre_U);
    stage.add(dm.use_inertial ? pb->preint_jacobian : nullptr, Ns * 45, &v.pre_jac);
    stage.add(pb->prior_frames, (size_t)dm.prior_n, &v.prior_frames);
    stage.add(pb->prior_S, Dp * Dp, &v.prior_S);
    stage.add(pb->prior_s, Dp, &v.prior_s);
    stage.add(pb->prior_lin_state, (size_t)dm.prior_n * 16, &v.prior_lin);
    const size_t npo = dm.n_plane ? (size_t)pb->plane_obs_ptr[dm.n_plane] : 0;
    stage.add(pb->plane_obs_ptr, (size_t)dm.n_plane + 1, &v.plane_ptr);
    stage.add(pb->plane_obs_frame, npo, &v.plane_frame);
    stage.add(pl.plane_chunk, &v.plane_chunk);
    stage.add(pb->plane_obs_z, npo * 2, &v.plane_z);
    stage.add(pb->plane_normal, (size_t)dm.n_plane * 3, &v.plane_normal);
    stage.add(pb->plane_distance, (size_t)dm.n_plane, &v.plane_dist);
    v.plane_sic = pb->plane_sqrt_inv_cov;
    stage.add(pl.rot_slot, &v.rot_slot);
    stage.add(pl.prior_slot, &v.prior_slot);
    stage.add(pb->rot_prior_q0, (size_t)dm.n_rot * 4, &v.rot_q0);
    stage.add(pb->rot_prior_sqrt_info, (size_t)dm.n_rot * 9, &v.rot_W);
    // initial state: kept on the host (tiny for frames) and on the device in buffer 0
    h_init_fs_.assign(st->frame_state, st->frame_state + Ns * 16);
    h_init_rho_.assign(st->lm_inv_depth, st->lm_inv_depth + M);
    stage.add(h_init_fs_, &w.fs_init);
    stage.add(h_init_rho_, &w.rho_init);

    // ---- one staging pass, one DMA ----
    // small arrays ride in the staging buffer (front of the slab); a big one (the observation arrays of a 50 000-landmark
    // window) is cheaper sent from where it lies than copied twice, and lives behind them
    constexpr size_t kDirect = 1 << 20;
    size_t staged = 0, total = 0;
    for (auto &it : stage.items)
        if (it.bytes < kDirect) it.off = staged, staged += (std::max<size_t>(it.bytes, 8) + 255) & ~(size_t)255;
    total = staged;
    for (auto &it : stage.items)
        if (it.bytes >= kDirect) it.off = total, total += (it.bytes + 255) & ~(size_t)255;
    char *slab = static_cast<char *>(pool_.get("inputs", total, &w.grew));
    if (!slab) return fail(PVIO_ERR_OUT_OF_MEMORY, "device allocation failed");
    if (stage_in_flight_) {
        // the last upload returned with its staged copy queued and the call that was to synchronize behind it ended early (an error in
        // solve() / marginalize() before their own synchronization): drain the stream before the staging buffer is written again
        if (check(hipStreamSynchronize(stream_), "staging buffer still in flight")) return PVIO_ERR_HIP;
        stage_in_flight_ = false;
    }
    // (pinned host memory is the expensive allocation: headroom for the next windows of the sequence)
    char *h_stage = static_cast<char *>(h_stage_.reserve(staged, staged + staged / 2));
    if (!h_stage && staged) return fail(PVIO_ERR_OUT_OF_MEMORY, "hipHostMalloc failed");
    for (const auto &it : stage.items) {
        if (it.src && it.bytes < kDirect) std::memcpy(h_stage + it.off, it.src, it.bytes);
        *it.dst = slab + it.off;
    }
    if (check(hipMemcpyAsync(slab, h_stage, staged, hipMemcpyHostToDevice, stream_), "H2D inputs")) return PVIO_ERR_HIP;
    for (const auto &it : stage.items)
        if (it.src && it.bytes >= kDirect) {
            if (check(hipMemcpyAsync(slab + it.off, it.src, it.bytes, hipMemcpyHostToDevice, stream_), "H2D inputs")) return PVIO_ERR_HIP;
            w.sent_directly = true;
        }
    if (pl.lm_mult.empty()) v.lm_mult = nullptr; // no duplicates: the kernels take the unscaled path
    if (dm.prior_n > 0 && check(launch_prior_prep(v.prior_S, v.prior_s, (int)Dp, const_cast<double *>(v.prior_Lambda), const_cast<double *>(v.prior_eta),
                                                  const_cast<double *>(v.prior_ST), stream_), "k_prior_prep"))
        return PVIO_ERR_HIP;
    return PVIO_OK;
}

// commit: the new window becomes the context's.  The only step that writes members other than the staging buffers.
int BASolver::commit(const pvio_ba_problem *pb, const UploadWork &w, bool may_return_early) {
    const bool dims_changed = std::memcmp(&w.v.dm, &v_.dm, sizeof(Dims)) != 0;
    if (w.grew || dims_changed || std::memcmp(&w.v, &v_, sizeof(View)) != 0) invalidate_graph();
    v_ = w.v;
    fs_init_ = w.fs_init, rho_init_ = w.rho_init;
    uploaded_ = true;
    solves_since_upload_ = 0;
    trace_cap_ = w.v.dm.max_iter + 2;
    max_solver_time_ = pb->max_solver_time > 0 ? pb->max_solver_time : 0.0;
    // The caller of the public entry point may release its arrays as soon as upload() returns, and arrays that went straight from where they
    // lay (>= 1 MB; some of them the plan's, which upload() destroys) must have left: wait.  A solve that follows immediately on the same stream
    // (pvio_hip_ba_solve: may_return_early) synchronizes anyway before ITS caller gets the arrays back; the staged part was copied into the
    // pinned buffer, which is not written again before the next upload.
    if (may_return_early && !w.sent_directly) {
        stage_in_flight_ = true; // the DMA may still be reading h_stage_: the next upload waits for it before it writes there
        return PVIO_OK;
    }
    stage_in_flight_ = false;
    return check(hipStreamSynchronize(stream_), "upload sync");
}

int BASolver::upload(const pvio_ba_problem *pb, const pvio_ba_state *st, bool may_return_early) {
    UploadPlan plan; // outlives commit's wait for the arrays that are sent from where they lie
    const Reject bad = validate_upload(pb, st, plan.lm_seen);
    if (bad.code != PVIO_OK) return fail(bad.code, bad.msg); // the previous window stays as it was
    if (check(hipSetDevice(device_), "hipSetDevice")) return PVIO_ERR_HIP;
    if (cus_ <= 0) { // asked once: the query is slow
        hipDeviceProp_t prop;
        if (check(hipGetDeviceProperties(&prop, device_), "hipGetDeviceProperties")) return PVIO_ERR_HIP;
        cus_ = std::max(1, prop.multiProcessorCount);
    }
    plan_upload(pb, plan);
    UploadWork work;
    work.v.dm = plan.dm;
    int rc = allocate(work);
    if (rc == PVIO_OK) rc = stage_inputs(pb, st, plan, work);
    if (rc != PVIO_OK) {
        // Between windows: a pool slot that grew has freed what v_ and the captured graph point to, and the slab is half written.  Neither may be
        // used again (solve() / download() answer "no problem uploaded"), and nothing may still be reading the plan's or the caller's arrays.
        uploaded_ = false;
        invalidate_graph();
        (void)hipStreamSynchronize(stream_);
        stage_in_flight_ = false;
        return rc;
    }
    return commit(pb, work, may_return_early);
}

// ---------------------------------------------------------------------------------------------------------------------
// Read-back layouts, each written once (in doubles): the device request, the pinned reservation, the kernel arguments
// and the host-side pointers all come from them.
// ---------------------------------------------------------------------------------------------------------------------

// a solve's packed results (k_quality `pack`): frame states | inverse depths | quality | valid bytes, in one pinned buffer
struct SolvePack {
    size_t M, o_rho, o_quality, o_valid, n;
    explicit SolvePack(const Dims &dm) : M((size_t)dm.M), o_rho((size_t)dm.N * 16), o_quality(o_rho + M), o_valid(o_rho + 2 * M), n(o_valid + (M + 7) / 8) {}
};

// the eight arrays a marginalization reads back, gathered on the device (k_gather) into one block: segment k starts at off[k], a multiple of 8
struct MargGather {
    size_t n[8], off[9];
    explicit MargGather(const Dims &dm) {
        const size_t Ns = dm.N, Dp = 15 * (size_t)dm.prior_n, nS = (size_t)dm.n_tasks * 9, nV = (size_t)kNumPoseVec * dm.P6;
        const size_t sizes[8] = {nS + nV + kNumLinScal, Ns * 900, Ns * 30, Dp * Dp, Dp, Ns * 9, Ns * 3, ((size_t)dm.n_tasks + 1) / 2};
        off[0] = 0;
        for (int k = 0; k < 8; ++k) n[k] = sizes[k], off[k + 1] = off[k] + ((n[k] + 7) & ~(size_t)7);
    }
    size_t total() const { return off[8]; }
    GatherArgs args(const View &v) const {
        const void *src[8] = {v.red, v.pre_H, v.pre_g, v.prior_H, v.prior_g, v.rot_H, v.rot_g, v.task_desc};
        GatherArgs ga;
        for (int k = 0; k < 8; ++k) {
            ga.src[k] = src[k];
            ga.words[k] = (uint32_t)(k == 7 ? (size_t)v.dm.n_tasks : 2 * n[k]);
            ga.off[k] = (uint32_t)(2 * off[k]);
        }
        return ga;
    }
    MargSegments host(const double *h) const {
        return {h + off[0], h + off[1], h + off[2], h + off[3], h + off[4], h + off[5], h + off[6], reinterpret_cast<const int32_t *>(h + off[7])};
    }
};

// a covariance call's two slabs.  results: header | coord_free | frame_cov | lm_var | joint_cov (last: copied back only when the caller wants it);
// work: S | scale | tiles | sig6 | row_nz, free_coord (int32)
struct CovSlabs {
    size_t N, D, max_coords, o_free, o_frame, o_lm, o_joint, n_res, w_scale, w_tiles, w_sig6, w_int, n_work;
    CovSlabs(size_t N_, size_t M, size_t max_coords_)
        : N(N_), D(15 * N_), max_coords(max_coords_), o_free(2), o_frame(o_free + (D + 7) / 8), o_lm(o_frame + N * 225), o_joint(o_lm + ((M + 7) & ~(size_t)7)),
          n_res(o_joint + D * D), w_scale(D * D), w_tiles(w_scale + D), w_sig6(w_tiles + cov_tile_doubles(max_coords)), w_int(w_sig6 + 36 * N * N), n_work(w_int + D) {}
    CovArgs args(double *d_res, double *d_work) const {
        CovArgs a{};
        a.D = (int32_t)D, a.max_coords = (int32_t)max_coords;
        a.Sfull = d_work, a.scale = d_work + w_scale, a.tiles = d_work + w_tiles, a.sig6 = d_work + w_sig6;
        a.row_nz = reinterpret_cast<int32_t *>(d_work + w_int), a.free_coord = a.row_nz + D;
        a.hdr = reinterpret_cast<CovHdr *>(d_res), a.coord_free = reinterpret_cast<uint8_t *>(d_res + o_free);
        a.frame_cov = d_res + o_frame, a.lm_var = d_res + o_lm, a.joint_cov = d_res + o_joint;
        return a;
    }
};

// ---------------------------------------------------------------------------------------------------------------------
// solve = request buffers -> reset -> [profiling scope] replay the slots until the device reports done (the ranks agreeing
// on a time limit) -> summary -> unpack.  run_slots replays or captures the graph of enqueue_slot's launch sequence.
// ---------------------------------------------------------------------------------------------------------------------

// diagnostics (PVIO_HIP_DEBUG_CTRL=1, plain launches only): the control block as each kernel of the slot leaves it
void BASolver::dump_ctrl(const char *after) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(stream_, &cs);
    if (!solver_switches().debug_ctrl || cs != hipStreamCaptureStatusNone) return;
    Ctrl h;
    (void)hipStreamSynchronize(stream_);
    (void)hipMemcpy(&h, v_.ctrl, sizeof h, hipMemcpyDeviceToHost);
    std::fprintf(stderr, "[ctrl after %-11s] mode %d lin_result %d cur %d lin %d iter %d succ %d invalid %d term %d done %d reuse %d solve_ok %d scaling %d trace %d retry %d | radius %.6e mu %.3e x_cost %.9e "
                         "xn2 %.6e %.6e gmax %.3e | g2 %.6e gn2 %.6e gdot %.6e qvv %.6e qvy %.6e qyy %.6e gy %.6e lm_g2 %.6e | ca %.6e cb %.6e sn %.6e mcc %.6e | it %.6e %.3e %.3e %.3e v%d s%d | fin %d %d %.3e\n",
                 after, h.mode, h.lin_result, h.cur, h.lin, h.iter, h.num_success, h.invalid_steps, h.termination, h.done, h.reuse, h.solve_ok, h.scaling_ready, h.trace_len, h.retry_relin, h.radius, h.mu, h.x_cost,
                 h.x_norm2_pose, h.x_norm2_lm, h.grad_max, h.pose_g2, h.pose_gn2, h.pose_gdot, h.pose_qvv, h.pose_qvy, h.pose_qyy, h.pose_gy, h.lm_g2, h.ca, h.cb, h.dogleg_step_norm, h.model_cost_change,
                 h.it_cost, h.it_cost_change, h.it_step_norm, h.it_rel, h.it_valid, h.it_success, h.fin_flags, h.fin_trace_slot, h.fin_lm_gmax);
}

int BASolver::enqueue_slot(hipEvent_t *ev) {
    hipError_t e;
    View vl = v_;
    if (sharded_) vl.back_part = v_.back_red; // k_linearize reads the all-reduced row
    if (ev) (void)hipEventRecord(ev[0], stream_);
    if ((e = launch_linearize(vl, stream_)) != hipSuccess) return check(e, "k_linearize");
    if (ev) (void)hipEventRecord(ev[1], stream_);
    if ((e = launch_reduce(v_, stream_, sharded_ ? 1 : 0)) != hipSuccess) return check(e, "k_reduce");
    if (ev) (void)hipEventRecord(ev[2], stream_);
    if (sharded_) {
        const size_t n = (size_t)v_.dm.n_tasks * 9 + (size_t)kNumPoseVec * v_.dm.P6 + kNumLinScal;
        // ONE summing all-reduce per linearization: scalar 4 (max |b_l|) travels as one slot per rank behind the scalars
        // (k_reduce fills this rank's slot, zeros the others; k_dense takes the maximum), its summed copy is not used
        if (comm_allreduce(comm_, v_.red, n + (size_t)world_, 0, stream_)) return fail(PVIO_ERR_COMM, "all-reduce failed");
        // the all-reduced system -> tile image (every rank the same): the dense kernel then runs as on one GPU
        if ((e = launch_reduce(v_, stream_, 2)) != hipSuccess) return check(e, "k_reduce (image)");
    }
    if (ev) (void)hipEventRecord(ev[3], stream_);
    dump_ctrl("k_reduce");
    if ((e = launch_dense(v_, stream_)) != hipSuccess) return check(e, "k_dense");
    dump_ctrl("k_dense");
    if (ev) (void)hipEventRecord(ev[4], stream_);
    if (!v_.dm.fuse_backsub && (e = launch_backsub(v_, stream_)) != hipSuccess) return check(e, "k_backsub");
    dump_ctrl("k_backsub");
    if (ev) (void)hipEventRecord(ev[5], stream_);
    if (sharded_) {
        double *back_local = static_cast<double *>(pool_.get("back_local", kNumBackScal * sizeof(double)));
        if ((e = launch_back_reduce(v_, back_local, stream_)) != hipSuccess) return check(e, "k_back_reduce");
        if (comm_allreduce(comm_, v_.back_red, kNumBackScal, 0, stream_)) return fail(PVIO_ERR_COMM, "all-reduce failed");
    }
    if (ev) (void)hipEventRecord(ev[6], stream_);
    return PVIO_OK;
}

int BASolver::run_slots(int n_slots) {
    // A window that has just been uploaded with a new shape is solved with plain launches (they pipeline on the stream: the
    // state machine is on the device); capturing + instantiating a graph costs more than it saves on a single solve and
    // is left to the second solve of the same resident window.
    const bool have_graph = graph_exec_ && graph_slots_ == n_slots;
    // Landmark-sharded runs are captured too (RCCL supports stream capture; eager launches + two collectives per iteration cost
    // 9 257 against 9 779 iterations/s with one rank).  Only ever exercised with a one-rank communicator on this pool, hence the
    // safety net: if capturing or instantiating the sharded graph fails, this context falls back to eager launches for good.
    // PVIO_HIP_SHARDED_GRAPH=0 turns the capture off.
    if (use_graph_ && (!sharded_ || (solver_switches().sharded_graph && !sharded_graph_failed_)) && (have_graph || solves_since_upload_ > 0)) {
        bool ok = true;
        if (!have_graph) {
            invalidate_graph();
            if (check(hipStreamBeginCapture(stream_, hipStreamCaptureModeThreadLocal), "begin capture")) {
                if (!sharded_) return PVIO_ERR_HIP;
                ok = false;
            }
            if (ok) {
                int rc = PVIO_OK;
                for (int s = 0; s < n_slots && rc == PVIO_OK; ++s) rc = enqueue_slot();
                hipError_t e = hipStreamEndCapture(stream_, &graph_);
                if (rc != PVIO_OK || e != hipSuccess || hipGraphInstantiate(&graph_exec_, graph_, nullptr, nullptr, 0) != hipSuccess) {
                    if (!sharded_) return rc != PVIO_OK ? rc : fail(PVIO_ERR_HIP, "graph capture / instantiate failed");
                    ok = false;
                } else {
                    graph_slots_ = n_slots;
                }
            }
            if (!ok) { // sharded only: remember, clean up, run this and every later solve eagerly
                (void)hipGetLastError();
                invalidate_graph();
                sharded_graph_failed_ = true;
            }
        }
        if (ok) {
            ++graph_replays_;
            return check(hipGraphLaunch(graph_exec_, stream_), "graph launch");
        }
    }
    for (int s = 0; s < n_slots; ++s) {
        int rc = enqueue_slot();
        if (rc != PVIO_OK) return rc;
    }
    return PVIO_OK;
}

// the buffers a solve asks for by itself: the packed read-back (device + pinned) and the trace states
int BASolver::request_solve_buffers(const SolvePack &pack, bool read_back, bool want_states, double **d_pack) {
    if (read_back) {
        bool grew = false;
        if (!dev(pool_, "result_pack", pack.n, d_pack, &grew)) return fail(PVIO_ERR_OUT_OF_MEMORY, "result_pack");
        if (!h_pack_.reserve(pack.n * sizeof(double), (pack.n + pack.n / 2) * sizeof(double))) return fail(PVIO_ERR_OUT_OF_MEMORY, "hipHostMalloc failed");
    }
    // trace states are optional and live in a separate buffer so that bench runs do not pay for them
    double *ts = nullptr;
    if (want_states) {
        bool grew = false;
        if (!dev(pool_, "trace_states", (size_t)trace_cap_ * ((size_t)v_.dm.N * 16 + v_.dm.M), &ts, &grew)) return fail(PVIO_ERR_OUT_OF_MEMORY, "trace_states");
    }
    if (ts != v_.trace_states) {
        v_.trace_states = ts;
        invalidate_graph();
    }
    return PVIO_OK;
}

// reset: state buffer 0 <- initial state, user state, control block
// (one launch: k_reset; the control block's template lives on the device and is sent again only when it changes)
int BASolver::reset_for_solve() {
    Ctrl t;
    std::memset(&t, 0, sizeof t);
    t.mode = MODE_INIT;
    t.radius = 1e4;        // initial_trust_region_radius
    t.mu = 1e-8;           // DoglegStrategy kMinMu
    t.termination = PVIO_TERM_NO_CONVERGENCE;
    t.trace_cap = trace_cap_;
    t.dbg_fail_left = dbg_fail_, t.dbg_invalid_left = dbg_invalid_;
    bool grew = false;
    Ctrl *d_tmpl = nullptr;
    if (!dev(pool_, "ctrl_template", 1, &d_tmpl, &grew)) return fail(PVIO_ERR_OUT_OF_MEMORY, "ctrl template");
    if (grew || d_tmpl != d_ctrl_tmpl_ || std::memcmp(&t, &h_ctrl_tmpl_, sizeof t) != 0) {
        h_ctrl_tmpl_ = t, d_ctrl_tmpl_ = d_tmpl;
        // (pageable source: the copy is staged by the runtime before the call returns)
        if (check(hipMemcpyAsync(d_tmpl, &h_ctrl_tmpl_, sizeof t, hipMemcpyHostToDevice, stream_), "ctrl template")) return PVIO_ERR_HIP;
    }
    return check(launch_reset(v_, fs_init_, rho_init_, d_tmpl, stream_), "k_reset");
}

// solve(prof != nullptr): seven events around a slot's launches, the stamp buffer in v_.dbg / v_.dbg_sel and, with PVIO_HIP_PROFILE_GRAPH, a slot graph that
// carries it.  The destructor undoes all of it on every way out of solve().  Without `prof` the scope does nothing.
class BASolver::ProfileScope {
  public:
    ProfileScope(BASolver &s, pvio_ba_kernel_times *prof) : s_(s), prof_(prof), dbg_saved_(s.v_.dbg), sel_saved_(s.v_.dbg_sel) {}
    ProfileScope(const ProfileScope &) = delete;
    ~ProfileScope() {
        if (!prof_) return;
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
        s_.v_.dbg = dbg_saved_, s_.v_.dbg_sel = sel_saved_;
        if (graph) s_.invalidate_graph(); // the next solve captures a graph without the stamp buffer again
    }
    int begin() {
        if (!prof_) return PVIO_OK;
        std::memset(prof_, 0, sizeof *prof_);
        for (auto &e : ev) (void)hipEventCreate(&e);
        bool grew = false;
        long long *dbg = nullptr;
        if (!dev(s_.pool_, "dbg", 4 * 32, &dbg, &grew)) return s_.fail(PVIO_ERR_OUT_OF_MEMORY, "dbg");
        (void)hipMemsetAsync(dbg, 0, 4 * 32 * sizeof(long long), s_.stream_);
        // PVIO_HIP_STAMP_SEL: -1 (default) every stamp site stores, k >= 0 only site k (one store per launch), -2 none (events only)
        const char *sel = std::getenv("PVIO_HIP_STAMP_SEL");
        s_.v_.dbg_sel = sel ? std::atoi(sel) : -1;
        s_.v_.dbg = s_.v_.dbg_sel == -2 ? nullptr : dbg;
        // PVIO_HIP_PROFILE_GRAPH=1: the stamps are taken inside a REPLAY of the slot graph (kernels back to back, as in a normal
        // solve) instead of eager launches with a host synchronization per slot; no per-launch events then
        graph = std::getenv("PVIO_HIP_PROFILE_GRAPH") != nullptr && std::atoi(std::getenv("PVIO_HIP_PROFILE_GRAPH")) != 0;
        if (graph) s_.invalidate_graph(); // the graph bakes the View in: capture one that carries the stamp buffer
        return PVIO_OK;
    }
    bool eager() const { return prof_ && !graph; } // one slot at a time, events around every launch
    void read_stamps() {
        if (prof_ && s_.v_.dbg) (void)hipMemcpy(prof_->phase_ticks, s_.v_.dbg, 4 * 32 * sizeof(long long), hipMemcpyDeviceToHost);
    }
    hipEvent_t ev[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    bool graph = false;

  private:
    BASolver &s_;
    pvio_ba_kernel_times *prof_;
    long long *dbg_saved_;
    int sel_saved_;
};

// one profiled eager slot: events around every launch; counts only slots that did work
int BASolver::profiled_slot(hipEvent_t *pev, pvio_ba_kernel_times *prof) {
    int rc = enqueue_slot(pev);
    if (rc == PVIO_OK && check(hipStreamSynchronize(stream_), "profile sync")) rc = PVIO_ERR_HIP;
    if (rc != PVIO_OK) return rc;
    const int ia[4] = {0, 1, 3, 4}, ib[4] = {1, 2, 4, 5};
    for (int k = 0; k < 4; ++k) {
        float ms1 = 0;
        (void)hipEventElapsedTime(&ms1, pev[ia[k]], pev[ib[k]]);
        prof->total_ms[k] += ms1;
        prof->launches[k] += 1;
    }
    if (sharded_) { // the two exchange steps: between k_reduce and k_dense, behind k_backsub
        const int ca[2] = {2, 5}, cb[2] = {3, 6};
        for (int k = 0; k < 2; ++k) {
            float ms1 = 0;
            (void)hipEventElapsedTime(&ms1, pev[ca[k]], pev[cb[k]]);
            prof->comm_ms[k] += ms1;
            prof->comm_launches[k] += 1;
        }
    }
    return PVIO_OK;
}

// max_solver_time_in_seconds (solver_options.h:30): the state machine runs on the device, so the wall clock is looked at
// between replays of the slot graph only (one replay covers every iteration of an ordinary solve): NO_CONVERGENCE at
// the iterate reached, like Ceres' time-limit exit.  `timed_out`: what every rank agreed on.
int BASolver::time_limit_reached(Clock::time_point t0, bool *timed_out) {
    int out = std::chrono::duration<double>(Clock::now() - t0).count() > max_solver_time_ ? 1 : 0;
    const int dbg_timeout_rank = solver_switches().timeout_rank;
    if (dbg_timeout_rank >= 0) out = rank_ == dbg_timeout_rank ? 1 : 0;
    if (sharded_) {
        // every rank looks at its OWN clock, but the next replay contains collectives: a rank that left alone would leave the
        // others waiting in an all-reduce for good.  `done` is identical on all ranks (identical all-reduced inputs),
        // so they all arrive here in the same round; the decision is all-reduced (max) before anybody acts on it.
        double *flag = static_cast<double *>(pool_.get("timeout_flag", sizeof(double)));
        double hflag = out;
        if (!flag || check(hipMemcpyAsync(flag, &hflag, sizeof(double), hipMemcpyHostToDevice, stream_), "timeout flag H2D")) return PVIO_ERR_HIP;
        if (comm_allreduce(comm_, flag, 1, 1, stream_)) return fail(PVIO_ERR_COMM, "all-reduce failed");
        if (check(hipMemcpyAsync(&hflag, flag, sizeof(double), hipMemcpyDeviceToHost, stream_), "timeout flag D2H")) return PVIO_ERR_HIP;
        if (check(hipStreamSynchronize(stream_), "timeout flag sync")) return PVIO_ERR_HIP;
        out = hflag > 0.0;
    }
    *timed_out = out != 0;
    return PVIO_OK;
}

int BASolver::fill_summary(pvio_ba_summary *sum, bool want_states, Clock::time_point t0) {
    float ms = 0;
    (void)hipEventElapsedTime(&ms, ev0_, ev1_);
    sum->termination = h_ctrl_->termination;
    sum->is_usable = h_ctrl_->termination != PVIO_TERM_FAILURE;
    sum->num_iterations = h_ctrl_->iter;
    sum->num_successful_steps = h_ctrl_->num_success;
    sum->initial_cost = h_ctrl_->initial_cost;
    sum->final_cost = h_ctrl_->x_cost;
    sum->device_seconds = ms * 1e-3;
    sum->trace_len = 0;
    if (sum->trace && sum->trace_capacity > 0) {
        const int n = std::min(std::min(h_ctrl_->trace_len, trace_cap_), sum->trace_capacity);
        std::vector<TraceRec> tr(n);
        if (n && check(hipMemcpy(tr.data(), v_.trace, n * sizeof(TraceRec), hipMemcpyDeviceToHost), "trace D2H")) return PVIO_ERR_HIP;
        static_assert(sizeof(TraceRec) == sizeof(pvio_ba_iteration), "trace layout");
        std::memcpy(sum->trace, tr.data(), n * sizeof(TraceRec));
        sum->trace_len = n;
        if (want_states && n)
            if (check(hipMemcpy(sum->trace_states, v_.trace_states, (size_t)n * ((size_t)v_.dm.N * 16 + v_.dm.M) * sizeof(double), hipMemcpyDeviceToHost), "trace states D2H")) return PVIO_ERR_HIP;
    }
    sum->solve_seconds = std::chrono::duration<double>(Clock::now() - t0).count();
    return PVIO_OK;
}

// what the quality pass found, for unpack_results and download(): invalidated landmarks keep their old quality (bundle_adjustor.cpp:294)
static void copy_quality(pvio_ba_state *st, const double *q, const unsigned char *val, size_t M) {
    for (size_t l = 0; l < M; ++l) {
        if (st->lm_valid) st->lm_valid[l] = val[l];
        if (st->lm_quality && val[l]) st->lm_quality[l] = q[l];
    }
}

void BASolver::unpack_results(const SolvePack &pack, pvio_ba_state *read_back) const { // same semantics as download()
    const double *h_pack = h_pack_.as<double>();
    if (read_back->frame_state) std::memcpy(read_back->frame_state, h_pack, pack.o_rho * sizeof(double));
    if (pack.M && read_back->lm_inv_depth) std::memcpy(read_back->lm_inv_depth, h_pack + pack.o_rho, pack.M * sizeof(double));
    copy_quality(read_back, h_pack + pack.o_quality, reinterpret_cast<const unsigned char *>(h_pack + pack.o_valid), pack.M);
}

int BASolver::solve(pvio_ba_summary *sum, pvio_ba_kernel_times *prof, pvio_ba_state *read_back) {
    if (!uploaded_) return fail(PVIO_ERR_INVALID_ARGUMENT, "no problem uploaded");
    const auto t0 = Clock::now();
    if (check(hipSetDevice(device_), "hipSetDevice")) return PVIO_ERR_HIP;
    const Dims &dm = v_.dm;
    const SolvePack pack(dm);
    const bool want_states = sum && sum->trace_states && sum->trace_capacity > 0;
    double *d_pack = nullptr;
    int rc = request_solve_buffers(pack, read_back != nullptr, want_states, &d_pack);
    if (rc == PVIO_OK) rc = reset_for_solve();
    if (rc != PVIO_OK) return rc;
    if (check(hipEventRecord(ev0_, stream_), "event")) return PVIO_ERR_HIP;
    // every slot = one pass of [linearize, reduce, dense, backsub]; iteration 0 + max_iter iterations; relaunch while the device
    // has not reported done
    // (no slack slot: a solve whose mu escalates needs more slots than iterations and simply gets a second replay from the loop below;
    // every other solve saved four no-op launches per replay)
    // A real-time configuration (a limit far below the reference's default of 1e6 s, config.cpp:86-88) looks at the clock every two
    // slots instead of once per solve: Ceres tests its limit every iteration
    const bool time_limited = max_solver_time_ > 0 && max_solver_time_ < 1.0e5;
    const int n_slots = time_limited ? std::min(dm.max_iter + 1, 2) : dm.max_iter + 1;
    {
        ProfileScope profile(*this, prof);
        if ((rc = profile.begin()) != PVIO_OK) return rc;
        for (int rounds = 0;;) {
            rc = profile.eager() ? profiled_slot(profile.ev, prof) : run_slots(n_slots);
            if (profile.eager()) --rounds; // the round cap below is for graph replays
            if (rc != PVIO_OK) return rc;
            const auto t_enq = Clock::now();
            if (check(hipMemcpyAsync(h_ctrl_, v_.ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost, stream_), "ctrl D2H")) return PVIO_ERR_HIP;
            if (check(hipEventRecord(ev1_, stream_), "event")) return PVIO_ERR_HIP;
            if (read_back) { // speculative: all but never is the state machine still running after one replay (then this is repeated)
                if (check(launch_quality(v_, stream_, 1, nullptr, d_pack), "k_quality")) return PVIO_ERR_HIP;
                if (check(hipMemcpyAsync(h_pack_.data(), d_pack, pack.n * sizeof(double), hipMemcpyDeviceToHost, stream_), "results D2H")) return PVIO_ERR_HIP;
            }
            if (check(hipStreamSynchronize(stream_), "solve sync")) return PVIO_ERR_HIP;
            stage_in_flight_ = false;
            if (solver_switches().timing) // PVIO_HIP_TIMING=1: where the host's time of a solve goes (enqueueing the slots against waiting for them)
                std::fprintf(stderr, "[pvio-hip] solve host: reset + %d slots enqueued after %.0f us (%s), stream drained after %.0f us\n", n_slots, us(t0, t_enq),
                             graph_exec_ && graph_slots_ == n_slots ? "graph" : "plain launches", us(t0, Clock::now()));
            if (h_ctrl_->done || ++rounds > (time_limited ? 16 * (dm.max_iter + 1) : 16)) break;
            bool timed_out = false;
            if (max_solver_time_ > 0 && (rc = time_limit_reached(t0, &timed_out)) != PVIO_OK) return rc;
            if (timed_out) {
                h_ctrl_->done = 1, h_ctrl_->termination = PVIO_TERM_NO_CONVERGENCE;
                break;
            }
        }
        profile.read_stamps();
    }
    ++solves_since_upload_;
    if (!h_ctrl_->done) return fail(PVIO_ERR_HIP, "device state machine did not terminate");
    last_repeats_ = h_ctrl_->cand_repeats;
    if (sum && (rc = fill_summary(sum, want_states, t0)) != PVIO_OK) return rc;
    if (read_back) unpack_results(pack, read_back);
    return PVIO_OK;
}

int BASolver::download(pvio_ba_state *st) {
    if (!uploaded_ || !st) return fail(PVIO_ERR_INVALID_ARGUMENT, "nothing to download");
    const Dims &dm = v_.dm;
    const int cur = h_ctrl_->cur;
    if (check(launch_quality(v_, stream_, 1, nullptr), "k_quality")) return PVIO_ERR_HIP;
    if (check(hipMemcpyAsync(st->frame_state, v_.fs + (size_t)cur * dm.N * 16, (size_t)dm.N * 16 * sizeof(double), hipMemcpyDeviceToHost, stream_), "D2H")) return PVIO_ERR_HIP;
    if (dm.M) {
        if (check(hipMemcpyAsync(st->lm_inv_depth, v_.rho + (size_t)cur * dm.M, (size_t)dm.M * sizeof(double), hipMemcpyDeviceToHost, stream_), "D2H")) return PVIO_ERR_HIP;
        std::vector<double> q;
        std::vector<uint8_t> val;
        if (st->lm_quality || st->lm_valid) {
            q.resize(dm.M), val.resize(dm.M);
            if (check(hipMemcpyAsync(q.data(), v_.lm_quality, (size_t)dm.M * sizeof(double), hipMemcpyDeviceToHost, stream_), "D2H")) return PVIO_ERR_HIP;
            if (check(hipMemcpyAsync(val.data(), v_.lm_valid, (size_t)dm.M, hipMemcpyDeviceToHost, stream_), "D2H")) return PVIO_ERR_HIP;
            if (check(hipStreamSynchronize(stream_), "sync")) return PVIO_ERR_HIP;
            copy_quality(st, q.data(), val.data(), (size_t)dm.M);
        }
    }
    return check(hipStreamSynchronize(stream_), "download sync");
}

int BASolver::reprojection_error(double *out) {
    if (!uploaded_ || !out) return fail(PVIO_ERR_INVALID_ARGUMENT, "nothing uploaded");
    double *acc = static_cast<double *>(pool_.get("err_acc", 2 * sizeof(double)));
    if (!acc) return fail(PVIO_ERR_OUT_OF_MEMORY, "err_acc");
    if (check(hipMemsetAsync(acc, 0, 2 * sizeof(double), stream_), "memset")) return PVIO_ERR_HIP;
    // evaluates the uploaded initial state (buffer 0 after a reset)
    const size_t Ns = v_.dm.N, Ms = std::max(v_.dm.M, 1);
    const double *fs_init = fs_init_, *rho_init = rho_init_;
    if (check(hipMemcpyAsync(v_.fs, fs_init, Ns * 16 * sizeof(double), hipMemcpyDeviceToDevice, stream_), "reset fs")) return PVIO_ERR_HIP;
    if (v_.dm.M && check(hipMemcpyAsync(v_.rho, rho_init, (size_t)v_.dm.M * sizeof(double), hipMemcpyDeviceToDevice, stream_), "reset rho")) return PVIO_ERR_HIP;
    if (check(launch_quality(v_, stream_, 0, acc), "k_quality")) return PVIO_ERR_HIP;
    double h[2];
    if (check(hipMemcpyAsync(h, acc, sizeof h, hipMemcpyDeviceToHost, stream_), "D2H")) return PVIO_ERR_HIP;
    if (check(hipStreamSynchronize(stream_), "sync")) return PVIO_ERR_HIP;
    *out = h[0] / std::max(h[1], 1.0);
    return PVIO_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// The one-shot calls: marginalize and covariance = upload -> linearize_once -> their own kernels and read-back.  Both use
// the uploaded window up: from their upload on the context is between windows, whichever way they return.
// ---------------------------------------------------------------------------------------------------------------------

// One undamped linearization of the window just uploaded, at the uploaded state: k_reset, the control block, k_linearize, k_reduce.
int BASolver::linearize_once(int mode, int victim) {
    // working states <- the uploaded ones, in one launch (the control block it also copies is its own content: overwritten right below)
    if (check(launch_reset(v_, fs_init_, rho_init_, v_.ctrl, stream_), "k_reset")) return PVIO_ERR_HIP;
    std::memset(h_ctrl_, 0, sizeof(Ctrl));
    h_ctrl_->mode = mode;
    h_ctrl_->marg_victim = victim;
    h_ctrl_->mu = 0.0; // no damping: the Schur weight of a landmark is 1 / H_ll
    if (check(hipMemcpyAsync(v_.ctrl, h_ctrl_, sizeof(Ctrl), hipMemcpyHostToDevice, stream_), "ctrl")) return PVIO_ERR_HIP;
    hipError_t e;
    if ((e = launch_linearize(v_, stream_)) != hipSuccess) return check(e, "k_linearize");
    if ((e = launch_reduce(v_, stream_, sharded_ ? 1 : 0)) != hipSuccess) return check(e, "k_reduce");
    return PVIO_OK;
}

// The landmarks of the window that the victim observes (anchor or target), in their order, with their CSR rows, multiplicities and inverse depths.
// false (nothing written) when the landmark arrays are not a window upload() accepts: the caller then passes the whole window on, to be rejected.
static bool marg_subset(const pvio_ba_problem *pb, const pvio_ba_state *st, int victim, std::vector<int32_t> &anchor, std::vector<double> &anchor_z,
                        std::vector<int32_t> &ptr, std::vector<int32_t> &frame, std::vector<double> &z, std::vector<int32_t> &mult, std::vector<double> &rho) {
    const int M = pb->n_landmarks;
    std::vector<uint32_t> keep; // check_landmarks: the frames that observe the landmark; from here on: whether the victim is one of them (or its anchor)
    if (check_landmarks(pb, st, keep).code != PVIO_OK || M == 0) return false;
    size_t n_keep = 0, f_keep = 0;
    for (int l = 0; l < M; ++l) {
        keep[(size_t)l] = pb->lm_anchor_frame[l] == victim || ((keep[(size_t)l] >> victim) & 1u);
        if (keep[(size_t)l]) ++n_keep, f_keep += (size_t)(pb->lm_obs_ptr[l + 1] - pb->lm_obs_ptr[l]);
    }
    anchor.clear(), anchor_z.clear(), frame.clear(), z.clear(), mult.clear(), rho.clear();
    // (+ 1: a victim without landmarks still hands upload() arrays, not null pointers)
    anchor.reserve(n_keep + 1), anchor_z.reserve(2 * n_keep + 2), rho.reserve(n_keep + 1), frame.reserve(f_keep + 1), z.reserve(2 * f_keep + 2), mult.reserve(n_keep + 1);
    ptr.assign(1, 0);
    for (int l = 0; l < M; ++l) {
        if (!keep[(size_t)l]) continue;
        const int b = pb->lm_obs_ptr[l], e = pb->lm_obs_ptr[l + 1];
        anchor.push_back(pb->lm_anchor_frame[l]);
        anchor_z.push_back(pb->lm_anchor_z[2 * (size_t)l]), anchor_z.push_back(pb->lm_anchor_z[2 * (size_t)l + 1]);
        rho.push_back(st->lm_inv_depth[l]);
        if (pb->lm_multiplicity) mult.push_back(pb->lm_multiplicity[l]);
        for (int o = b; o < e; ++o) frame.push_back(pb->obs_frame[o]), z.push_back(pb->obs_z[2 * (size_t)o]), z.push_back(pb->obs_z[2 * (size_t)o + 1]);
        ptr.push_back((int32_t)frame.size());
    }
    return true;
}

// read-back as ONE copy into a pinned buffer: a D2H copy into pageable memory is staged synchronously by the runtime (about 20 us
// each, eight of them); the eight arrays are gathered on the device first (k_gather).  Synchronizes.
int BASolver::read_back_marg(const MargGather &lay, const double **h_out) {
    double *const h_back = static_cast<double *>(h_back_.reserve(lay.total() * sizeof(double), (lay.total() + lay.total() / 2) * sizeof(double)));
    if (!h_back) return fail(PVIO_ERR_OUT_OF_MEMORY, "hipHostMalloc failed");
    double *d_back = nullptr;
    bool grew = false;
    if (!dev(pool_, "marg_back", lay.total(), &d_back, &grew)) return fail(PVIO_ERR_OUT_OF_MEMORY, "marg_back");
    if (check(launch_gather(lay.args(v_), d_back, stream_), "k_gather")) return PVIO_ERR_HIP;
    if (check(hipMemcpyAsync(h_back, d_back, lay.total() * sizeof(double), hipMemcpyDeviceToHost, stream_), "D2H")) return PVIO_ERR_HIP;
    if (check(hipStreamSynchronize(stream_), "marginalize sync")) return PVIO_ERR_HIP;
    stage_in_flight_ = false;
    *h_out = h_back;
    return PVIO_OK;
}

// BundleAdjustor::marginalize_frame (bundle_adjustor.cpp:348-599).  The O(F) part -- un-robustified J^T J / J^T r of
// every reprojection factor of the victim's landmarks, the scalar landmark elimination, the prior and the two IMU
// factors -- runs on the GPU through k_linearize (MODE_MARG) + k_reduce; the 15N-dimensional dense tail (victim block
// elimination, eigen-decomposition: marg_prior.h) is a few hundred kflop and stays on the host.
int BASolver::marginalize(const pvio_ba_problem *pb, const pvio_ba_state *st, int victim, pvio_ba_prior *out) {
    if (!pb || !st || !out || !out->S || !out->s) return fail(PVIO_ERR_INVALID_ARGUMENT, "null argument");
    const int N = pb->n_frames, R = 15 * (N - 1);
    if (victim < 0 || victim >= N || N < 2) return fail(PVIO_ERR_INVALID_ARGUMENT, "victim frame out of range");
    const auto tm0 = Clock::now();
    // marginalization always works on the full 15-dim error state and ignores FF_FIX_POSE; IMU factors are used
    // whenever they exist (:416-450), regardless of how the last solve was configured
    pvio_ba_problem p2 = *pb;
    p2.use_inertial = 1;
    // :453-461: the problem is built from the tracks the victim observes (as their anchor or as a target) and from nothing else -- the other tracks
    // are never evaluated, so whatever they hold (a zero or non-finite inverse depth, a point behind a camera) cannot reach the prior.  The kernels get
    // those landmarks only.  (A window that upload() would reject is passed on whole, so that it is rejected for the same reason.)
    pvio_ba_state st2 = *st;
    std::vector<int32_t> k_anchor, k_ptr, k_frame, k_mult;
    std::vector<double> k_anchor_z, k_z, k_rho;
    if (marg_subset(pb, st, victim, k_anchor, k_anchor_z, k_ptr, k_frame, k_z, k_mult, k_rho)) {
        p2.n_landmarks = (int32_t)k_anchor.size(), p2.n_obs = (int32_t)k_frame.size();
        p2.lm_anchor_frame = k_anchor.data(), p2.lm_anchor_z = k_anchor_z.data(), p2.lm_obs_ptr = k_ptr.data();
        p2.obs_frame = k_frame.data(), p2.obs_z = k_z.data();
        p2.lm_multiplicity = pb->lm_multiplicity ? k_mult.data() : nullptr;
        st2.lm_inv_depth = k_rho.data();
    }
    int rc = upload(&p2, &st2, /*may_return_early=*/true); // (read_back_marg synchronizes, before the caller's arrays can change)
    if (rc != PVIO_OK) return rc;
    uploaded_ = false; // the device buffers are about to hold a marginalization pass, not a solvable window: whichever way this call ends
    const auto tm1 = Clock::now();
    if ((rc = linearize_once(MODE_MARG, victim)) != PVIO_OK) return rc;
    const Dims &dm = v_.dm;
    const MargGather lay(dm);
    // landmark shards: every rank holds the victim's landmarks of its own range only -> sum the reduced buffers (the IMU
    // factors, the old prior and the rotation prior are replicated and are added once, below, on every rank alike)
    if (sharded_ && comm_allreduce(comm_, v_.red, lay.n[0] + (size_t)world_, 0, stream_)) return fail(PVIO_ERR_COMM, "all-reduce failed");
    const double *h_back = nullptr;
    if ((rc = read_back_marg(lay, &h_back)) != PVIO_OK) return rc;
    const auto tm2 = Clock::now();
    // (the large work arrays are members: a fresh 180 KB vector per call is an mmap, its page faults and an munmap)
    std::vector<double> b, cv;
    assemble_information(lay.host(h_back), pb->preint_valid, pb->prior_frames, dm.prior_n, N, victim, dm.n_tasks, dm.P6, marg_H_, b);
    if (!eliminate_victim(marg_H_, b, N, victim, marg_C_, cv)) return fail(PVIO_ERR_INVALID_ARGUMENT, "singular victim block");
    if (out->info_matrix) std::memcpy(out->info_matrix, marg_C_.data(), sizeof(double) * R * R); // (before sqrt_information uses C up)
    if (out->info_vector) std::memcpy(out->info_vector, cv.data(), sizeof(double) * R);
    out->n = N - 1;
    const SqrtInfoStats eig = sqrt_information(marg_C_, cv, R, marg_V_, out->S, out->s);
    if (solver_switches().timing) // diagnostics: where a marginalization's time goes
        std::fprintf(stderr, "[pvio-hip] marginalize: upload %.0f us, kernels + read-back %.0f us, assembly + elimination %.0f us, eigen-decomposition (%d x %d) %.0f us, sqrt-information %.0f us\n",
                     us(tm0, tm1), us(tm1, tm2), us(tm2, eig.eig_begin), eig.Rk, eig.Rk, us(eig.eig_begin, eig.eig_end), us(eig.eig_end, Clock::now()));
    return PVIO_OK;
}

// Marginal covariances of the window at `st` (pvio_hip_ba_covariance; no reference counterpart).  The first half is marginalize()'s -- upload and
// linearize_once -- in MODE_INIT over the whole window: the robustified, multiplicity-weighted J^T J the solver's own
// iteration 0 sees, constant blocks constant.  The kernels of ba_cov.hip then assemble, scale, invert and scatter on the solver's stream; the
// results come back as ONE copy through a pinned buffer.
int BASolver::covariance(const pvio_ba_problem *pb, const pvio_ba_state *st, pvio_ba_covariance *out) {
    if (!pb || !st || !out || !out->frame_cov) return fail(PVIO_ERR_INVALID_ARGUMENT, "null argument");
    if (sharded_) return fail(PVIO_ERR_UNSUPPORTED, "pvio_hip_ba_covariance: landmark-sharded contexts are not supported");
    const bool timing = solver_switches().timing; // diagnostics: hipEvents around the three kernels
    int rc = upload(pb, st, /*may_return_early=*/true); // (this call synchronizes below, before the caller's arrays can change)
    if (rc != PVIO_OK) return rc;
    uploaded_ = false; // the device buffers are about to hold an undamped linearization, not a solvable window: whichever way this call ends
    if ((rc = linearize_once(MODE_INIT, 0)) != PVIO_OK) return rc;
    const Dims &dm = v_.dm;
    const size_t N = (size_t)dm.N, M = (size_t)dm.M, D = 15 * N;
    // every coordinate that can be free: the pose of a frame that is not fixed, the motion blocks of a 15-dimensional system
    size_t max_coords = 0;
    for (size_t f = 0; f < N; ++f) max_coords += (pb->frame_fixed[f] ? 0 : 6) + (dm.d == 15 ? 9 : 0);
    const CovSlabs lay(N, M, max_coords);
    double *d_res = nullptr, *d_work = nullptr;
    bool grew = false;
    if (!dev(pool_, "cov_result", lay.n_res, &d_res, &grew) || !dev(pool_, "cov_work", lay.n_work, &d_work, &grew)) return fail(PVIO_ERR_OUT_OF_MEMORY, "covariance buffers");
    const size_t n_back = out->joint_cov ? lay.n_res : lay.o_joint;
    double *const h_back = static_cast<double *>(h_cov_.reserve(n_back * sizeof(double), (n_back + n_back / 2) * sizeof(double)));
    if (!h_back) return fail(PVIO_ERR_OUT_OF_MEMORY, "hipHostMalloc failed");
    const CovArgs a = lay.args(d_res, d_work);
    // coordinates that are not free have zero rows and columns in every output: the kernels write the free part only
    if (check(hipMemsetAsync(d_res, 0, lay.n_res * sizeof(double), stream_), "memset")) return PVIO_ERR_HIP;
    if (check(hipMemsetAsync(a.sig6, 0, 36 * N * N * sizeof(double), stream_), "memset")) return PVIO_ERR_HIP;
    if (timing)
        for (hipEvent_t &ev : cov_ev_)
            if (!ev && check(hipEventCreate(&ev), "hipEventCreate")) return PVIO_ERR_HIP;
    hipError_t e;
    if (timing) (void)hipEventRecord(cov_ev_[0], stream_);
    if ((e = launch_cov_assemble(v_, a, stream_)) != hipSuccess) return check(e, "k_cov_assemble");
    if (timing) (void)hipEventRecord(cov_ev_[1], stream_);
    if ((e = launch_cov_invert(v_, a, stream_)) != hipSuccess) return check(e, "k_cov_invert");
    if (timing) (void)hipEventRecord(cov_ev_[2], stream_);
    if (out->lm_var && (e = launch_cov_landmarks(v_, a, stream_)) != hipSuccess) return check(e, "k_cov_landmarks");
    if (timing) (void)hipEventRecord(cov_ev_[3], stream_);
    if (check(hipMemcpyAsync(h_back, d_res, n_back * sizeof(double), hipMemcpyDeviceToHost, stream_), "D2H")) return PVIO_ERR_HIP;
    if (check(hipStreamSynchronize(stream_), "covariance sync")) return PVIO_ERR_HIP;
    stage_in_flight_ = false;
    if (timing)
        for (int k = 0; k < 3; ++k) {
            float ms = 0.0f;
            (void)hipEventElapsedTime(&ms, cov_ev_[k], cov_ev_[k + 1]);
            cov_ms_[k] = ms;
        }
    const CovHdr *hdr = reinterpret_cast<const CovHdr *>(h_back);
    if (hdr->layout_error) return fail(PVIO_ERR_HIP, "k_cov_assemble: unexpected order of the tile tasks");
    out->positive_definite = hdr->positive_definite;
    out->first_bad_coord = hdr->positive_definite ? -1 : hdr->first_bad_coord;
    if (!hdr->positive_definite) return PVIO_OK; // an unobservable window is an answer, not an error: nothing else is written
    std::memcpy(out->frame_cov, h_back + lay.o_frame, N * 225 * sizeof(double));
    if (out->joint_cov) std::memcpy(out->joint_cov, h_back + lay.o_joint, D * D * sizeof(double));
    if (out->lm_var) std::memcpy(out->lm_var, h_back + lay.o_lm, M * sizeof(double));
    if (out->coord_free) std::memcpy(out->coord_free, h_back + lay.o_free, D);
    return PVIO_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// triangulate = validate -> stage -> launch -> fetch (pvio_hip_triangulate).  One buffer on the device and its pinned twin on the host, both
// the call's own and kept between calls: neither the pool nor the View of an uploaded window is touched.
// ---------------------------------------------------------------------------------------------------------------------

// a triangulation call's buffer, in doubles: view_P | obs_z | track_ptr | obs_view | header | results.  The upload is [0, o_res) -- the header
// goes up as zeros --, the read-back is [o_hdr, n_total).
struct TriLayout {
    size_t V = 0, T = 0, n_obs = 0, o_z = 0, o_ptr = 0, o_view = 0, o_hdr = 0, o_res = 0, n_total = 0;
    int max_obs = 0; // the longest track of the call
    void set(size_t V_, size_t T_, size_t n_obs_, int max_obs_) {
        V = V_, T = T_, n_obs = n_obs_, max_obs = max_obs_;
        o_z = 12 * V, o_ptr = o_z + 2 * n_obs, o_view = o_ptr + (T + 2) / 2, o_hdr = o_view + (n_obs + 1) / 2, o_res = o_hdr + 1, n_total = o_res + kTriRecord * T;
    }
    TriArgs args(double *d) const {
        TriArgs a{};
        a.n_tracks = (int32_t)T;
        a.view_P = d, a.obs_z = d + o_z;
        a.track_ptr = reinterpret_cast<const int32_t *>(d + o_ptr), a.obs_view = reinterpret_cast<const int32_t *>(d + o_view);
        a.max_sweeps = reinterpret_cast<int32_t *>(d + o_hdr), a.result = d + o_res;
        return a;
    }
};

// every rejection of include/pvio_hip.h, before anything is written anywhere
int BASolver::validate_tracks(const pvio_tri_problem *pb, const pvio_tri_result *out, TriLayout &lay) {
    if (!pb || !out || !out->point || !out->ok) return fail(PVIO_ERR_INVALID_ARGUMENT, "pvio_hip_triangulate: null argument (point and ok are not optional)");
    if (pb->n_views < 1 || pb->n_tracks < 0) return fail(PVIO_ERR_INVALID_ARGUMENT, "pvio_hip_triangulate: n_views < 1 or n_tracks < 0");
    const size_t T = (size_t)pb->n_tracks;
    if (T == 0) {
        lay.set((size_t)pb->n_views, 0, 0, 0);
        return PVIO_OK;
    }
    if (!pb->view_P || !pb->track_ptr) return fail(PVIO_ERR_INVALID_ARGUMENT, "pvio_hip_triangulate: null view_P or track_ptr");
    if (pb->track_ptr[0] != 0) return fail(PVIO_ERR_INVALID_ARGUMENT, "pvio_hip_triangulate: track_ptr[0] != 0");
    int max_obs = 0;
    for (size_t t = 0; t < T; ++t) {
        const int64_t k = (int64_t)pb->track_ptr[t + 1] - (int64_t)pb->track_ptr[t];
        if (k < 0) return fail(PVIO_ERR_INVALID_ARGUMENT, "pvio_hip_triangulate: track_ptr decreases at track " + std::to_string(t));
        if (k > PVIO_TRI_MAX_OBS) return fail(PVIO_ERR_INVALID_ARGUMENT, "pvio_hip_triangulate: track " + std::to_string(t) + " has more than PVIO_TRI_MAX_OBS observations");
        max_obs = std::max(max_obs, (int)k);
    }
    const size_t n_obs = (size_t)pb->track_ptr[T];
    if (n_obs > 0 && (!pb->obs_view || !pb->obs_z)) return fail(PVIO_ERR_INVALID_ARGUMENT, "pvio_hip_triangulate: null obs_view or obs_z");
    for (size_t o = 0; o < n_obs; ++o)
        if (pb->obs_view[o] < 0 || pb->obs_view[o] >= pb->n_views) return fail(PVIO_ERR_INVALID_ARGUMENT, "pvio_hip_triangulate: obs_view[" + std::to_string(o) + "] is outside [0, n_views)");
    lay.set((size_t)pb->n_views, T, n_obs, max_obs);
    return PVIO_OK;
}

// the inputs into the pinned twin, then ONE copy to the device
int BASolver::stage_tracks(const pvio_tri_problem *pb, const TriLayout &lay) {
    const size_t bytes = lay.n_total * sizeof(double);
    if (!d_tri_.reserve(bytes, bytes + bytes / 2)) return fail(PVIO_ERR_OUT_OF_MEMORY, "hipMalloc failed (triangulation buffer)");
    double *const h = static_cast<double *>(h_tri_.reserve(bytes, bytes + bytes / 2));
    if (!h) return fail(PVIO_ERR_OUT_OF_MEMORY, "hipHostMalloc failed (triangulation buffer)");
    std::memcpy(h, pb->view_P, 12 * lay.V * sizeof(double));
    if (lay.n_obs) std::memcpy(h + lay.o_z, pb->obs_z, 2 * lay.n_obs * sizeof(double));
    std::memset(h + lay.o_ptr, 0, (lay.o_res - lay.o_ptr) * sizeof(double)); // the int arrays' padding and the header
    std::memcpy(h + lay.o_ptr, pb->track_ptr, (lay.T + 1) * sizeof(int32_t));
    if (lay.n_obs) std::memcpy(h + lay.o_view, pb->obs_view, lay.n_obs * sizeof(int32_t));
    return check(hipMemcpyAsync(d_tri_.data(), h, lay.o_res * sizeof(double), hipMemcpyHostToDevice, stream_), "triangulate H2D");
}

int BASolver::launch_tracks(const TriLayout &lay) {
    const bool timing = solver_switches().timing; // diagnostics: hipEvents around the kernel
    if (timing)
        for (hipEvent_t &ev : tri_ev_)
            if (!ev && check(hipEventCreate(&ev), "hipEventCreate")) return PVIO_ERR_HIP;
    if (timing) (void)hipEventRecord(tri_ev_[0], stream_);
    const hipError_t e = launch_triangulate(lay.args(d_tri_.as<double>()), tri_group_lanes(lay.max_obs), stream_);
    if (e != hipSuccess) return check(e, "k_triangulate");
    if (timing) (void)hipEventRecord(tri_ev_[1], stream_);
    return PVIO_OK;
}

// ONE copy back through the pinned twin, then the records into the caller's arrays
int BASolver::fetch_tracks(const TriLayout &lay, pvio_tri_result *out) {
    double *const h = h_tri_.as<double>();
    if (check(hipMemcpyAsync(h + lay.o_hdr, d_tri_.as<double>() + lay.o_hdr, (lay.n_total - lay.o_hdr) * sizeof(double), hipMemcpyDeviceToHost, stream_), "triangulate D2H")) return PVIO_ERR_HIP;
    if (check(hipStreamSynchronize(stream_), "triangulate sync")) return PVIO_ERR_HIP;
    stage_in_flight_ = false; // whatever an upload left queued on the stream has been read as well
    if (solver_switches().timing) {
        float ms = 0.0f;
        (void)hipEventElapsedTime(&ms, tri_ev_[0], tri_ev_[1]);
        tri_ms_ = ms;
    }
    tri_sweeps_ = *reinterpret_cast<const int32_t *>(h + lay.o_hdr);
    for (size_t t = 0; t < lay.T; ++t) {
        const double *rec = h + lay.o_res + kTriRecord * t;
        if (out->homogeneous) std::memcpy(out->homogeneous + 4 * t, rec, 4 * sizeof(double));
        std::memcpy(out->point + 3 * t, rec + 4, 3 * sizeof(double));
        if (out->score) out->score[t] = rec[7];
        out->ok[t] = rec[8] != 0.0 ? 1 : 0;
    }
    return PVIO_OK;
}

int BASolver::triangulate(const pvio_tri_problem *pb, pvio_tri_result *out) {
    TriLayout lay;
    int rc = validate_tracks(pb, out, lay);
    if (rc != PVIO_OK) return rc;
    tri_sweeps_ = 0, tri_ms_ = 0.0;
    if (lay.T == 0) return PVIO_OK;
    if ((rc = stage_tracks(pb, lay)) != PVIO_OK) return rc;
    if ((rc = launch_tracks(lay)) != PVIO_OK) return rc;
    return fetch_tracks(lay, out);
}

// ---------------------------------------------------------------------------------------------------------------------
// plane_ransac = validate -> stage (points + the samples of every hypothesis) -> score -> replay -> refit -> unpack (pvio_hip_plane_ransac).
// One buffer on the device and its pinned twin on the host, both the call's own and kept between calls: neither the pool nor the View of an
// uploaded window is touched.  Two stream round trips: the replay of the stopping rule between them runs on the host (log, pow).
// ---------------------------------------------------------------------------------------------------------------------

// a plane RANSAC call's buffer, in doubles: points | samples (int32) | counts (int32) | models | record | mask (bytes).  The upload is
// [0, o_models) -- the counts go up as zeros --, the first read-back [o_counts, o_record), the second [o_record, n_total).
// PVIO_HIP_PLANE_CHUNK=<points> (experiments, read at every call so that one process can time both forms; rounded up to a multiple of 64, clamped
// to 64 .. 2^24): the points one wave of k_plane_hypotheses scores.  2^24 is the first form, a hypothesis walked by one wave.
static int32_t plane_chunk() {
    const char *s = std::getenv("PVIO_HIP_PLANE_CHUNK");
    const long v = s ? std::atol(s) : (long)kPlaneChunk;
    return (int32_t)((std::min(std::max(v, 64L), (long)kPlaneMaxPoints) + 63) / 64 * 64);
}

struct PlaneLayout {
    size_t n = 0, H = 0, o_samples = 0, o_counts = 0, o_models = 0, o_record = 0, o_mask = 0, n_total = 0;
    void set(size_t n_, size_t H_) {
        n = n_, H = H_;
        o_samples = 3 * n, o_counts = o_samples + (3 * H + 1) / 2, o_models = o_counts + (H + 1) / 2, o_record = o_models + 4 * H;
        o_mask = o_record + kPlaneRecord, n_total = o_mask + (n + 7) / 8;
    }
    PlaneArgs args(double *d, double threshold) const {
        PlaneArgs a{};
        a.n = (int32_t)n, a.n_hyp = (int32_t)H, a.chunk = plane_chunk(), a.threshold = threshold;
        a.points = d, a.samples = reinterpret_cast<const int32_t *>(d + o_samples), a.counts = reinterpret_cast<int32_t *>(d + o_counts);
        a.models = d + o_models, a.record = d + o_record, a.mask = reinterpret_cast<uint8_t *>(d + o_mask);
        return a;
    }
};

// every rejection of include/pvio_hip.h, before anything is written anywhere
int BASolver::validate_points(const pvio_plane_problem *pb, const pvio_plane_result *out) {
    if (!pb || !out) return fail(PVIO_ERR_INVALID_ARGUMENT, "pvio_hip_plane_ransac: null argument");
    if (pb->n_points < 0 || pb->n_points > kPlaneMaxPoints) return fail(PVIO_ERR_INVALID_ARGUMENT, "pvio_hip_plane_ransac: n_points outside [0, 2^24]");
    if (pb->n_points > 0 && (!pb->points || !out->inlier_mask)) return fail(PVIO_ERR_INVALID_ARGUMENT, "pvio_hip_plane_ransac: null points or inlier_mask");
    if (pb->max_iterations < 1 || pb->max_iterations > kPlaneMaxIterations) return fail(PVIO_ERR_INVALID_ARGUMENT, "pvio_hip_plane_ransac: max_iterations outside [1, 4096]");
    if (!std::isfinite(pb->threshold) || pb->threshold < 0.0) return fail(PVIO_ERR_INVALID_ARGUMENT, "pvio_hip_plane_ransac: the threshold is negative or not finite");
    if (std::isnan(pb->confidence)) return fail(PVIO_ERR_INVALID_ARGUMENT, "pvio_hip_plane_ransac: the confidence is NaN");
    return PVIO_OK;
}

// the points and the samples of all H hypotheses, in the order the sequential loop would draw them, into the pinned twin; then ONE copy up
int BASolver::stage_points(const pvio_plane_problem *pb, const PlaneLayout &lay) {
    const size_t bytes = lay.n_total * sizeof(double);
    if (!d_plane_.reserve(bytes, bytes + bytes / 2)) return fail(PVIO_ERR_OUT_OF_MEMORY, "hipMalloc failed (plane RANSAC buffer)");
    double *const h = static_cast<double *>(h_plane_.reserve(bytes, bytes + bytes / 2));
    if (!h) return fail(PVIO_ERR_OUT_OF_MEMORY, "hipHostMalloc failed (plane RANSAC buffer)");
    std::memcpy(h, pb->points, 3 * lay.n * sizeof(double));
    h[lay.o_counts - 1] = 0.0; // the int array's padding
    std::memset(h + lay.o_counts, 0, (lay.o_models - lay.o_counts) * sizeof(double)); // the counts start at 0
    int32_t *const samples = reinterpret_cast<int32_t *>(h + lay.o_samples);
    pvpl::PlSampler sampler((int)lay.n, pb->seed);
    for (size_t k = 0; k < lay.H; ++k) sampler.sample(samples + 3 * k);
    return check(hipMemcpyAsync(d_plane_.data(), h, lay.o_models * sizeof(double), hipMemcpyHostToDevice, stream_), "plane_ransac H2D");
}

// k_plane_hypotheses over every hypothesis; counts and models come back
int BASolver::score_hypotheses(const PlaneLayout &lay, double threshold) {
    const bool timing = solver_switches().timing; // diagnostics: hipEvents around the kernels
    if (timing)
        for (hipEvent_t &ev : plane_ev_)
            if (!ev && check(hipEventCreate(&ev), "hipEventCreate")) return PVIO_ERR_HIP;
    if (timing) (void)hipEventRecord(plane_ev_[0], stream_);
    const hipError_t e = launch_plane_hypotheses(lay.args(d_plane_.as<double>(), threshold), stream_);
    if (e != hipSuccess) return check(e, "k_plane_hypotheses");
    if (timing) (void)hipEventRecord(plane_ev_[1], stream_);
    double *const h = h_plane_.as<double>();
    if (check(hipMemcpyAsync(h + lay.o_counts, d_plane_.as<double>() + lay.o_counts, (lay.o_record - lay.o_counts) * sizeof(double), hipMemcpyDeviceToHost, stream_), "plane_ransac D2H (counts)")) return PVIO_ERR_HIP;
    if (check(hipStreamSynchronize(stream_), "plane_ransac sync")) return PVIO_ERR_HIP;
    stage_in_flight_ = false; // whatever an upload left queued on the stream has been read as well
    plane_scored_ = (int)lay.H;
    if (timing) {
        float ms = 0.0f;
        (void)hipEventElapsedTime(&ms, plane_ev_[0], plane_ev_[1]);
        plane_ms_[0] = ms;
    }
    return PVIO_OK;
}

// k_plane_refit for the winning model; record and mask come back
int BASolver::refit_winner(const PlaneLayout &lay, double threshold, const double *model) {
    const bool timing = solver_switches().timing;
    PlaneArgs a = lay.args(d_plane_.as<double>(), threshold);
    for (int k = 0; k < 4; ++k) a.model[k] = model[k];
    if (timing) (void)hipEventRecord(plane_ev_[2], stream_);
    const hipError_t e = launch_plane_refit(a, stream_);
    if (e != hipSuccess) return check(e, "k_plane_refit");
    if (timing) (void)hipEventRecord(plane_ev_[3], stream_);
    double *const h = h_plane_.as<double>();
    if (check(hipMemcpyAsync(h + lay.o_record, d_plane_.as<double>() + lay.o_record, (lay.n_total - lay.o_record) * sizeof(double), hipMemcpyDeviceToHost, stream_), "plane_ransac D2H (refit)")) return PVIO_ERR_HIP;
    if (check(hipStreamSynchronize(stream_), "plane_ransac sync")) return PVIO_ERR_HIP;
    if (timing) {
        float ms = 0.0f;
        (void)hipEventElapsedTime(&ms, plane_ev_[2], plane_ev_[3]);
        plane_ms_[1] = ms;
    }
    return PVIO_OK;
}

int BASolver::plane_ransac(const pvio_plane_problem *pb, pvio_plane_result *out) {
    int rc = validate_points(pb, out);
    if (rc != PVIO_OK) return rc;
    plane_scored_ = 0, plane_ms_[0] = plane_ms_[1] = 0.0;
    const size_t n = (size_t)pb->n_points;
    uint8_t *const mask = out->inlier_mask; // (the empty result: zeros everywhere, no winner)
    *out = pvio_plane_result{};
    out->inlier_mask = mask, out->best_iteration = -1;
    if (n > 0) std::memset(mask, 0, n);
    if (n < 3) return PVIO_OK; // ransac.h:53-57
    PlaneLayout lay;
    lay.set(n, (size_t)pb->max_iterations);
    if ((rc = stage_points(pb, lay)) != PVIO_OK) return rc;
    if ((rc = score_hypotheses(lay, pb->threshold)) != PVIO_OK) return rc;
    // the sequential loop's bookkeeping over the counts, in the order the samples were drawn; hypotheses beyond its end are not looked at
    const double *const h = h_plane_.as<double>();
    const int32_t *const counts = reinterpret_cast<const int32_t *>(h + lay.o_counts);
    pvpl::PlBest run(pb->confidence, pb->max_iterations);
    int iter = 0;
    for (; iter < run.iter_max; ++iter) run.offer(counts[iter], iter, (int)n);
    out->iterations = iter;
    if (run.best_iter < 0) return PVIO_OK; // no hypothesis had an inlier (a zero threshold, non-finite points)
    const double *const model = h + lay.o_models + 4 * (size_t)run.best_iter;
    if ((rc = refit_winner(lay, pb->threshold, model)) != PVIO_OK) return rc;
    const double *const rec = h + lay.o_record;
    if ((int)rec[0] != run.count)
        return fail(PVIO_ERR_HIP, "pvio_hip_plane_ransac: k_plane_refit counts " + std::to_string((int)rec[0]) + " inliers of the winning model, k_plane_hypotheses counted " + std::to_string(run.count));
    out->n_inliers = run.count, out->best_iteration = run.best_iter, out->refit_valid = rec[1] != 0.0 ? 1 : 0;
    std::memcpy(mask, h + lay.o_mask, n);
    std::memcpy(out->normal, model, 3 * sizeof(double));
    out->distance = model[3];
    std::memcpy(out->refit_normal, rec + 2, 3 * sizeof(double));
    out->refit_distance = rec[5];
    std::memcpy(out->reference_point, rec + 6, 3 * sizeof(double));
    return PVIO_OK;
}

} // namespace pvba

// The kernels of covariance() and their launchers.  They are compiled as part of this translation unit, not as an object of their own: whatever
// builds ba_solver.cpp -- the product Makefile, the fiber emulator of tests/hipemu, the variant builds of tests/micro -- has them without a
// change to its list of sources.
#include "ba_cov.hip"
// The kernel of triangulate() and its launcher, for the same reason.
#include "ba_triangulate.hip"
// ... and the kernels of plane_ransac().
#include "ba_plane.hip"
