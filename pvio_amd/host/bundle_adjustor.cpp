// bundle_adjustor.cpp -- pvio::BundleAdjustor on top of the HIP C-ABI (include/pvio_hip.h).
//
// Drop-in for pvio/src/pvio/estimation/bundle_adjustor.cpp: same class (pimpl included, bundle_adjustor.h:29-42), same
// three methods, same in-place semantics (states are read from and written back into Frame::pose/motion and
// Track::landmark, flags and Plane::tracks are updated like :251-296), same return value (IsSolutionUsable(), :298), no
// exceptions.  What it does NOT contain any more: ceres::Problem assembly and ceres::Solve -- the Map is flattened, in the
// reference's residual-block order, into a pvio_ba_problem and handed to the GPU.
//
// ONE source, two builds (host_seam.h): against the reference's real headers inside the PVIO tree
// (-DPVIO_HOST_USE_REFERENCE_TYPES; `make -C tests/host refcheck` proves that it compiles there), and against the
// look-alike declarations of pvio_min.h for the standalone tests.  Only members that exist in the reference are used:
// frame->image->t, get_preintegration_factor(), Track::flag(f) = v, Factor::create_marginalization_error,
// Map::set/get_marginalization_factor, MarginalizationErrorCost::related_frames() (+ the four accessors of the Ceres-free
// holder, dropin/.../marginalization_error_cost.h), Track::try_triangulate / set_landmark_point / get_landmark_point,
// PlaneExtractor::enough_baseline, Frame::get_pose.  Eigen objects are touched through (i, j), [i], .data() of vectors,
// .coeffs(), .dot() only; every matrix crosses the C ABI element by element (the ABI is row-major, Eigen column-major).
#include "host_seam.h"
#include "flat_layout.h"
#include "ptr_tables.h"

#include <cmath>
#include <cstdio>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <iterator>
#include <mutex>
#include <stdexcept>
#include <algorithm>
#include <cstdint>
#include <unordered_map>

#include "../../include/pvio_hip.h"

// (see device_triangulation() below)
extern "C" int32_t pvio_hip_triangulate(pvio_hip_ctx *ctx, const pvio_tri_problem *problem, pvio_tri_result *out) __attribute__((weak));

namespace pvio {

namespace {

// One GPU context per process: the reference constructs a BundleAdjustor temporary per call
// (sliding_window_tracker.cpp:113), so the context must outlive the object.
pvio_hip_ctx *process_ctx() {
    static pvio_hip_ctx *ctx = nullptr;
    static std::once_flag once;
    std::call_once(once, [] {
        pvio_hip_opts o;
        std::memset(&o, 0, sizeof o);
        o.world_size = 1, o.use_graph = 1;
        // A candidate that is bit-identical to the one just rejected is not evaluated again (include/pvio_hip.h): same iterations, records and
        // results as the reference, which does re-evaluate it; PVIO_HIP_REUSE_CANDIDATES=0 turns it off.
        const char *reuse = std::getenv("PVIO_HIP_REUSE_CANDIDATES");
        o.reuse_identical_candidates = (reuse && std::atoi(reuse) == 0) ? 0 : 1;
        if (const char *dev = std::getenv("PVIO_HIP_DEVICE")) o.device = std::atoi(dev); // one ctx per process and GPU
        if (pvio_hip_abi_version() != PVIO_HIP_ABI_VERSION) { // pvio_hip_opts is copied by value: a library built against another header reads another layout
            std::fprintf(stderr, "[pvio-hip] libpvio_hip.so has ABI version %d, this adapter was built against %d\n", (int)pvio_hip_abi_version(), PVIO_HIP_ABI_VERSION);
            ctx = nullptr;
            return;
        }
        if (pvio_hip_create(&o, &ctx) != PVIO_OK) {
            std::fprintf(stderr, "[pvio-hip] no usable GPU context: BundleAdjustor::solve will report failure\n");
            ctx = nullptr;
        }
    });
    return ctx;
}

struct Flat { // owns the arrays a pvio_ba_problem points into
    std::vector<uint8_t> frame_fixed, pre_valid;
    std::vector<double> cam, imu, sic, intr, fstate, lm_z, obs_z, rho, pre_delta, pre_U, pre_jac, prior_S, prior_s, prior_lin, plane_z, plane_n, plane_d;
    std::vector<int32_t> lm_anchor, lm_ptr, obs_frame, prior_frames, plane_ptr, plane_frame, lm_mult;
    std::vector<Track *> lm_track; // landmark index -> track (write-back)
    std::vector<double> quality;
    std::vector<uint8_t> valid;
    pvio_ba_problem pb;
};

constexpr int kMaxWindow = 64; // windows of more frames are flattened without the observation cache
using FrameIndex = PtrIndex<Frame>; // frame -> window index; room for PtrIndex::kMaxKeys = 128 frames, a window has at most PVIO_MAX_FRAMES

// What ObsCache (ptr_tables.h) asks of a track: the non-anchor observations in keypoint_map() order, i.e. ascending frame id (track.h:69).
struct TrackObservations {
    const Track *track;
    const Frame *anchor;
    size_t id_before_last() const { return std::prev(track->keypoint_map().end(), 2)->first->id(); }
    template <class Put>
    void newest(Put &&put) const {
        const auto last = track->last_keypoint();
        const auto &z = last.first->get_keypoint(last.second);
        put(last.first->id(), z(0), z(1));
    }
    template <class Put>
    void each(Put &&put) const {
        for (const auto &kv : track->keypoint_map()) {
            if (kv.first == anchor) continue; // the anchor observation has no factor (:149)
            const auto &z = kv.first->get_keypoint(kv.second);
            put(kv.first->id(), z(0), z(1));
        }
    }
};

// The reference's block order: frames in map index order (:75-88); inverse depths by first encounter scanning frames then
// keypoint index (:91-103); reprojection blocks per track in ascending frame id with the anchor first (track.h:69).
// (Ceres sums residual blocks frame-major; the flat CSR is landmark-major -- a different summation order, i.e. a
// difference at rounding level only.)
// One method per concern, called in the reference's order by flatten() below; the members are what the steps share.
struct Flattening {
    Map *const map;
    const int N;
    Flat &F;
    ObsCache *cache;           // nullptr: every track is walked from scratch
    PtrSet &visited;           // the tracks that add_landmark() has seen
    FrameIndex fidx;           // frame -> window index
    size_t win_id[kMaxWindow]; // window index -> frame id (ascending), what the cache replays against

    Flattening(Map *map, Flat &F, ObsCache *cache, PtrSet &visited) : map(map), N((int)map->frame_num()), F(F), cache(N > kMaxWindow ? nullptr : cache), visited(visited) {
        // the device path takes windows of at most PVIO_MAX_FRAMES frames (the reference's sliding window holds 10): say so before
        // walking a larger map -- and before the pointer table, which refuses more than FrameIndex::kMaxKeys frames
        if (N > PVIO_MAX_FRAMES) throw std::out_of_range("window of " + std::to_string(N) + " frames: the HIP back-end takes at most " + std::to_string(PVIO_MAX_FRAMES));
        for (int i = 0; i < N; ++i) fidx.put(map->get_frame(i), i);
        for (int i = 0; i < N && i < kMaxWindow; ++i) win_id[i] = map->get_frame(i)->id();
    }

    // frame records (:75-88)
    void frames() {
        F.frame_fixed.assign(N, 0), F.pre_valid.assign(N, 0);
        F.cam.assign(7 * N, 0), F.imu.assign(7 * N, 0), F.sic.assign(4 * N, 0), F.intr.assign(4 * N, 0), F.fstate.assign(16 * N, 0);
        F.pre_delta.assign(11 * N, 0), F.pre_U.assign(225 * N, 0), F.pre_jac.assign(45 * N, 0);
        for (int i = 0; i < N; ++i) {
            Frame *f = map->get_frame(i);
            F.frame_fixed[i] = f->flag(FrameFlag::FF_FIX_POSE) ? 1 : 0;
            flat::put_extrinsic(&F.cam[7 * i], f->camera), flat::put_extrinsic(&F.imu[7 * i], f->imu);
            flat::put_sqrt_inv_cov(&F.sic[4 * i], f->sqrt_inv_cov), flat::put_intrinsics(&F.intr[4 * i], f->K);
            flat::put_state(&F.fstate[16 * i], f);
        }
    }

    // planes with >= 20 tracks constrain their best-plane tracks through the plane-distance factor; tracks of smaller
    // planes fall back to plain reprojection blocks (:165-195)
    std::vector<std::pair<Track *, Plane *>> plane_factor_candidates() const {
        std::vector<std::pair<Track *, Plane *>> candidates;
        for (size_t i = 0; i < map->plane_num(); ++i) {
            Plane *pl = map->get_plane(i);
            if (pl->tracks.size() < 20) continue;
            for (Track *t : pl->tracks)
                if (t->landmark.plane_id == pl->id()) candidates.emplace_back(t, pl); // only under its best plane (:183)
        }
        return candidates;
    }

    // one landmark with its CSR row, unless the track is listed already or its anchor frame is outside the window
    void add_landmark(Track *track) {
        if (!visited.insert(track)) return;
        const auto first = track->first_keypoint();
        const int anchor = fidx.find(first.first);
        if (anchor < 0) return;
        F.lm_track.push_back(track);
        F.lm_anchor.push_back(anchor);
        const auto &za = first.first->get_keypoint(first.second);
        F.lm_z.push_back(za(0)), F.lm_z.push_back(za(1));
        F.rho.push_back(track->landmark.inv_depth);
        if (cache) {
            const ObsCache::Signature sig{track->id(), track->keypoint_num(), first.first->id(), track->last_keypoint().first->id()};
            cache->replay(track, sig, TrackObservations{track, first.first}, win_id, N, [this](int w, double z0, double z1) {
                F.obs_frame.push_back(w);
                F.obs_z.push_back(z0), F.obs_z.push_back(z1);
            });
        } else {
            for (const auto &kv : track->keypoint_map()) {
                if (kv.first == first.first) continue; // the anchor observation has no factor (:149)
                const int t = fidx.find(kv.first);
                if (t < 0) continue;
                const auto &z = kv.first->get_keypoint(kv.second);
                F.obs_frame.push_back(t);
                F.obs_z.push_back(z(0)), F.obs_z.push_back(z(1));
            }
        }
        F.lm_ptr.push_back((int32_t)F.obs_frame.size());
    }

    // the VALID, non-PLANE tracks of the walked frames, by first encounter (:91-103).  `victim` >= 0 (marginalization only): the landmarks are the
    // tracks the victim frame observes (:453-457), in its keypoint order -- the other frames' keypoints are not walked at all.
    void landmarks_of_walked_frames(int victim) {
        visited.reset(F.lm_track.size()); // sized by the previous window
        F.lm_track.clear(), F.lm_anchor.clear(), F.lm_ptr.assign(1, 0), F.obs_frame.clear(), F.lm_z.clear(), F.obs_z.clear(), F.rho.clear();
        if (cache) cache->begin_window(F.obs_frame.capacity());
        for (int i = 0; i < N; ++i) {
            if (victim >= 0 && i != victim) continue;
            Frame *f = map->get_frame(i);
            for (size_t j = 0; j < f->keypoint_num(); ++j) {
                Track *track = f->get_track(j);
                if (!track || !track->flag(TrackFlag::TF_VALID) || track->flag(TrackFlag::TF_PLANE)) continue;
                add_landmark(track);
            }
        }
    }

    // Tracks of planes with fewer than 20 members get their reprojection blocks (again) at :165-179 -- whatever their flags, once per
    // such plane.  A track that already has its blocks from the walk above (VALID, not PLANE), or from another small plane, is listed
    // twice in the ceres::Problem and weighs twice: that is the landmark's multiplicity (include/pvio_hip.h).
    void small_plane_duplicates() {
        bool any_small = false;
        for (size_t i = 0; i < map->plane_num(); ++i) any_small |= map->get_plane(i)->tracks.size() < 20 && !map->get_plane(i)->tracks.empty();
        if (!any_small) return;
        std::unordered_map<const Track *, size_t> index;
        for (size_t l = 0; l < F.lm_track.size(); ++l) index.emplace(F.lm_track[l], l);
        F.lm_mult.assign(F.lm_track.size(), 1);
        for (size_t i = 0; i < map->plane_num(); ++i) {
            if (map->get_plane(i)->tracks.size() >= 20) continue;
            for (Track *t : map->get_plane(i)->tracks) {
                auto it = index.find(t);
                if (it != index.end()) {
                    F.lm_mult[it->second] += 1;
                    continue;
                }
                const size_t before = F.lm_track.size();
                add_landmark(t);
                if (F.lm_track.size() > before) index.emplace(t, before), F.lm_mult.push_back(1);
            }
        }
        if (std::all_of(F.lm_mult.begin(), F.lm_mult.end(), [](int32_t m) { return m == 1; })) F.lm_mult.clear();
    }

    // plane-distance factors (:180-195)
    void plane_distance_factors(const std::vector<std::pair<Track *, Plane *>> &candidates) {
        F.plane_ptr.assign(1, 0), F.plane_frame.clear(), F.plane_z.clear(), F.plane_n.clear(), F.plane_d.clear();
        for (const auto &tp : candidates) {
            for (const auto &kv : tp.first->keypoint_map()) {
                const int t = fidx.find(kv.first);
                if (t < 0) continue;
                const auto &z = kv.first->get_keypoint(kv.second);
                F.plane_frame.push_back(t);
                F.plane_z.push_back(z(0)), F.plane_z.push_back(z(1));
            }
            F.plane_ptr.push_back((int32_t)F.plane_frame.size());
            for (int k = 0; k < 3; ++k) F.plane_n.push_back(tp.second->parameter.normal[k]);
            F.plane_d.push_back(tp.second->parameter.distance);
        }
    }

    // IMU factors: re-integrate at frame_i's current biases first (:224); marginalization reuses the stored delta (:416-450)
    void imu_factors(bool for_marginalization) {
        for (int j = 1; j < N; ++j) {
            Frame *fi = map->get_frame(j - 1), *fj = map->get_frame(j);
            const bool ok = for_marginalization ? fj->get_preintegration_factor() != nullptr
                                                : fj->preintegration.integrate(fj->image->t, fi->motion.bg, fi->motion.ba, true, true);
            if (!ok) continue;
            F.pre_valid[j] = 1;
            flat::put_preintegration(&F.pre_delta[11 * j], &F.pre_U[225 * j], &F.pre_jac[45 * j], fj->preintegration);
        }
    }

    // marginalization prior (:126-139): S, s, the related frames and the linearization states the holder captured
    void prior() {
        F.prior_frames.clear(), F.prior_S.clear(), F.prior_s.clear(), F.prior_lin.clear();
        Factor *mf = map->get_marginalization_factor();
        if (!mf) return;
        const MarginalizationErrorCost *mc = mf->get_cost_function<MarginalizationErrorCost>();
        const std::vector<Frame *> &rel = mc->related_frames();
        for (size_t i = 0; i < rel.size(); ++i) {
            const int pf = fidx.find(rel[i]);
            if (pf < 0) throw std::out_of_range("marginalization prior refers to a frame outside the window"); // unordered_map::at threw here too; caught by the callers
            F.prior_frames.push_back(pf);
            F.prior_lin.resize(16 * (i + 1));
            flat::put_state(&F.prior_lin[16 * i], mc->linearization_pose(i), mc->linearization_motion(i));
        }
        const matrix<> &S = mc->sqrt_information();
        const vector<> &sv = mc->information_vector();
        const size_t D = 15 * rel.size();
        F.prior_S.resize(D * D), F.prior_s.resize(D);
        for (size_t r = 0; r < D; ++r) {
            F.prior_s[r] = sv[r];
            for (size_t c = 0; c < D; ++c) F.prior_S[r * D + c] = S(r, c);
        }
    }

    // the pvio_ba_problem over the arrays filled above
    void bind_problem(Config *config, bool use_inertial) {
        pvio_ba_problem &pb = F.pb;
        std::memset(&pb, 0, sizeof pb);
        pb.n_frames = N, pb.n_landmarks = (int32_t)F.lm_anchor.size(), pb.n_obs = (int32_t)F.obs_frame.size();
        pb.use_inertial = use_inertial ? 1 : 0;
        pb.frame_fixed = F.frame_fixed.data(), pb.cam_extrinsic = F.cam.data(), pb.imu_extrinsic = F.imu.data();
        pb.sqrt_inv_cov = F.sic.data(), pb.intrinsics = F.intr.data();
        pb.lm_anchor_frame = F.lm_anchor.data(), pb.lm_anchor_z = F.lm_z.data(), pb.lm_obs_ptr = F.lm_ptr.data();
        pb.obs_frame = F.obs_frame.data(), pb.obs_z = F.obs_z.data();
        pb.preint_valid = F.pre_valid.data(), pb.preint_delta = F.pre_delta.data(), pb.preint_sqrt_inv_cov = F.pre_U.data(), pb.preint_jacobian = F.pre_jac.data();
        pb.prior_n = (int32_t)F.prior_frames.size(), pb.prior_frames = F.prior_frames.data();
        pb.prior_S = F.prior_S.data(), pb.prior_s = F.prior_s.data(), pb.prior_lin_state = F.prior_lin.data();
        pb.lm_multiplicity = F.lm_mult.empty() ? nullptr : F.lm_mult.data();
        pb.n_plane_factors = (int32_t)F.plane_d.size();
        pb.plane_obs_ptr = F.plane_ptr.data(), pb.plane_obs_frame = F.plane_frame.data(), pb.plane_obs_z = F.plane_z.data();
        pb.plane_normal = F.plane_n.data(), pb.plane_distance = F.plane_d.data();
        pb.plane_sqrt_inv_cov = std::sqrt(1.0 / config->plane_distance_cov()); // :181
        pb.max_iterations = (int32_t)config->solver_iteration_limit();
        pb.max_solver_time = config->solver_time_limit();
    }
};

void flatten(Map *map, Config *config, bool use_inertial, bool for_marginalization, Flat &F, ObsCache *cache = nullptr, int victim = -1) {
    static thread_local PtrSet visited; // keeps its table between solves
    Flattening w(map, F, cache, visited);
    w.frames();
    std::vector<std::pair<Track *, Plane *>> plane_candidates;
    if (!for_marginalization) plane_candidates = w.plane_factor_candidates();
    w.landmarks_of_walked_frames(victim);
    F.lm_mult.clear();
    if (!for_marginalization) w.small_plane_duplicates();
    w.plane_distance_factors(plane_candidates);
    if (use_inertial || for_marginalization) w.imu_factors(for_marginalization);
    w.prior();
    w.bind_problem(config, use_inertial);
}

// ---- post-solve passes (bundle_adjustor.cpp:251-296), host side ---------------------------------------------------
// depth gate + mean pixel error of one track from the map's current states (:279-295); false when the gate fails
bool track_quality(const Track *track, double &quality) {
    const vector<3> x = track->get_landmark_point();
    double sum = 0, num = 0;
    for (const auto &fk : track->keypoint_map()) {
        const Frame *frame = fk.first;
        const PoseState cam = frame->get_pose(frame->camera);
        const vector<3> y = cam.q.conjugate() * (x - cam.p);
        if (y.z() <= 1.0e-3 || y.z() > 50) return false;
        const vector<2> &z = frame->get_keypoint(fk.second);
        const double du = (y.x() / y.z() * frame->K(0, 0) + frame->K(0, 2)) - (z[0] * frame->K(0, 0) + frame->K(0, 2)); // apply_k, stereo.h:25-27
        const double dv = (y.y() / y.z() * frame->K(1, 1) + frame->K(1, 2)) - (z[1] * frame->K(1, 1) + frame->K(1, 2));
        sum += std::sqrt(du * du + dv * dv), num += 1.0;
    }
    quality = sum / std::max(num, 1.0);
    return true;
}

// PVIO_HIP_DEVICE_TRIANGULATION=1 (read once; default off): the re-validation below triangulates its tracks in one pvio_hip_triangulate call
// in place of one host SVD per track (Track::try_triangulate).  The reference to that entry point is weak (below, outside the namespaces): it
// was added without a change of PVIO_HIP_ABI_VERSION, so a back end of the same ABI version may not have it (an older libpvio_hip.so; the
// oracle-backed C ABI of the parity chain), and an option that is off by default must not keep the adapter from loading above one.  Asking for
// the device path above such a back end is reported once and the host path is taken.
bool device_triangulation() {
    static const bool on = [] {
        const char *v = std::getenv("PVIO_HIP_DEVICE_TRIANGULATION");
        if (!(v && std::atoi(v) != 0)) return false;
        if (!pvio_hip_triangulate) {
            std::fprintf(stderr, "[pvio-hip] PVIO_HIP_DEVICE_TRIANGULATION: this back end has no pvio_hip_triangulate, the plane tracks are triangulated on the host\n");
            return false;
        }
        return true;
    }();
    return on;
}

// Track::try_triangulate (track.cpp:61-80) for all of `tracks` at once: view_P = [R | -R p], R = R_wc^T, of every frame's current camera pose,
// one pvio_hip_triangulate call.  ok[i] / point[i] are what try_triangulate returns / writes.  A track the call does not take (more than
// PVIO_TRI_MAX_OBS observations, a frame outside the map) is marked in `on_host` and left to try_triangulate; false: the call itself failed.
bool triangulate_on_device(pvio_hip_ctx *ctx, Map *map, const std::vector<Track *> &tracks, std::vector<uint8_t> &ok, std::vector<double> &point, std::vector<uint8_t> &on_host) {
    static thread_local std::vector<double> view_P, obs_z;
    static thread_local std::vector<int32_t> track_ptr, obs_view;
    static thread_local FrameIndex index;
    const size_t V = map->frame_num();
    index.clear();
    view_P.resize(12 * V);
    for (size_t i = 0; i < V; ++i) {
        const Frame *frame = map->get_frame(i);
        index.put(frame, (int)i);
        const PoseState cam = frame->get_pose(frame->camera);
        const double x = cam.q.coeffs()[0], y = cam.q.coeffs()[1], z = cam.q.coeffs()[2], w = cam.q.coeffs()[3];
        const double R[3][3] = {{1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)},  // R_wc
                                {2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)},
                                {2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)}};
        double *P = &view_P[12 * i];
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) P[4 * r + c] = R[c][r];
            P[4 * r + 3] = -(R[0][r] * cam.p[0] + R[1][r] * cam.p[1] + R[2][r] * cam.p[2]);
        }
    }
    const size_t T = tracks.size();
    track_ptr.assign(1, 0), obs_view.clear(), obs_z.clear();
    on_host.assign(T, 0);
    for (size_t i = 0; i < T; ++i) {
        const size_t first = obs_view.size();
        if (tracks[i]->keypoint_num() > PVIO_TRI_MAX_OBS) on_host[i] = 1;
        else
            for (const auto &fk : tracks[i]->keypoint_map()) {
                const int v = index.find(fk.first);
                if (v < 0) {
                    on_host[i] = 1;
                    break;
                }
                const vector<2> &kp = fk.first->get_keypoint(fk.second);
                obs_view.push_back(v), obs_z.push_back(kp[0]), obs_z.push_back(kp[1]);
            }
        if (on_host[i]) obs_view.resize(first), obs_z.resize(2 * first); // an empty track: the device reports ok = 0, the caller does not look
        track_ptr.push_back((int32_t)obs_view.size());
    }
    ok.assign(T, 0), point.assign(3 * T, 0.0);
    pvio_tri_problem pb{(int32_t)V, (int32_t)T, view_P.data(), track_ptr.data(), obs_view.data(), obs_z.data()};
    pvio_tri_result out{point.data(), ok.data(), nullptr, nullptr};
    if (pvio_hip_triangulate(ctx, &pb, &out) != PVIO_OK) {
        std::fprintf(stderr, "[pvio-hip] triangulate failed: %s (the plane tracks are triangulated on the host)\n", pvio_hip_last_error(ctx));
        return false;
    }
    return true;
}

// :251-275 -- PLANE tracks that can be triangulated on their own are checked against the planes they sit in (0.1 m): a
// plane that does not hold the point loses the track, a track that no plane holds goes back to being an ordinary VALID
// landmark at the triangulated point.  Returns the tracks whose inverse depth it replaced.  The triangulations are one host SVD per track
// (Track::try_triangulate) or, with device_triangulation(), one call for all of them; the gate and what follows it are the same code.
std::vector<Track *> revalidate_plane_tracks(Map *map, pvio_hip_ctx *ctx, size_t *on_device_count) {
    std::vector<Track *> moved;
    static thread_local std::vector<Track *> candidates;
    static thread_local std::vector<uint8_t> ok, on_host;
    static thread_local std::vector<double> point;
    candidates.clear();
    for (size_t i = 0; i < map->track_num(); ++i) {
        Track *track = map->get_track(i);
        if (!track->flag(TrackFlag::TF_PLANE)) continue;
        if (track->keypoint_num() < 2) continue;
        if (!(track->life > 10 && PlaneExtractor::enough_baseline(track))) continue;
        candidates.push_back(track);
    }
    const bool device = device_triangulation() && ctx && !candidates.empty() && triangulate_on_device(ctx, map, candidates, ok, point, on_host);
    *on_device_count = 0;
    for (size_t i = 0; i < candidates.size(); ++i) {
        Track *track = candidates[i];
        vector<3> p;
        if (device && !on_host[i]) {
            ++*on_device_count;
            if (!ok[i]) continue;
            for (int k = 0; k < 3; ++k) p[k] = point[3 * i + k];
        } else if (!track->try_triangulate(p)) {
            continue;
        }
        bool held = false;
        for (size_t j = 0; j < map->plane_num(); ++j) {
            Plane *plane = map->get_plane(j);
            if (plane->tracks.count(track) == 0) continue;
            if (std::abs(plane->parameter.normal.dot(p) - plane->parameter.distance) > 0.1) plane->tracks.erase(track);
            else held = true;
        }
        if (!held) {
            track->flag(TrackFlag::TF_PLANE) = false;
            track->flag(TrackFlag::TF_VALID) = true;
            track->set_landmark_point(p);
            moved.push_back(track);
        }
    }
    return moved;
}

struct DefaultConfig : Config { // solver_iteration_limit / solver_time_limit / plane_distance_cov defaults (config.cpp:24-26,82-88)
    matrix<3> camera_intrinsic() const override { return matrix<3>(); }
    quaternion camera_to_body_rotation() const override { return quaternion(); }
    vector<3> camera_to_body_translation() const override { return vector<3>(); }
    quaternion imu_to_body_rotation() const override { return quaternion(); }
    vector<3> imu_to_body_translation() const override { return vector<3>(); }
    matrix<2> keypoint_noise_cov() const override { return matrix<2>(); }
    matrix<3> gyroscope_noise_cov() const override { return matrix<3>(); }
    matrix<3> accelerometer_noise_cov() const override { return matrix<3>(); }
    matrix<3> gyroscope_bias_noise_cov() const override { return matrix<3>(); }
    matrix<3> accelerometer_bias_noise_cov() const override { return matrix<3>(); }
};

// tests: the cached flattening against a walk from scratch
void verify_flattening(Map *map, Config *config, bool use_inertial, const Flat &F) {
    Flat G;
    flatten(map, config, use_inertial, false, G, nullptr);
    if (G.lm_track != F.lm_track || G.lm_anchor != F.lm_anchor || G.lm_ptr != F.lm_ptr || G.obs_frame != F.obs_frame || G.obs_z != F.obs_z || G.lm_z != F.lm_z || G.rho != F.rho)
        throw std::logic_error("incremental flattening differs from the walk from scratch");
}

// write the states back in place, like Ceres does through the parameter-block pointers
void write_back_states(Map *map, const Flat &F, bool use_inertial) {
    const bool motion_blocks = use_inertial || map->get_marginalization_factor() != nullptr;
    for (size_t i = 0; i < map->frame_num(); ++i) flat::write_back_state(&F.fstate[16 * i], map->get_frame(i), motion_blocks);
    for (size_t l = 0; l < F.lm_track.size(); ++l) F.lm_track[l]->landmark.inv_depth = F.rho[l];
}

// ---- the gate and the quality of :279-295.  For the flattened landmarks both come from the device (k_quality, evaluated on the final
// states); the tracks the device never saw (PLANE tracks of planes with >= 20 tracks, tracks the re-validation has just moved) are done
// on the host. ----
void apply_device_quality(const Flat &F, const std::vector<Track *> &moved, PtrSet &on_device) {
    on_device.reset(F.lm_track.size());
    for (size_t l = 0; l < F.lm_track.size(); ++l) {
        Track *t = F.lm_track[l];
        if (std::find(moved.begin(), moved.end(), t) != moved.end()) continue; // its point changed after the solve
        if (!t->flag(TrackFlag::TF_VALID) && !t->flag(TrackFlag::TF_PLANE)) continue; // (:279)
        on_device.insert(t);
        if (!F.valid[l]) t->flag(TrackFlag::TF_VALID) = false, t->flag(TrackFlag::TF_PLANE) = false; // depth gate (:286-290)
        else if (t->flag(TrackFlag::TF_VALID)) t->landmark.quality = F.quality[l];                  // (:294-295)
    }
}
void apply_host_quality(Map *map, const PtrSet &on_device) {
    for (size_t i = 0; i < map->track_num(); ++i) {
        Track *t = map->get_track(i);
        if (!t->flag(TrackFlag::TF_VALID) && !t->flag(TrackFlag::TF_PLANE)) continue;
        if (on_device.contains(t)) continue;
        double q = 0;
        if (!track_quality(t, q)) t->flag(TrackFlag::TF_VALID) = false, t->flag(TrackFlag::TF_PLANE) = false;
        else if (t->flag(TrackFlag::TF_VALID)) t->landmark.quality = q;
    }
}

// The new prior over the frames that remain, from the row-major S (D x D) and s (D) of pvio_hip_ba_marginalize.
void install_prior(Map *map, size_t victim, const std::vector<double> &S, const std::vector<double> &s) {
    const size_t D = s.size();
    matrix<> sqrt_infomat;
    vector<> sqrt_infovec;
    sqrt_infomat.resize((int)D, (int)D), sqrt_infovec.resize((int)D);
    for (size_t r = 0; r < D; ++r) {
        sqrt_infovec[(int)r] = s[r];
        for (size_t c = 0; c < D; ++c) sqrt_infomat((int)r, (int)c) = S[r * D + c];
    }
    std::vector<Frame *> remaining; // linearized at their current states by the holder's constructor (:592-598)
    for (size_t i = 0; i < map->frame_num(); ++i)
        if (i != victim) remaining.emplace_back(map->get_frame(i));
    map->set_marginalization_factor(Factor::create_marginalization_error(sqrt_infomat, sqrt_infovec, std::move(remaining)));
}

// Whatever goes wrong in marginalize_frame, Map::marginalize_frame erases the victim right after the call (map.cpp:78-87): a prior that
// still names it would hold a dangling Frame* and make every later flatten fail or match a recycled address.
// So the map never keeps the old prior past a failed marginalization: it is dropped (the window loses its gauge prior
// until the next successful one -- the solve stays well-posed through the IMU factors, and says so on stderr).
struct DropStalePrior {
    Map *map;
    bool armed = true;
    ~DropStalePrior() {
        if (armed && map->get_marginalization_factor()) {
            std::fprintf(stderr, "[pvio-hip] marginalize_frame failed: the old prior is dropped (it names the frame that is being erased)\n");
            map->set_marginalization_factor(nullptr);
        }
    }
};

// PVIO_HIP_TIMING (read once): the host share of a keyframe solve and of a marginalization, one stderr line per call.
bool timing_lines() {
    static const bool on = std::getenv("PVIO_HIP_TIMING") != nullptr;
    return on;
}
class Stopwatch { // microseconds since its construction or the last lap
  public:
    double lap_us() {
        const auto now = std::chrono::steady_clock::now();
        const double us = std::chrono::duration<double, std::micro>(now - last_).count();
        last_ = now;
        return us;
    }

  private:
    std::chrono::steady_clock::time_point last_ = std::chrono::steady_clock::now();
};

} // namespace

// diagnostics (tests/host/roundtrip.cpp): seconds per flattening of `map`, steady state (the arrays keep their capacity)
// reps > 0: walk from scratch every time; reps < 0: |reps| repetitions with the observation cache (steady state of an unchanged window)
double flatten_seconds(Map *map, bool use_inertial, int reps) {
    DefaultConfig dc;
    Flat F;
    ObsCache cache;
    ObsCache *c = reps < 0 ? &cache : nullptr;
    if (reps < 0) reps = -reps;
    flatten(map, &dc, use_inertial, false, F, c);
    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < reps; ++i) flatten(map, &dc, use_inertial, false, F, c);
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() / (reps > 0 ? reps : 1);
}

struct BundleAdjustor::BundleAdjustorSolver { // the pimpl of bundle_adjustor.h:30,41; the GPU context is process-wide, see process_ctx()
    Flat F; // a BundleAdjustor temporary lives for one call: the arrays that should keep their capacity are thread_local below

    static Flat &window() {
        static thread_local Flat F; // keeps the capacity of its arrays from one keyframe to the next
        return F;
    }
    static ObsCache &obs_cache() {
        static thread_local ObsCache c; // the flattened observation lists of the tracks, kept from one keyframe to the next
        return c;
    }

    // post-solve passes (:251-296) included
    bool solve(Map *map, Config *config, bool use_inertial) {
        pvio_hip_ctx *ctx = process_ctx();
        if (!ctx) return false;
        DefaultConfig dc;
        if (!config) config = &dc;
        Flat &F = window();
        static const bool no_cache = std::getenv("PVIO_HIP_FLATTEN_NOCACHE") != nullptr;
        Stopwatch watch;
        flatten(map, config, use_inertial, false, F, no_cache ? nullptr : &obs_cache());
        const double flatten_us = watch.lap_us();
        if (std::getenv("PVIO_HIP_FLATTEN_VERIFY")) verify_flattening(map, config, use_inertial, F); // read per call: a test sets it after load

        F.quality.assign(F.lm_track.size(), 0.0), F.valid.assign(F.lm_track.size(), 1);
        pvio_ba_state st{F.fstate.data(), F.rho.data(), F.quality.data(), F.valid.data()};
        pvio_ba_summary sum;
        std::memset(&sum, 0, sizeof sum);
        if (pvio_hip_ba_solve(ctx, &F.pb, &st, &sum) != PVIO_OK) {
            std::fprintf(stderr, "[pvio-hip] ba_solve failed: %s\n", pvio_hip_last_error(ctx));
            return false;
        }
        const double call_us = watch.lap_us();

        write_back_states(map, F, use_inertial);
        Stopwatch reval_watch;
        size_t reval_on_device = 0;
        const std::vector<Track *> moved = revalidate_plane_tracks(map, ctx, &reval_on_device);
        const double reval_us = reval_watch.lap_us();
        static thread_local PtrSet on_device;
        apply_device_quality(F, moved, on_device);
        apply_host_quality(map, on_device);

        if (timing_lines()) {
            std::fprintf(stderr, "[pvio-hip] solve: %d frames, %d landmarks, %d factors: flatten %.1f us, upload+solve+download %.1f us (device %.1f us, %d iterations), write-back + post passes %.1f us\n",
                         F.pb.n_frames, F.pb.n_landmarks, F.pb.n_obs, flatten_us, call_us, 1e6 * sum.device_seconds, sum.num_iterations, watch.lap_us());
            std::fprintf(stderr, "[pvio-hip] plane re-validation: %.1f us, %zu tracks triangulated on the device, %zu tracks moved (PVIO_HIP_DEVICE_TRIANGULATION %s)\n",
                         reval_us, reval_on_device, moved.size(), device_triangulation() ? "on" : "off");
        }
        return sum.is_usable != 0;
    }

    void marginalize_frame(Map *map, size_t index) {
        DropStalePrior guard{map}; // first: every way out of this function below leaves no prior that names the victim
        pvio_hip_ctx *ctx = process_ctx();
        if (!ctx || index >= map->frame_num() || map->frame_num() < 2) return;
        DefaultConfig dc;
        Stopwatch watch;
        flatten(map, &dc, true, true, F, &obs_cache(), (int)index); // the tracks were flattened by the last solve: their lists are replayed
        const double flatten_us = watch.lap_us();

        const size_t D = 15 * (map->frame_num() - 1);
        std::vector<double> S(D * D, 0.0), s(D, 0.0); // row-major, like the C ABI
        pvio_ba_state st{F.fstate.data(), F.rho.data(), nullptr, nullptr};
        pvio_ba_prior out;
        std::memset(&out, 0, sizeof out);
        out.S = S.data(), out.s = s.data();
        if (pvio_hip_ba_marginalize(ctx, &F.pb, &st, (int32_t)index, &out) != PVIO_OK) {
            std::fprintf(stderr, "[pvio-hip] ba_marginalize failed: %s\n", pvio_hip_last_error(ctx));
            return;
        }
        const double call_us = watch.lap_us();

        install_prior(map, index, S, s);
        guard.armed = false;
        if (timing_lines())
            std::fprintf(stderr, "[pvio-hip] marginalize_frame: %d frames, %d landmarks: flatten %.1f us, pvio_hip_ba_marginalize %.1f us, new prior factor %.1f us\n",
                         F.pb.n_frames, F.pb.n_landmarks, flatten_us, call_us, watch.lap_us());
    }

    double compute_reprojection_error(Map *map) {
        pvio_hip_ctx *ctx = process_ctx();
        if (!ctx) return 0.0;
        DefaultConfig dc;
        flatten(map, &dc, false, true, F);
        pvio_ba_state st{F.fstate.data(), F.rho.data(), nullptr, nullptr};
        double err = 0;
        if (pvio_hip_ba_reprojection_error(ctx, &F.pb, &st, &err) != PVIO_OK) return 0.0;
        return err;
    }
};

BundleAdjustor::BundleAdjustor() { solver = std::make_unique<BundleAdjustorSolver>(); }
BundleAdjustor::~BundleAdjustor() = default;

// The reference's methods do not throw (Ceres reports failure through the summary); neither do these: anything the
// flattening or the standard library raises (bad_alloc, a prior that names a frame outside the window) ends the call as
// "not usable" / "no new prior" with one line on stderr.
// The reference's forensics timers at the two seams (bundle_adjustor.cpp:308-319 running average of the solve time, :349-353
// marginalization time: pvio-pc's "BA Time" graphs, main.cpp:165-167).  Inside the PVIO tree they are the reference's own
// `forensics` / `make_timer` (forensics.h:96-101, utility/unique_timer.h) and obey PVIO_ENABLE_FORENSICS like there; the standalone
// test build has neither header and no GUI to feed.
#ifdef PVIO_HOST_USE_REFERENCE_TYPES
#define PVIO_HOST_SOLVE_TIMER()                                              \
    auto ba_timer = make_timer([](double t) {                                \
        forensics(bundle_adjustor_solve_time, time) {                        \
            static double avg_time = 0;                                      \
            static double avg_count = 0;                                     \
            avg_time = (avg_time * avg_count + t) / (avg_count + 1);         \
            avg_count += 1.0;                                                \
            time = avg_time;                                                 \
        }                                                                    \
    })
#define PVIO_HOST_MARG_TIMER()                                               \
    auto ba_timer = make_timer([](double t) {                                \
        forensics(bundle_adjustor_marginalization_time, time) { time = t; }  \
    })
#else
#define PVIO_HOST_SOLVE_TIMER() ((void)0)
#define PVIO_HOST_MARG_TIMER() ((void)0)
#endif

bool BundleAdjustor::solve(Map *map, Config *config, bool use_inertial) {
    PVIO_HOST_SOLVE_TIMER();
    try {
        return solver->solve(map, config, use_inertial);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "[pvio-hip] BundleAdjustor::solve: %s\n", e.what());
        return false;
    }
}

void BundleAdjustor::marginalize_frame(Map *map, size_t index) {
    PVIO_HOST_MARG_TIMER();
    try {
        solver->marginalize_frame(map, index);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "[pvio-hip] BundleAdjustor::marginalize_frame: %s\n", e.what());
    }
}

double BundleAdjustor::compute_reprojection_error(Map *map) {
    try {
        return solver->compute_reprojection_error(map);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "[pvio-hip] BundleAdjustor::compute_reprojection_error: %s\n", e.what());
        return 0.0;
    }
}

} // namespace pvio