"""Thin ctypes driver over the C-ABI (include/pvio_hip.h) used by tests and bench.py.

It adds nothing to the product path: every call goes straight into libpvio_hip.so.
"""
import ctypes as C

import numpy as np

from . import capi
from .problem import BAState, BASummary


class HipError(RuntimeError):
    pass


class HipContext:
    def __init__(self, device=0, rank=0, world_size=1, use_graph=True, lib=None, debug_fail_factorizations=0, debug_invalid_steps=0,
                 linearize_mode=0, force_sharded=False, reuse_identical_candidates=False):
        self.lib = lib or capi.load()
        opts = capi.HipOpts()
        opts.device, opts.rank, opts.world_size, opts.use_graph = device, rank, world_size, int(use_graph)
        opts.debug_fail_factorizations, opts.debug_invalid_steps = debug_fail_factorizations, debug_invalid_steps  # tests only
        opts.linearize_mode = linearize_mode
        opts.debug_force_sharded = int(force_sharded)
        opts.reuse_identical_candidates = int(reuse_identical_candidates)  # pvio_hip_opts: skip re-evaluating a bit-identical rejected candidate
        self.ctx = C.c_void_p()
        rc = self.lib.pvio_hip_create(C.byref(opts), C.byref(self.ctx))
        if rc != 0:
            raise HipError("pvio_hip_create failed with status %d (no usable GPU? there is no CPU fallback)" % rc)
        self._keep = None

    def close(self):
        if self.ctx:
            self.lib.pvio_hip_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            msg = self.lib.pvio_hip_last_error(self.ctx)
            raise HipError("%s failed: status %d (%s)" % (what, rc, msg.decode() if msg else ""))

    # one-shot: upload + solve + download (what the BundleAdjustor adapter calls)
    def solve(self, problem, state=None, summary=None, trace=True):
        state = state or BAState(problem)
        summary = summary or BASummary(problem, trace=trace)
        pb, st = problem.as_c(), state.as_c()
        self._check(self.lib.pvio_hip_ba_solve(self.ctx, C.byref(pb), C.byref(st), C.byref(summary.c)), "pvio_hip_ba_solve")
        return state, summary

    # device-resident variant (bench): upload once, solve many times from the same initial state
    def upload(self, problem, state=None):
        state = state or BAState(problem)
        pb, st = problem.as_c(), state.as_c()
        self._keep = (problem, state)
        self._check(self.lib.pvio_hip_ba_upload(self.ctx, C.byref(pb), C.byref(st)), "pvio_hip_ba_upload")
        return state

    def graph_replays(self):
        """solves of this context that ran as a replay of the captured slot graph"""
        self.lib.pvio_hip_ba_graph_replays.argtypes = [C.c_void_p]
        return int(self.lib.pvio_hip_ba_graph_replays(self.ctx))

    def last_candidate_repeats(self):
        """candidate evaluations the last solve short-circuited (reuse_identical_candidates)"""
        self.lib.pvio_hip_ba_last_candidate_repeats.argtypes = [C.c_void_p]
        return int(self.lib.pvio_hip_ba_last_candidate_repeats(self.ctx))

    def solve_resident(self, summary):
        self._check(self.lib.pvio_hip_ba_solve_resident(self.ctx, C.byref(summary.c)), "pvio_hip_ba_solve_resident")
        return summary

    def profile_resident(self, summary):
        """One resident solve with hipEvents around every kernel launch -> {kernel: (total_ms, launches)}."""
        kt = capi.BAKernelTimesC()
        self._check(self.lib.pvio_hip_ba_profile_resident(self.ctx, C.byref(summary.c), C.byref(kt)), "pvio_hip_ba_profile_resident")
        names = ["k_linearize", "k_reduce", "k_dense", "k_backsub"]
        self.last_phase_ticks = {n: [int(x) for x in kt.phase_ticks[i]] for i, n in enumerate(names)}
        # landmark-sharded solves: the two exchange steps of an iteration (zero on a single GPU)
        self.last_comm = {"allreduce_system": (kt.comm_ms[0], kt.comm_launches[0]), "allreduce_backsub": (kt.comm_ms[1], kt.comm_launches[1])}
        return {n: (kt.total_ms[i], kt.launches[i]) for i, n in enumerate(names)}

    def download(self, state):
        st = state.as_c()
        self._check(self.lib.pvio_hip_ba_download(self.ctx, C.byref(st)), "pvio_hip_ba_download")
        return state

    def reprojection_error(self, problem, state):
        pb, st = problem.as_c(), state.as_c()
        out = C.c_double(0)
        self._check(self.lib.pvio_hip_ba_reprojection_error(self.ctx, C.byref(pb), C.byref(st), C.byref(out)), "reprojection_error")
        return out.value

    def marginalize(self, problem, state, victim, want_info=True):
        pb, st = problem.as_c(), state.as_c()
        n = problem.n_frames - 1
        S, s = np.zeros((15 * n, 15 * n)), np.zeros(15 * n)
        IM, iv = np.zeros((15 * n, 15 * n)), np.zeros(15 * n)
        pr = capi.BAPriorC()
        pr.S, pr.s = S.ctypes.data_as(capi.c_double_p), s.ctypes.data_as(capi.c_double_p)
        if want_info:
            pr.info_matrix, pr.info_vector = IM.ctypes.data_as(capi.c_double_p), iv.ctypes.data_as(capi.c_double_p)
        self._check(self.lib.pvio_hip_ba_marginalize(self.ctx, C.byref(pb), C.byref(st), int(victim), C.byref(pr)), "pvio_hip_ba_marginalize")
        return S, s, IM, iv

    def covariance(self, problem, state, joint=False, landmarks=False, into=None):
        """pvio_hip_ba_covariance: marginal covariances of the window at `state` (include/pvio_hip.h).  Returns a dict: positive_definite,
        first_bad_coord, frame_cov [N, 15, 15], coord_free [15 N] and, on request, joint_cov [15 N, 15 N] and lm_var [M].  `into`: arrays of
        those names to be written in place of fresh ones (an unobservable window leaves them as they are)."""
        pb, st = problem.as_c(), state.as_c()
        N, M = problem.n_frames, problem.n_landmarks
        into = into or {}
        res = dict(frame_cov=into.get("frame_cov", np.zeros((N, 15, 15))), coord_free=into.get("coord_free", np.zeros(15 * N, np.uint8)))
        if joint:
            res["joint_cov"] = into.get("joint_cov", np.zeros((15 * N, 15 * N)))
        if landmarks:
            res["lm_var"] = into.get("lm_var", np.zeros(max(M, 1))[:M])
        cv = capi.BACovarianceC()
        cv.positive_definite, cv.first_bad_coord = -1, -1
        cv.frame_cov = res["frame_cov"].ctypes.data_as(capi.c_double_p)
        cv.coord_free = res["coord_free"].ctypes.data_as(capi.c_uint8_p)
        if joint:
            cv.joint_cov = res["joint_cov"].ctypes.data_as(capi.c_double_p)
        if landmarks:
            cv.lm_var = res["lm_var"].ctypes.data_as(capi.c_double_p)
        self._check(self.lib.pvio_hip_ba_covariance(self.ctx, C.byref(pb), C.byref(st), C.byref(cv)), "pvio_hip_ba_covariance")
        res["positive_definite"], res["first_bad_coord"] = int(cv.positive_definite), int(cv.first_bad_coord)
        return res

    def covariance_kernel_ms(self):
        """hipEvent ms of k_cov_assemble, k_cov_invert, k_cov_landmarks in the last covariance() (recorded only with PVIO_HIP_TIMING set)"""
        ms = np.zeros(3)
        self._check(self.lib.pvio_hip_ba_covariance_kernel_ms(self.ctx, ms.ctypes.data_as(capi.c_double_p)), "pvio_hip_ba_covariance_kernel_ms")
        return ms

    def triangulate(self, view_P, track_ptr, obs_view, obs_z, homogeneous=False):
        """pvio_hip_triangulate: batched multi-view DLT triangulation (include/pvio_hip.h).  view_P [V, 3, 4] (or [V, 12]) onto normalized image
        coordinates, track_ptr [T + 1] CSR over obs_view [n] / obs_z [n, 2].  Returns a dict: point [T, 3], ok [T] (uint8), score [T] and, on
        request, homogeneous [T, 4]."""
        view_P = np.ascontiguousarray(view_P, np.float64).reshape(-1, 12)
        track_ptr = np.ascontiguousarray(track_ptr, np.int32)
        obs_view = np.ascontiguousarray(obs_view, np.int32)
        obs_z = np.ascontiguousarray(obs_z, np.float64).reshape(-1, 2)
        T = track_ptr.shape[0] - 1
        res = dict(point=np.zeros((T, 3)), ok=np.zeros(T, np.uint8), score=np.zeros(T))
        if homogeneous:
            res["homogeneous"] = np.zeros((T, 4))
        pb, out = capi.TriProblemC(), capi.TriResultC()
        pb.n_views, pb.n_tracks = view_P.shape[0], T
        pb.view_P, pb.obs_z = view_P.ctypes.data_as(capi.c_double_p), obs_z.ctypes.data_as(capi.c_double_p)
        pb.track_ptr, pb.obs_view = track_ptr.ctypes.data_as(capi.c_int32_p), obs_view.ctypes.data_as(capi.c_int32_p)
        out.point, out.ok, out.score = res["point"].ctypes.data_as(capi.c_double_p), res["ok"].ctypes.data_as(capi.c_uint8_p), res["score"].ctypes.data_as(capi.c_double_p)
        if homogeneous:
            out.homogeneous = res["homogeneous"].ctypes.data_as(capi.c_double_p)
        self._check(self.lib.pvio_hip_triangulate(self.ctx, C.byref(pb), C.byref(out)), "pvio_hip_triangulate")
        return res

    def triangulate_stats(self):
        """(max_sweeps, kernel_ms) of the last triangulate(): the most Jacobi sweeps a track took; the kernel's hipEvent time, recorded only with
        PVIO_HIP_TIMING set (else 0)"""
        sweeps, ms = C.c_int32(0), C.c_double(0.0)
        self._check(self.lib.pvio_hip_triangulate_stats(self.ctx, C.byref(sweeps), C.byref(ms)), "pvio_hip_triangulate_stats")
        return int(sweeps.value), float(ms.value)

    def plane_ransac(self, points, threshold=0.03, confidence=0.999, max_iterations=1000, seed=0):
        """pvio_hip_plane_ransac: the reference's 3-point plane RANSAC over points [n, 3] and the least-squares refit of the winner's inliers
        (include/pvio_hip.h; the defaults are PlaneExtractor::work's).  Returns a dict: n_inliers, iterations, best_iteration, refit_valid,
        inlier_mask [n] (uint8), normal [3], distance, refit_normal [3], refit_distance, reference_point [3].  The reference keeps the plane
        only if n_inliers > 30: that rule is the caller's."""
        points = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
        n = points.shape[0]
        mask = np.zeros(n, np.uint8)
        pb, out = capi.PlaneProblemC(), capi.PlaneResultC()
        pb.n_points, pb.max_iterations, pb.points = n, max_iterations, points.ctypes.data_as(capi.c_double_p)
        pb.threshold, pb.confidence, pb.seed = threshold, confidence, seed
        out.inlier_mask = mask.ctypes.data_as(capi.c_uint8_p)
        self._check(self.lib.pvio_hip_plane_ransac(self.ctx, C.byref(pb), C.byref(out)), "pvio_hip_plane_ransac")
        return dict(n_inliers=int(out.n_inliers), iterations=int(out.iterations), best_iteration=int(out.best_iteration), refit_valid=int(out.refit_valid),
                    inlier_mask=mask, normal=np.array(out.normal[:]), distance=float(out.distance), refit_normal=np.array(out.refit_normal[:]),
                    refit_distance=float(out.refit_distance), reference_point=np.array(out.reference_point[:]))

    def plane_ransac_stats(self):
        """(hypotheses_scored, kernel_ms [2]) of the last plane_ransac(): the hypotheses the device scored; the hipEvent times of
        k_plane_hypotheses and k_plane_refit, recorded only with PVIO_HIP_TIMING set (else 0)"""
        scored, ms = C.c_int32(0), np.zeros(2)
        self._check(self.lib.pvio_hip_plane_ransac_stats(self.ctx, C.byref(scored), ms.ctypes.data_as(capi.c_double_p)), "pvio_hip_plane_ransac_stats")
        return int(scored.value), ms

    def triangulate_window(self, problem, state, planes=False):
        """The landmarks of a flattened window (or, planes=True, its plane tracks) triangulated from the camera poses of `state`.  Views are
        the frames' cameras (Frame::get_pose(camera): q_c = q_b * q_cs, p_c = p_b + R(q_b) p_cs); a landmark's track is its anchor observation
        followed by its CSR observations, a plane track is its CSR list.  Adds inv_depth [T] = 1 / (R_a^T (point - p_a)).z in the camera of the
        track's first observation (Track::set_landmark_point), NaN where ok == 0, and returns the flattening next to the results."""
        view_P, R_wc, p_wc = window_views(problem, state)
        track_ptr, obs_view, obs_z = window_tracks(problem, planes)
        res = self.triangulate(view_P, track_ptr, obs_view, obs_z, homogeneous=True)
        first = obs_view[track_ptr[:-1]]
        depth = np.einsum("tk,tk->t", R_wc[first][:, :, 2], res["point"] - p_wc[first])
        with np.errstate(divide="ignore", invalid="ignore"):
            res["inv_depth"] = np.where(res["ok"] == 1, 1.0 / depth, np.nan)
        res.update(view_P=view_P, track_ptr=track_ptr, obs_view=obs_view, obs_z=obs_z)
        return res


def window_views(problem, state):
    """(view_P [N, 3, 4], R_wc [N, 3, 3], p_wc [N, 3]) of a window's cameras at `state`: P = [R_wc^T | -R_wc^T p_wc] (track.cpp:66-73)"""
    from .synth import qmat
    N = problem.n_frames
    view_P, R_wc, p_wc = np.zeros((N, 3, 4)), np.zeros((N, 3, 3)), np.zeros((N, 3))
    for f in range(N):
        R_b = qmat(state.frame_state[f, 0:4] / np.linalg.norm(state.frame_state[f, 0:4]))
        R_wc[f] = R_b @ qmat(problem.cam_extrinsic[f, 0:4] / np.linalg.norm(problem.cam_extrinsic[f, 0:4]))
        p_wc[f] = state.frame_state[f, 4:7] + R_b @ problem.cam_extrinsic[f, 4:7]
        view_P[f, :, :3] = R_wc[f].T
        view_P[f, :, 3] = -R_wc[f].T @ p_wc[f]
    return view_P, R_wc, p_wc


def window_tracks(problem, planes=False):
    """(track_ptr, obs_view, obs_z) of a window's landmarks -- anchor observation first -- or of its plane tracks"""
    if planes:
        return (np.ascontiguousarray(problem.plane_obs_ptr, np.int32), np.ascontiguousarray(problem.plane_obs_frame, np.int32),
                np.ascontiguousarray(problem.plane_obs_z, np.float64).reshape(-1, 2))
    M = problem.n_landmarks
    lm_ptr = np.asarray(problem.lm_obs_ptr, np.int64)
    track_ptr = (lm_ptr + np.arange(M + 1)).astype(np.int32)
    n = int(track_ptr[-1])
    obs_view, obs_z = np.zeros(n, np.int32), np.zeros((n, 2))
    anchor_at = track_ptr[:-1].astype(np.int64)
    is_anchor = np.zeros(n, bool)
    is_anchor[anchor_at] = True
    obs_view[anchor_at], obs_z[anchor_at] = problem.lm_anchor_frame[:M], np.asarray(problem.lm_anchor_z).reshape(-1, 2)[:M]
    obs_view[~is_anchor], obs_z[~is_anchor] = problem.obs_frame[:lm_ptr[M]], np.asarray(problem.obs_z).reshape(-1, 2)[:lm_ptr[M]]
    return track_ptr, obs_view, obs_z


class HipUndistort:
    """Device-resident fixed-point remap tables (pvio_hip_undistort_create): map_xy int16 [h][w][2], map_frac uint16 [h][w]."""

    def __init__(self, ctx, map_xy, map_frac):
        self.ctx = ctx
        xy = np.ascontiguousarray(map_xy, dtype=np.int16)
        fr = np.ascontiguousarray(map_frac, dtype=np.uint16)
        self.h, self.w = fr.shape
        assert xy.shape == (self.h, self.w, 2)
        self.handle = C.c_void_p()
        ctx._check(ctx.lib.pvio_hip_undistort_create(ctx.ctx, xy.ctypes.data_as(capi.c_int16_p), fr.ctypes.data_as(C.POINTER(C.c_uint16)),
                                                     self.w, self.h, C.byref(self.handle)), "pvio_hip_undistort_create")

    def release(self):
        if self.handle:
            self.ctx.lib.pvio_hip_undistort_release(self.ctx.ctx, self.handle)
            self.handle = C.c_void_p()


class HipImage:
    """Device-resident CLAHE'd pyramid (pvio_hip_image_create); mirrors OpenCvImage::preprocess.  With `undistort` the
    pixels are the distorted camera image and are remapped on the device first (the dataset readers' cv::undistort / remap)."""

    def __init__(self, ctx, pixels, clahe=True, undistort=None):
        self.ctx = ctx
        px = np.ascontiguousarray(pixels, dtype=np.uint8)
        self.h, self.w = px.shape
        self.handle = C.c_void_p()
        if undistort is not None:
            ctx._check(ctx.lib.pvio_hip_image_create_undistorted(ctx.ctx, undistort.handle, px.ctypes.data_as(capi.c_uint8_p), self.w, self.h, self.w,
                                                                 int(clahe), C.byref(self.handle)), "pvio_hip_image_create_undistorted")
            self.h, self.w = undistort.h, undistort.w
            return
        ctx._check(ctx.lib.pvio_hip_image_create(ctx.ctx, px.ctypes.data_as(capi.c_uint8_p), self.w, self.h, self.w, int(clahe), C.byref(self.handle)),
                   "pvio_hip_image_create")

    def level(self, l):
        w, h = C.c_int32(0), C.c_int32(0)
        self.ctx._check(self.ctx.lib.pvio_hip_image_download_level(self.ctx.ctx, self.handle, l, None, None, C.byref(w), C.byref(h)), "download_level")
        img = np.zeros((h.value, w.value), np.uint8)
        drv = np.zeros((h.value, w.value, 2), np.int16)
        self.ctx._check(self.ctx.lib.pvio_hip_image_download_level(self.ctx.ctx, self.handle, l, img.ctypes.data_as(capi.c_uint8_p),
                                                                 drv.ctypes.data_as(capi.c_int16_p), C.byref(w), C.byref(h)), "download_level")
        return img, drv

    def release(self):
        if self.handle:
            self.ctx.lib.pvio_hip_image_release(self.ctx.ctx, self.handle)
            self.handle = C.c_void_p()


def klt_track(ctx, prev, nxt, prev_xy, next_xy_init):
    """pvio_hip_klt_track: returns (next_xy, status, device_ms); mirrors OpenCvImage::track_keypoints up to the border kill."""
    p = np.ascontiguousarray(prev_xy, dtype=np.float32)
    q = np.array(next_xy_init, dtype=np.float32, order="C", copy=True)
    st = np.zeros(p.shape[0], np.uint8)
    ctx._check(ctx.lib.pvio_hip_klt_track(ctx.ctx, prev.handle, nxt.handle, p.shape[0], p.ctypes.data_as(capi.c_float_p), q.ctypes.data_as(capi.c_float_p),
                                          st.ctypes.data_as(capi.c_uint8_p)), "pvio_hip_klt_track")
    return q, st, ctx.lib.pvio_hip_klt_last_device_ms(ctx.ctx)


def fundamental_ransac(ctx, p_xy, q_xy, threshold=1.0, confidence=0.99, max_iterations=1000):
    """pvio_hip_fundamental_ransac: cv::findFundamentalMat(FM_RANSAC) with the hypotheses evaluated in batches on the device.
    -> (inlier count, mask uint8 [n], F 3x3, hypotheses evaluated)"""
    p = np.ascontiguousarray(p_xy, dtype=np.float32)
    q = np.ascontiguousarray(q_xy, dtype=np.float32)
    n = p.shape[0]
    mask, F, good = np.zeros(max(n, 1), np.uint8), np.zeros(9), C.c_int32(0)
    fp = C.POINTER(C.c_float)
    ctx._check(ctx.lib.pvio_hip_fundamental_ransac(ctx.ctx, n, p.ctypes.data_as(fp), q.ctypes.data_as(fp), float(threshold), float(confidence), int(max_iterations),
                                                   mask.ctypes.data_as(capi.c_uint8_p), F.ctypes.data_as(capi.c_double_p), C.byref(good)), "fundamental_ransac")
    return good.value, mask[:n], F.reshape(3, 3), int(ctx.lib.pvio_hip_ransac_last_hypotheses(ctx.ctx))


def preintegrate(t, w, a, t_end, bg, ba, noise, lib=None):
    """Product host-side pre-integration (pvio_preintegrate); same signature as oracle_py.preintegrate."""
    lib = lib or capi.load()
    f64 = lambda x: np.ascontiguousarray(x, dtype=np.float64)
    t, w, a, bg, ba = f64(t), f64(w), f64(a), f64(bg), f64(ba)
    delta, cov, U, jac = np.zeros(11), np.zeros(225), np.zeros(225), np.zeros(45)
    nz = capi.ImuNoiseC()
    for k in ("cov_w", "cov_a", "cov_bg", "cov_ba"):
        getattr(nz, k)[:] = list(np.asarray(noise[k], float).ravel())
    p = lambda x: x.ctypes.data_as(capi.c_double_p)
    rc = lib.pvio_preintegrate(len(t), p(t), p(w), p(a), float(t_end), p(bg), p(ba), C.byref(nz), p(delta), p(cov), p(U), p(jac))
    if rc != 0:
        raise HipError("pvio_preintegrate failed: %d" % rc)
    return delta, cov, U, jac


def detect_corners(ctx, img, max_corners=1000, quality=1.0e-3, min_distance=20.0, want_response_map=False):
    """pvio_hip_image_detect: Harris corners (goodFeaturesToTrack semantics) of a preprocessed HipImage.
    Returns (xy float32 [n, 2], response float32 [n]) and, on request, the response map."""
    xy = np.zeros((max_corners, 2), np.float32)
    resp = np.zeros(max_corners, np.float32)
    n = C.c_int32(0)
    ctx._check(ctx.lib.pvio_hip_image_detect(ctx.ctx, img.handle, max_corners, quality, min_distance, xy.ctypes.data_as(capi.c_float_p),
                                             resp.ctypes.data_as(capi.c_float_p), C.byref(n)), "pvio_hip_image_detect")
    if not want_response_map:
        return xy[:n.value].copy(), resp[:n.value].copy()
    rmap = np.zeros((img.h, img.w), np.float32)
    ctx._check(ctx.lib.pvio_hip_image_download_response(ctx.ctx, img.handle, rmap.ctypes.data_as(capi.c_float_p)), "pvio_hip_image_download_response")
    return xy[:n.value].copy(), resp[:n.value].copy(), rmap
