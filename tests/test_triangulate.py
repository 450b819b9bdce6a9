"""pvio_hip_triangulate (include/pvio_hip.h; kernel in pvio_amd/csrc/ba_triangulate.hip) against the numpy reference of tri_compare.py: in the
fiber emulator (tests/hipemu) and on the GPU (-m gpu).  The tolerance of every track is computed from the reference alone (tri_compare's
docstring); `ok` must be identical for every track of every case.

Strict cases -- views from synth's arc and calibration, points 2-8 m in front of their cameras, synth's pixel noise, tol_q <= 1e-9:
  K = 2 (the system is square), 3 (smallest multi-view track), 11 (the reference's window), 16 / 17 (either side of the 32- / 64-lane group),
  32 (every lane holds a row); T = 1, 5 (a partly filled block), 257 (more than one block);
  a mixed call with K in {1, 2, 11, 16, 17, 32}: 64-lane groups, a one-observation track;  T = 0;  observations in descending order.
Then: noise-free points, the gates (60 m, 150 m, behind a camera, NaN), low parallax (its own, larger tolerance), a rank-deficient track, sweeps
below the kernel's bound, repeatability and no residue in a resident window, the argument errors, triangulate_window on a solved plane window."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ba_compare
import cov_compare
import tri_compare
from pvio_amd import BASummary, capi, solver
from pvio_amd.solver import HipContext

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu")
STRICT_K = (2, 3, 11, 16, 17, 32)
STRICT_T = (1, 5, 257)

_cache = {}


def strict_case(K, T):
    """(input, reference) of a strict case, computed once per session and shared, never written"""
    if (K, T) not in _cache:
        inp = tri_compare.make_tracks([K] * T, seed=1000 * K + T)
        _cache[(K, T)] = (inp, tri_compare.reference(inp["view_P"], inp["track_ptr"], inp["obs_view"], inp["obs_z"]))
    return _cache[(K, T)]


def run_strict(ctx, K, T):
    inp, ref = strict_case(K, T)
    _, fig = tri_compare.check(ctx, inp, ref, strict=True, what="K=%d T=%d" % (K, T))
    print("K=%d T=%d max_sweeps %d" % (K, T, fig["max_sweeps"]))
    assert 1 <= fig["max_sweeps"] < tri_compare.MAX_SWEEPS
    return fig


def run_mixed(ctx):
    inp = tri_compare.make_tracks([1, 2, 11, 16, 17, 32] * 3, seed=77)
    res, fig = tri_compare.check(ctx, inp, strict=True, what="mixed")
    assert (res["ok"][0::6] == 0).all() and (res["score"][0::6] == np.inf).all()  # the one-observation tracks
    assert 1 <= fig["max_sweeps"] < tri_compare.MAX_SWEEPS
    return fig


def run_empty(ctx):
    view_P, _, _ = tri_compare.arc_views()
    res = ctx.triangulate(view_P, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros((0, 2)), homogeneous=True)  # PVIO_OK: HipContext raises on anything else
    assert res["point"].shape == (0, 3) and res["ok"].shape == (0,)
    assert ctx.triangulate_stats() == (0, 0.0)
    # NULL inputs are fine when there is no track
    pb, out = capi.TriProblemC(), capi.TriResultC()
    pb.n_views, pb.n_tracks = 1, 0
    point, ok = np.zeros(3), np.zeros(1, np.uint8)
    out.point, out.ok = point.ctypes.data_as(capi.c_double_p), ok.ctypes.data_as(capi.c_uint8_p)
    assert ctx.lib.pvio_hip_triangulate(ctx.ctx, C.byref(pb), C.byref(out)) == 0


def run_descending(ctx):
    asc = tri_compare.make_tracks([11] * 5, seed=5)
    desc = tri_compare.reversed_inside_tracks(asc)
    assert (desc["obs_view"][:11] == asc["obs_view"][:11][::-1]).all() and (np.diff(desc["obs_view"][:11]) < 0).all()
    ref = tri_compare.reference(asc["view_P"], asc["track_ptr"], asc["obs_view"], asc["obs_z"])
    a, _ = tri_compare.check(ctx, asc, ref, what="ascending")
    d, _ = tri_compare.check(ctx, desc, ref, what="descending")  # against the reference of the ascending rows
    assert (a["ok"] == d["ok"]).all()
    assert (np.linalg.norm(a["homogeneous"] - d["homogeneous"], axis=1) <= ref["tol_q"]).all()
    assert (np.linalg.norm(a["point"] - d["point"], axis=1) <= ref["tol_point"]).all()


def run_noise_free(ctx):
    for K in (2, 11, 32):
        inp = tri_compare.make_tracks([K] * 5, seed=300 + K, noise=False)
        ref = tri_compare.reference(inp["view_P"], inp["track_ptr"], inp["obs_view"], inp["obs_z"])
        res, _ = tri_compare.check(ctx, inp, ref, strict=True, what="noise-free K=%d" % K)
        assert (res["ok"] == 1).all()
        e = np.linalg.norm(res["point"] - inp["truth"], axis=1)
        print("noise-free K=%d: |point - truth| / tol_point %.3g" % (K, (e / ref["tol_point"]).max()))
        assert (e <= ref["tol_point"]).all(), (e, ref["tol_point"])


def gates_input():
    """two views with parallel axes, 10 m apart ((8, 0, 6): sideways and along the axis, so that a point can be behind one of them only)"""
    R = np.stack([np.eye(3), np.eye(3)])
    p = np.array([[0.0, 0.0, 0.0], [8.0, 0.0, 6.0]])
    view_P = tri_compare.views_from_poses(R, p)
    points = np.array([[4.0, 0.0, 60.0], [4.0, 0.0, 150.0], [4.0, 1.0, 3.0], [4.0, 0.0, 60.0], [3.0, -2.0, 30.0]])
    z = np.concatenate([tri_compare.project(view_P, np.array([0, 1]), x)[0] for x in points])
    z[2 * 3 + 1, 0] = np.nan  # track 3: NaN in its second observation
    return dict(view_P=view_P, track_ptr=np.arange(0, 11, 2).astype(np.int32), obs_view=np.tile(np.array([0, 1], np.int32), 5), obs_z=z), points


def run_gates(ctx):
    inp, points = gates_input()
    ref = tri_compare.reference(inp["view_P"], inp["track_ptr"], inp["obs_view"], inp["obs_z"])
    assert list(ref["ok"]) == [1, 0, 0, 0, 1] and list(ref["finite"]) == [True, True, True, False, True]
    res, _ = tri_compare.check(ctx, inp, ref, strict=False, what="gates")  # every other track of the call within its tolerance
    assert list(res["ok"]) == [1, 0, 0, 0, 1]
    assert abs(np.linalg.norm(res["point"][2]) - 1.0) <= 4 * tri_compare.EPS  # behind the second camera: the direction, of unit length
    assert np.linalg.norm(res["point"][0] - points[0]) <= ref["tol_point"][0] and np.linalg.norm(res["point"][4] - points[4]) <= ref["tol_point"][4]


def run_low_parallax(ctx):
    """two adjacent views (0.23 m apart), points at 40 m, exact projections: with pixel noise the reference's own depth would land on either side
    of the gates by chance"""
    view_P, R_wc, p_wc = tri_compare.arc_views()
    rng = np.random.RandomState(40)
    T = 5
    pts = p_wc[0] + (R_wc[0] @ np.stack([rng.uniform(-8, 8, T), rng.uniform(-5, 5, T), np.full(T, 40.0)])).T
    z = np.concatenate([tri_compare.project(view_P, np.array([0, 1]), x)[0] for x in pts])
    inp = dict(view_P=view_P, track_ptr=np.arange(0, 2 * T + 1, 2).astype(np.int32), obs_view=np.tile(np.array([0, 1], np.int32), T), obs_z=z)
    _, fig = tri_compare.check(ctx, inp, strict=False, what="low parallax")
    return fig


def run_rank_deficient(ctx):
    """every view of the track is the same camera: rank <= 3 with two small singular values -- a degenerate input, not a fault"""
    good, _ = strict_case(11, 5)
    inp = dict(good, obs_view=np.full_like(good["obs_view"], 3))
    res = tri_compare.call(ctx, inp)  # PVIO_OK: HipContext raises on anything else
    sweeps = ctx.triangulate_stats()[0]
    print("rank-deficient: max_sweeps %d, ok %s" % (sweeps, res["ok"]))
    assert 1 <= sweeps <= tri_compare.MAX_SWEEPS
    run_strict(ctx, 11, 5)


def run_repeat_and_residue(ctx, oracle):
    inp, _ = strict_case(17, 5)
    a, b = tri_compare.call(ctx, inp), tri_compare.call(ctx, inp)
    for k in ("point", "ok", "score", "homogeneous"):
        assert (a[k] == b[k]).all() or (k == "score" and np.array_equal(a[k], b[k], equal_nan=True)), "%s differs between two calls on the same input" % k
    pb = ba_compare.make(oracle, **ba_compare.CASES["vio_rot_prior"])
    st = ctx.upload(pb)
    sm0 = ctx.solve_resident(BASummary(pb))
    st0 = ctx.download(solver.BAState(pb))
    tri_compare.call(ctx, inp)
    sm1 = ctx.solve_resident(BASummary(pb))
    st1 = ctx.download(solver.BAState(pb))
    assert (st0.frame_state == st1.frame_state).all() and (st0.lm_inv_depth == st1.lm_inv_depth).all()
    t0, t1 = sm0.trace(), sm1.trace()
    assert len(t0) == len(t1) and all(x == y for x, y in zip(t0, t1)), "a triangulation call leaves a residue in the next resident solve"
    assert sm0.final_cost == sm1.final_cost and sm0.initial_cost == sm1.initial_cost and sm0.num_iterations == sm1.num_iterations


def run_argument_errors(ctx):
    inp, _ = strict_case(3, 5)
    T = 5
    sentinel = -12345.0
    arrays = dict(point=np.full((T, 3), sentinel), ok=np.full(T, 77, np.uint8), score=np.full(T, sentinel), homogeneous=np.full((T, 4), sentinel))

    def rc(edit_pb=None, edit_out=None, expect_untouched=True, **replace):
        a = dict(inp, **replace)
        keep = [np.ascontiguousarray(a["view_P"], float), np.ascontiguousarray(a["track_ptr"], np.int32), np.ascontiguousarray(a["obs_view"], np.int32),
                np.ascontiguousarray(a["obs_z"], float)]
        pb, out = capi.TriProblemC(), capi.TriResultC()
        pb.n_views, pb.n_tracks = keep[0].reshape(-1, 12).shape[0], len(keep[1]) - 1
        pb.view_P, pb.obs_z = keep[0].ctypes.data_as(capi.c_double_p), keep[3].ctypes.data_as(capi.c_double_p)
        pb.track_ptr, pb.obs_view = keep[1].ctypes.data_as(capi.c_int32_p), keep[2].ctypes.data_as(capi.c_int32_p)
        out.point, out.ok = arrays["point"].ctypes.data_as(capi.c_double_p), arrays["ok"].ctypes.data_as(capi.c_uint8_p)
        out.score, out.homogeneous = arrays["score"].ctypes.data_as(capi.c_double_p), arrays["homogeneous"].ctypes.data_as(capi.c_double_p)
        if edit_pb:
            edit_pb(pb)
        if edit_out:
            edit_out(out)
        code = ctx.lib.pvio_hip_triangulate(ctx.ctx, C.byref(pb), C.byref(out))
        if expect_untouched:
            assert (arrays["point"] == sentinel).all() and (arrays["ok"] == 77).all() and (arrays["score"] == sentinel).all() and (arrays["homogeneous"] == sentinel).all()
        return code

    INVALID = -1  # PVIO_ERR_INVALID_ARGUMENT
    assert rc(edit_out=lambda o: setattr(o, "point", None)) == INVALID
    assert rc(edit_out=lambda o: setattr(o, "ok", None)) == INVALID
    for field in ("view_P", "track_ptr", "obs_view", "obs_z"):
        assert rc(edit_pb=lambda p, f=field: setattr(p, f, None)) == INVALID, field
    assert ctx.lib.pvio_hip_triangulate(ctx.ctx, None, None) == INVALID
    ptr = inp["track_ptr"].copy()
    ptr[0] = 1
    assert rc(track_ptr=ptr) == INVALID  # does not start at 0
    ptr = inp["track_ptr"].copy()
    ptr[2] = ptr[1] - 1
    assert rc(track_ptr=ptr) == INVALID  # decreases
    long_ptr = np.array([0, tri_compare.MAX_OBS + 1], np.int32)
    assert rc(track_ptr=long_ptr, obs_view=np.zeros(33, np.int32), obs_z=np.zeros((33, 2))) == INVALID  # 33 observations
    for v in (-1, tri_compare.MAX_OBS):
        ov = inp["obs_view"].copy()
        ov[7] = v
        assert rc(obs_view=ov) == INVALID  # outside [0, V)
    assert rc(edit_pb=lambda p: setattr(p, "n_views", 0)) == INVALID
    # ... and the same arguments unedited are accepted and written
    assert rc(expect_untouched=False) == 0 and (arrays["ok"] != 77).all() and (arrays["point"] != sentinel).all()


def run_window(ctx, oracle):
    if "window" not in _cache:
        _cache["window"] = cov_compare.solved(oracle, **ba_compare.CASES["vio_plane"])
    pb, st = _cache["window"]
    _, R_wc, p_wc = solver.window_views(pb, st)
    for planes in (False, True):
        res = ctx.triangulate_window(pb, st, planes=planes)
        T = pb.n_plane_factors if planes else pb.n_landmarks
        assert T > 0 and res["point"].shape == (T, 3)
        first = res["obs_view"][res["track_ptr"][:-1]]
        if not planes:  # the anchor observation leads, the CSR observations follow
            assert (first == pb.lm_anchor_frame).all() and (res["obs_z"][res["track_ptr"][:-1]] == pb.lm_anchor_z).all()
            assert (np.diff(res["track_ptr"]) == np.diff(pb.lm_obs_ptr) + 1).all()
            assert (res["obs_view"][1:res["track_ptr"][1]] == pb.obs_frame[:pb.lm_obs_ptr[1]]).all()
        ref = tri_compare.reference(res["view_P"], res["track_ptr"], res["obs_view"], res["obs_z"])
        tri_compare.compare(res, ref, strict=False, what="window planes=%s" % planes)
        # inv_depth = 1 / depth, depth = r_3 . (point - p_a) with |r_3| = 1: |d depth| <= tol_point, |d (1 / depth)| <= tol_point / depth^2 to first
        # order (the factor 2 covers the second), plus the rounding of the evaluation itself
        depth = np.einsum("tk,tk->t", R_wc[first][:, :, 2], ref["point"] - p_wc[first])
        ok = ref["ok"] == 1
        assert ok.sum() >= T // 2, "most tracks of a solved window triangulate"
        assert np.isnan(res["inv_depth"][~ok]).all()
        tol = 2 * ref["tol_point"][ok] / depth[ok] ** 2 + 16 * tri_compare.EPS / np.abs(depth[ok])
        err = np.abs(res["inv_depth"][ok] - 1.0 / depth[ok])
        print("window planes=%s: %d tracks, %d ok, inv_depth error / tol %.3g" % (planes, T, ok.sum(), (err / tol).max()))
        assert (err <= tol).all()
        if not planes:  # sanity of the whole chain: the solved window's own inverse depths are what its observations triangulate to, roughly
            assert np.median(np.abs(res["inv_depth"][ok] - st.lm_inv_depth[ok])) < 0.05


# ---- the reference alone (no kernels) ----

@pytest.mark.parametrize("K", STRICT_K)
def test_reference_tolerance_of_the_strict_cases(K):
    """tol_q of the construction: between 1e-14 and a few 1e-12, spread far below the bound"""
    _, ref = strict_case(K, 257)
    print(K, "tol_q %.3g .. %.3g, spread <= %.3g, margin >= %.3g" % (ref["tol_q"].min(), ref["tol_q"].max(), ref["spread"].max(), ref["margin"].min()))
    assert (ref["tol_q"] <= 1e-9).all() and (ref["tol_q"] >= 16 * tri_compare.EPS).all()
    assert (ref["ok"] == 1).all() and (ref["margin"] >= tri_compare.GATE_MARGIN).all()


# ---- emulator ----

@pytest.fixture(scope="module")
def emu_ctx():
    subprocess.check_call(["make", "-s", "-C", EMU_DIR, "libpvio_hipemu.so"])
    ctx = HipContext(lib=capi.load(os.path.join(EMU_DIR, "libpvio_hipemu.so")), use_graph=True)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("T", STRICT_T)
@pytest.mark.parametrize("K", STRICT_K)
def test_emulated_triangulation(emu_ctx, K, T):
    run_strict(emu_ctx, K, T)


def test_emulated_triangulation_mixed_lengths(emu_ctx):
    run_mixed(emu_ctx)


def test_emulated_triangulation_without_tracks(emu_ctx):
    run_empty(emu_ctx)


def test_emulated_triangulation_descending_views(emu_ctx):
    run_descending(emu_ctx)


def test_emulated_triangulation_noise_free(emu_ctx):
    run_noise_free(emu_ctx)


def test_emulated_triangulation_gates(emu_ctx):
    run_gates(emu_ctx)


def test_emulated_triangulation_low_parallax(emu_ctx):
    run_low_parallax(emu_ctx)


def test_emulated_triangulation_rank_deficient(emu_ctx):
    run_rank_deficient(emu_ctx)


def test_emulated_triangulation_repeats_and_leaves_no_residue(emu_ctx, oracle):
    run_repeat_and_residue(emu_ctx, oracle)


def test_emulated_triangulation_argument_errors(emu_ctx):
    run_argument_errors(emu_ctx)


def test_emulated_triangulate_window(emu_ctx, oracle):
    run_window(emu_ctx, oracle)


# ---- GPU ----

@pytest.fixture(scope="module")
def gpu_ctx():
    ctx = HipContext(device=0, use_graph=True)  # raises without a GPU: no fallback
    yield ctx
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("T", STRICT_T)
@pytest.mark.parametrize("K", STRICT_K)
def test_gpu_triangulation(gpu_ctx, K, T):
    run_strict(gpu_ctx, K, T)


@pytest.mark.gpu
def test_gpu_triangulation_3000_tracks_of_11_views(gpu_ctx):
    run_strict(gpu_ctx, 11, 3000)


@pytest.mark.gpu
def test_gpu_triangulation_mixed_lengths(gpu_ctx):
    run_mixed(gpu_ctx)


@pytest.mark.gpu
def test_gpu_triangulation_without_tracks(gpu_ctx):
    run_empty(gpu_ctx)


@pytest.mark.gpu
def test_gpu_triangulation_descending_views(gpu_ctx):
    run_descending(gpu_ctx)


@pytest.mark.gpu
def test_gpu_triangulation_noise_free(gpu_ctx):
    run_noise_free(gpu_ctx)


@pytest.mark.gpu
def test_gpu_triangulation_gates(gpu_ctx):
    run_gates(gpu_ctx)


@pytest.mark.gpu
def test_gpu_triangulation_low_parallax(gpu_ctx):
    run_low_parallax(gpu_ctx)


@pytest.mark.gpu
def test_gpu_triangulation_rank_deficient(gpu_ctx):
    run_rank_deficient(gpu_ctx)


@pytest.mark.gpu
def test_gpu_triangulation_repeats_and_leaves_no_residue(gpu_ctx, oracle):
    run_repeat_and_residue(gpu_ctx, oracle)


@pytest.mark.gpu
def test_gpu_triangulation_argument_errors(gpu_ctx):
    run_argument_errors(gpu_ctx)


@pytest.mark.gpu
def test_gpu_triangulate_window(gpu_ctx, oracle):
    run_window(gpu_ctx, oracle)
