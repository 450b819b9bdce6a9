"""pvio_hip_ba_covariance (include/pvio_hip.h; kernels in pvio_amd/csrc/ba_cov.hip) against the references of cov_compare.py: in the fiber
emulator (tests/hipemu) with linearize_mode 1 and 2, on the GPU (-m gpu) with linearize_mode 0, 1 and 2.

Every window is taken at the oracle's solved state.  The tolerance of a case is computed from the reference alone (cov_compare.
reference_with_tolerance); a strict case also asserts that this tolerance is at most 1e-6.  Strict cases -- the smallest shapes at which
the kernels can still go wrong:
  vision_4x40_two_fixed     d = 6, fixed blocks, 12 free coordinates, no motion coordinate free
  vio_4x30                  P = 60: not a multiple of the 16 x 16 tile
  vio_plane_5x60, vio_rot_prior_5x40, vio_duplicate_blocks_6x70 (first reference only: the dense one does not model lm_multiplicity)
  vio_11x80                 P = 165, the largest reduced system the reference's window sizes produce
  vio_12x80 / vio_13x80     either side of k_cov_invert's LDS / global-memory boundary: ba_cov.h's kCovLdsMaxCoords = 192 free coordinates
                            (12 tile rows = 78 tiles = 159 744 bytes of LDS); 180 coordinates stay in LDS, 195 run on global memory
  vio_32x160                P = 480 = 15 PVIO_MAX_FRAMES (GPU only)
  vio_last_frame_without_information   no IMU factor into the last frame, prior over frames 0..N-2: its velocity and biases have zero rows"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ba_compare
import cov_compare
from pvio_amd import capi
from pvio_amd.solver import HipContext, HipError

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu")
LDS_MAX_COORDS = 192  # kCovLdsMaxCoords of pvio_amd/csrc/ba_cov.h


def _fix(*frames):
    def edit(pb):
        for f in frames:
            pb.frame_fixed[f] = 1
    return edit


def _no_last_imu_factor(pb):
    pb.preint_valid[pb.n_frames - 1] = 0
    assert list(pb.prior_frames) == list(range(pb.n_frames - 1))


def _vio(n, m, **kw):
    return dict(n_frames=n, n_landmarks=m, use_inertial=True, **kw)


STRICT = {
    "vision_4x40_two_fixed": dict(kw=dict(n_frames=4, n_landmarks=40), edit=_fix(0, 1)),
    "vio_4x30": dict(kw=_vio(4, 30), prior="regular"),
    "vio_plane_5x60": dict(kw=ba_compare.CASES["vio_plane"], prior="regular"),
    "vio_rot_prior_5x40": dict(kw=ba_compare.CASES["vio_rot_prior"], prior="regular"),
    "vio_duplicate_blocks_6x70": dict(kw=ba_compare.CASES["vio_duplicate_blocks"], prior="regular"),
    "vio_11x80": dict(kw=_vio(11, 80, visibility=6), prior="regular"),
    "vio_12x80": dict(kw=_vio(12, 80, visibility=6), prior="regular"),
    "vio_13x80": dict(kw=_vio(13, 80, visibility=6), prior="regular"),
    "vio_32x160": dict(kw=_vio(32, 160, visibility=8), prior="regular"),
    "vio_last_frame_without_information": dict(kw=_vio(5, 40, visibility=4), prior="regular", edit=_no_last_imu_factor),
}
OTHER = {
    "gauge_prior_vio_4x30": dict(kw=_vio(4, 30)),                       # synth's 1e15 prior: the scaling path, kappa ~ 1e10
    "unobservable_vision_4x40": dict(kw=dict(n_frames=4, n_landmarks=40)),  # only frame 0 fixed: the scale is free
    "unobservable_vio_4x30_no_prior": dict(kw=_vio(4, 30), prior="empty"),
}
GPU_ONLY = {"vio_32x160"}
NO_DENSE_REFERENCE = {"vio_duplicate_blocks_6x70"}

_cache = {}


def window(oracle, name):
    """(problem, state, reference) of a case, computed once per session and shared, never written"""
    if name not in _cache:
        spec = STRICT.get(name) or OTHER[name]
        pb, st = cov_compare.solved(oracle, prior=spec.get("prior"), edit=spec.get("edit"), **spec["kw"])
        _cache[name] = (pb, st, cov_compare.reference_with_tolerance(oracle, pb, st))
    return _cache[name]


def run_strict(ctxs, oracle, name):
    pb, st, ref = window(oracle, name)
    if name == "vision_4x40_two_fixed":
        assert ref["n_free"] == 12
    if name == "vio_12x80":
        assert ref["n_free"] == 180 <= LDS_MAX_COORDS
    if name == "vio_13x80":
        assert ref["n_free"] == 195 > LDS_MAX_COORDS
    if name == "vio_last_frame_without_information":
        last = 15 * (pb.n_frames - 1)
        assert not ref["free"][last + 6:last + 15].any() and ref["free"][last:last + 6].all() and ref["n_free"] == 15 * pb.n_frames - 9
    out = {}
    for mode, ctx in ctxs.items():
        try:
            out[mode] = cov_compare.check(ctx, pb, st, ref, strict=True)
        except AssertionError as e:
            raise AssertionError("linearize_mode %d: %s" % (mode, e)) from None
    # the two landmark roles differ in the order of their sums only
    r1, r2 = out[1][0], out[2][0]
    e_cov, e_lm = cov_compare.errors(r2["joint_cov"], r2["lm_var"], dict(ref, joint_cov=r1["joint_cov"], lm_var=r1["lm_var"]))
    assert e_cov <= ref["tol"] and e_lm <= ref["tol"], (e_cov, e_lm, ref["tol"])
    return {m: o[1] for m, o in out.items()}


def run_gauge_prior(ctx, oracle):
    pb, st, ref = window(oracle, "gauge_prior_vio_4x30")
    assert ref["kappa"] > 1e8 and ref["min_pivot"] > 1e3 * cov_compare.MIN_PIVOT, (ref["kappa"], ref["min_pivot"])
    return cov_compare.check(ctx, pb, st, ref, strict=False)[1]  # finite, symmetric, positive definite, within its own (loose) tolerance


def run_unobservable(ctx, oracle, name):
    pb, st, ref = window(oracle, name)
    assert ref["positive_definite"] == 0 and max(ref["pivots_by_order"]) <= cov_compare.MIN_PIVOT, ref["pivots_by_order"]
    N, M = pb.n_frames, pb.n_landmarks
    sentinel = -12345.0
    into = dict(frame_cov=np.full((N, 15, 15), sentinel), joint_cov=np.full((15 * N, 15 * N), sentinel), lm_var=np.full(M, sentinel),
                coord_free=np.full(15 * N, 77, np.uint8))
    res = ctx.covariance(pb, st, joint=True, landmarks=True, into=into)  # returns PVIO_OK: HipContext raises on anything else
    assert res["positive_definite"] == 0
    assert 0 <= res["first_bad_coord"] < 15 * N and ref["free"][res["first_bad_coord"]], res["first_bad_coord"]
    assert (into["frame_cov"] == sentinel).all() and (into["joint_cov"] == sentinel).all() and (into["lm_var"] == sentinel).all()
    assert (into["coord_free"] == 77).all()
    return dict(first_bad_coord=res["first_bad_coord"], reference_first_bad_coord=ref["first_bad_coord"], reference_min_pivots=ref["pivots_by_order"])


def run_repeat_and_residue(ctx, oracle, name="vio_rot_prior_5x40"):
    pb, st, _ = window(oracle, name)
    st0, sm0 = ctx.solve(pb)
    a = ctx.covariance(pb, st, joint=True, landmarks=True)
    b = ctx.covariance(pb, st, joint=True, landmarks=True)
    for k in ("frame_cov", "joint_cov", "lm_var", "coord_free"):
        assert (a[k] == b[k]).all(), "%s differs between two calls on the same input" % k
    assert a["positive_definite"] == b["positive_definite"] == 1
    st1, sm1 = ctx.solve(pb)
    assert (st0.frame_state == st1.frame_state).all() and (st0.lm_inv_depth == st1.lm_inv_depth).all()
    t0, t1 = sm0.trace(), sm1.trace()
    assert len(t0) == len(t1) and all(x == y for x, y in zip(t0, t1)), "a covariance call leaves a residue in the next solve"
    assert sm0.final_cost == sm1.final_cost and sm0.num_iterations == sm1.num_iterations


def run_argument_errors(ctx, oracle):
    pb, st, _ = window(oracle, "vio_4x30")
    pc, sc = pb.as_c(), st.as_c()
    assert ctx.lib.pvio_hip_ba_covariance(ctx.ctx, C.byref(pc), C.byref(sc), None) == -1  # PVIO_ERR_INVALID_ARGUMENT
    cv = capi.BACovarianceC()
    jc = np.zeros((15 * pb.n_frames, 15 * pb.n_frames))
    cv.joint_cov = jc.ctypes.data_as(capi.c_double_p)
    assert ctx.lib.pvio_hip_ba_covariance(ctx.ctx, C.byref(pc), C.byref(sc), C.byref(cv)) == -1  # frame_cov is not optional
    assert (jc == 0).all()
    bad = ba_compare.make(oracle, n_frames=4, n_landmarks=30, use_inertial=True)
    bad.obs_frame = bad.obs_frame.copy()
    bad.obs_frame[0] = bad.n_frames  # a window upload() rejects is rejected with the same code
    with pytest.raises(HipError) as e_up:
        ctx.upload(bad)
    with pytest.raises(HipError) as e_cov:
        ctx.covariance(bad, st)
    code = lambda e: str(e.value).split("status")[1].split()[0]
    assert code(e_up) == code(e_cov)


# ---- the two references against each other (no kernels) ----

@pytest.mark.parametrize("name", sorted(set(STRICT) - NO_DENSE_REFERENCE))
def test_references_agree(oracle, name):
    pb, st, ref = window(oracle, name)
    assert ref["positive_definite"] == 1 and ref["tol"] <= 1e-6, ref.get("tol")
    dense = cov_compare.reference_dense(oracle, pb, st)
    nf = ~ref["free"]
    assert (dense["joint_cov"][nf] == 0).all()
    e_cov, e_lm = cov_compare.errors(dense["joint_cov"], dense["lm_var"], ref)
    print(name, "kappa %.3g bound %.3g spread %.3g; dense reference: cov %.3g lm_var %.3g" % (ref["kappa"], ref["bound"], ref["spread"], e_cov, e_lm))
    assert e_cov <= ref["tol"] and e_lm <= ref["tol"], (e_cov, e_lm, ref["tol"])


def test_reference_pivot_rule_separates_the_windows(oracle):
    """singular windows sit at rounding level, the worst legitimate window four decades above PVIO_COV_MIN_PIVOT"""
    for name in ("unobservable_vision_4x40", "unobservable_vio_4x30_no_prior"):
        assert max(window(oracle, name)[2]["pivots_by_order"]) <= 1e-4 * cov_compare.MIN_PIVOT
    assert min(window(oracle, "gauge_prior_vio_4x30")[2]["pivots_by_order"]) >= 1e3 * cov_compare.MIN_PIVOT


# ---- emulator ----

@pytest.fixture(scope="module")
def emu_lib():
    subprocess.check_call(["make", "-s", "-C", EMU_DIR, "libpvio_hipemu.so"])
    return capi.load(os.path.join(EMU_DIR, "libpvio_hipemu.so"))


@pytest.fixture(scope="module")
def emu_roles(emu_lib):
    ctxs = {m: HipContext(lib=emu_lib, use_graph=True, linearize_mode=m) for m in (1, 2)}
    yield ctxs
    for c in ctxs.values():
        c.close()


@pytest.mark.parametrize("name", sorted(set(STRICT) - GPU_ONLY))
def test_emulated_covariance(emu_roles, oracle, name):
    print(name, run_strict(emu_roles, oracle, name))


def test_emulated_covariance_gauge_prior(emu_roles, oracle):
    for ctx in emu_roles.values():
        print(run_gauge_prior(ctx, oracle))


@pytest.mark.parametrize("name", ["unobservable_vision_4x40", "unobservable_vio_4x30_no_prior"])
def test_emulated_covariance_unobservable(emu_roles, oracle, name):
    for ctx in emu_roles.values():
        print(name, run_unobservable(ctx, oracle, name))


def test_emulated_covariance_repeats_and_leaves_no_residue(emu_roles, oracle):
    for ctx in emu_roles.values():
        run_repeat_and_residue(ctx, oracle)


def test_emulated_covariance_argument_errors(emu_roles, emu_lib, oracle):
    run_argument_errors(emu_roles[1], oracle)
    pb, st, _ = window(oracle, "vio_4x30")
    sharded = HipContext(lib=emu_lib, force_sharded=True)
    try:
        with pytest.raises(HipError, match=r"status -5 .*sharded"):  # PVIO_ERR_UNSUPPORTED
            sharded.covariance(pb, st)
    finally:
        sharded.close()


# ---- GPU ----

@pytest.fixture(scope="module")
def gpu_roles():
    ctxs = {m: HipContext(device=0, use_graph=True, linearize_mode=m) for m in (0, 1, 2)}  # raises without a GPU: no fallback
    yield ctxs
    for c in ctxs.values():
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(STRICT))
def test_gpu_covariance(gpu_roles, oracle, name):
    print(name, run_strict(gpu_roles, oracle, name))


@pytest.mark.gpu
def test_gpu_covariance_gauge_prior(gpu_roles, oracle):
    for ctx in gpu_roles.values():
        print(run_gauge_prior(ctx, oracle))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["unobservable_vision_4x40", "unobservable_vio_4x30_no_prior"])
def test_gpu_covariance_unobservable(gpu_roles, oracle, name):
    for ctx in gpu_roles.values():
        print(name, run_unobservable(ctx, oracle, name))


@pytest.mark.gpu
def test_gpu_covariance_repeats_and_leaves_no_residue(gpu_roles, oracle):
    for ctx in gpu_roles.values():
        run_repeat_and_residue(ctx, oracle)
    run_repeat_and_residue(gpu_roles[0], oracle, "vio_13x80")  # the global-memory form of k_cov_invert


@pytest.mark.gpu
def test_gpu_covariance_argument_errors(gpu_roles, oracle):
    run_argument_errors(gpu_roles[0], oracle)
    pb, st, _ = window(oracle, "vio_4x30")
    sharded = HipContext(device=0, force_sharded=True)
    try:
        with pytest.raises(HipError, match=r"status -5 .*sharded"):
            sharded.covariance(pb, st)
    finally:
        sharded.close()
