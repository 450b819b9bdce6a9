"""Bundle adjustment on windows make_window never produces (tests/window_variants.py): the C ABI -- in the fiber emulator with linearize_mode 1
and 2, on the GPU (-m gpu) with 0, 1 and 2 -- against the oracle.

  A  per-frame calibration: its own camera extrinsic, sqrt_inv_cov, intrinsics and IMU extrinsic in every frame, one field at a time and all
     together: solve (every iterate, trace, lm_quality, lm_valid), marginalize_frame for victim 0 and a middle victim in both landmark roles,
     the roles against each other, the mean reprojection error
  B  (oracle only) the variants discriminate: with frame 0's value put into every frame the oracle's own result moves by more than
     1000 x STATE_TOL -- a kernel that ignored the frame index would miss A by as much
  C  moved gauges: a world yaw about gravity, a translation of up to 1e5 m, negated quaternions; against the oracle on the moved window and
     against the carried-over solution of the unmoved one, within 4 x the oracle's own deviation between "solve moved" and "move solved"
  D  rotation residuals on each side of every series switch of so3_right_jacobian and of the branches of q_logmap (pv_math.h), in the
     marginalization prior and the rotation prior, with both signs of the reference quaternion"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ba_compare
import marg_compare
import window_variants as wv
from ba_compare import STATE_TOL
from pvio_amd import BAState, BASummary, capi
from pvio_amd.solver import HipContext

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu")
SEED = 2024

# name -> (make_window arguments, marg_compare's regular prior from the start)
BASE = {
    "vision": (dict(n_frames=5, n_landmarks=40, visibility=4), False),
    "vio_prior": (dict(n_frames=6, n_landmarks=60, use_inertial=True, visibility=4), True),
    "vio_plane": (ba_compare.CASES["vio_plane"], False),
    "vio_rot_prior": (ba_compare.CASES["vio_rot_prior"], False),
    "vio_duplicate_blocks": (ba_compare.CASES["vio_duplicate_blocks"], False),
    "vio_11_frames": (ba_compare.CASES["vio_11_frames_lds_limit"], False),   # k_dense with the matrix in LDS
    "vio_13_frames": (ba_compare.CASES["vio_13_frames_global_matrix"], False),  # ... and in HBM
}
_cache = {}


def _oracle_solve(oracle, pb):
    st, sm = BAState(pb), BASummary(pb)
    oracle.solve(pb, st, sm)
    return st, sm


def base_window(oracle, name):
    """never edited: every rewrite returns a new problem"""
    if name not in _cache:
        kw, regular = BASE[name]
        pb = ba_compare.make(oracle, **kw)
        if regular:
            marg_compare.set_regular_prior(pb, pb.prior_frames)
        _cache[name] = pb
    return _cache[name]


def _fields_of(case):
    return wv.FIELDS if case == "all" else (case,)


def variant_window(oracle, name, case):
    key = (name, case)
    if key not in _cache:
        pb = base_window(oracle, name)
        fields = [f for f in _fields_of(case) if f != "imu" or pb.use_inertial]
        _cache[key] = wv.per_frame_calibration(pb, oracle, fields, SEED)
    return _cache[key]


A_CASES = ["%s-%s" % (n, c) for n in BASE for c in ("cam", "W", "intr", "imu", "all") if c != "imu" or BASE[n][0].get("use_inertial")]
# the 11- and 13-frame windows take 20-40 s per case in the fiber emulator (five solves and eight marginalizations each): GPU only
GPU_ONLY = {c for c in A_CASES if c.startswith(("vio_11_frames", "vio_13_frames"))}


# ---- the checks of A, shared with C ----

def marg_input(oracle, pb, victim):
    """(problem, state) to marginalize `victim` from: the window at the oracle's solution.  synth's own first-time prior is rank-deficient
    once the victim is not frame 0 (marg_compare.solved_window), so a middle victim gets marg_compare's regular prior BEFORE the solve; a
    vision-only window has no IMU factor and gets one over every frame AFTER it (test_marg_edges._case_f)."""
    if not pb.use_inertial:
        st, _ = _oracle_solve(oracle, pb)
        pb = wv.clone(pb)
        marg_compare.set_regular_prior(pb, np.arange(pb.n_frames))
        return pb, st
    if victim != 0 and not (pb.prior_S[6:, 6:] != 0).any():
        pb = wv.clone(pb)
        lin = pb.prior_lin_state.copy()
        marg_compare.set_regular_prior(pb, pb.prior_frames)
        pb.prior_lin_state = lin  # (the same rows for a synth window; a moved or flipped one keeps its own)
    return pb, _oracle_solve(oracle, pb)[0]


def check_window(ctxs, oracle, pb, solve_kw=None):
    out = {}
    st0, _ = _oracle_solve(oracle, pb)
    e0 = oracle.reprojection_error(pb, st0)
    for mode, ctx in ctxs.items():
        try:
            out["solve_%d" % mode] = ba_compare.check_against_oracle(ctx, oracle, pb, **(solve_kw or {}))["worst_state_diff"]
            np.testing.assert_allclose(ctx.reprojection_error(pb, st0), e0, rtol=1e-10)
        except AssertionError as e:
            raise AssertionError("linearize_mode %d: %s" % (mode, e)) from None
    for victim in (0, pb.n_frames // 2):
        pbst = marg_input(oracle, pb, victim)
        for mode, ctx in ctxs.items():
            try:
                marg_compare.check_marginalize(ctx, oracle, victim, pbst=pbst)
            except AssertionError as e:
                raise AssertionError("linearize_mode %d, victim %d: %s" % (mode, victim, e)) from None
        out["roles_%d" % victim] = marg_compare.check_roles_agree(ctxs[1], ctxs[2], pbst[0], pbst[1], victim)["info_matrix_rel"]
    return out


def run_a(ctxs, oracle, case):
    name, field = case.rsplit("-", 1)
    return check_window(ctxs, oracle, variant_window(oracle, name, field))


# ---- C: moved gauges ----

MOVES = {  # yaw [rad], |t| [m], flips
    "flips_only": (0.0, 0.0, True),
    "yaw_2.9": (2.9, 0.0, False),           # the composed quaternions pass through w < 0
    "yaw_2.9_t_1e3_flips": (2.9, 1.0e3, True),
    "yaw_1.0_t_1e5": (1.0, 1.0e5, False),
}
C_WINDOWS = ("vio_prior", "vio_plane", "vio_rot_prior")
C_CASES = ["%s-%s" % (n, m) for n in C_WINDOWS for m in MOVES]


def translation(pb, yaw, length):
    """a translation of the given length: a fixed generic direction, projected -- where the window has plane factors -- onto the complement
    of their moved normals (window_variants.move_gauge: only then is the moved window the same problem)"""
    d = np.array([0.6, -0.64, 0.48])
    if pb.n_plane_factors:
        normals = np.unique(pb.plane_normal, axis=0) @ wv.Gauge(yaw, np.zeros(3)).R.T
        for n in np.linalg.qr(normals.T)[0].T:
            d = d - (d @ n) * n
        assert np.linalg.norm(d) > 0.1, "the planes' normals span the space"
    return length * d / np.linalg.norm(d)


def sign_free_diff(a, b):
    """worst difference of two sets of frame states, quaternions compared up to their sign"""
    a, b = np.array(a, float, copy=True), np.array(b, float, copy=True)
    for i in range(a.shape[0]):
        if a[i, 0:4] @ b[i, 0:4] < 0:
            b[i, 0:4] *= -1.0
    return float(np.abs(a - b).max())


def decisions(sm):
    return [(t["step_is_valid"], t["step_is_successful"]) for t in sm.trace()]


def oracle_gauge_deviation(oracle, pb, moved, gauge):
    """the oracle's own distance between "solve the moved window" and "move the solution" (frame states up to quaternion sign, inverse depths)"""
    st_u, sm_u = _oracle_solve(oracle, pb)
    st_m, sm_m = _oracle_solve(oracle, moved)
    assert decisions(sm_m) == decisions(sm_u)
    return max(sign_free_diff(gauge.states(st_u.frame_state), st_m.frame_state), float(np.abs(st_u.lm_inv_depth - st_m.lm_inv_depth).max()))


def run_c(ctxs, oracle, case):
    name, move = case.rsplit("-", 1)
    yaw, length, flip = MOVES[move]
    pb = base_window(oracle, name)
    moved, gauge = wv.move_gauge(pb, yaw, translation(pb, yaw, length), flip)
    dev = oracle_gauge_deviation(oracle, pb, moved, gauge)
    if move == "flips_only":
        assert dev == 0.0, dev
    assert dev < 5e-4, "the oracle itself moves by %.3e under this gauge change: a finding about the window" % dev
    tol = max(STATE_TOL, 4.0 * dev)
    out = dict(oracle_deviation=dev, tol=tol)
    out.update(check_window(ctxs, oracle, moved))
    for mode, ctx in ctxs.items():
        st_u, sm_u = ctx.solve(pb)
        st_m, sm_m = ctx.solve(moved)
        assert decisions(sm_m) == decisions(sm_u), "linearize_mode %d" % mode
        d = max(sign_free_diff(gauge.states(st_u.frame_state), st_m.frame_state), float(np.abs(st_u.lm_inv_depth - st_m.lm_inv_depth).max()))
        out["carried_%d" % mode] = d
        print("%s linearize_mode %d: carried-over solution within %.3e (oracle %.3e, allowed %.3e)" % (case, mode, d, dev, tol))
        assert d <= tol, "linearize_mode %d: %.3e > %.3e" % (mode, d, tol)
    return out


# ---- D: the rotation-residual ladder ----

# each side of so3_right_jacobian's switches (7.30e-8, 1.63e-7, 6.32e-4, 1.03e-3 rad), q_logmap's exact-zero branch, a large angle, nearly pi
ANGLES = (0.0, 5e-8, 1e-7, 3e-7, 5e-4, 8e-4, 2e-3, 0.5, 3.1)
SOLVE_ANGLES = ANGLES[:7]  # (the larger ones make the prior dominate the cost: left to the marginalization check)
D_WINDOWS = ("vio_prior", "vio_rot_prior")
D_CASES = ["%s-from%d-%s" % (n, o, s) for n in D_WINDOWS for o in (0, 5) for s in ("plus", "minus")]


def ladder(oracle, name, offset, negate, angles):
    """(window with marg_compare's regular prior, the oracle's solution of it, that window with its references on the ladder): slot k --
    the prior frames, then the rotation priors -- gets angles[(offset + k) % len(angles)]"""
    key = ("solved", name)
    if key not in _cache:
        pb = wv.clone(base_window(oracle, name))
        marg_compare.set_regular_prior(pb, pb.prior_frames)
        _cache[key] = (pb, _oracle_solve(oracle, pb)[0])
    pb, st = _cache[key]
    n, r = pb.prior_frames.shape[0], pb.rot_prior_frame.shape[0]
    a = [angles[(offset + k) % len(angles)] for k in range(n + r)]
    return pb, st, wv.rotate_prior_reference(pb, st, a[:n], a[n:] if r else None, negate=negate, seed=offset)


def run_d(ctxs, oracle, case):
    name, off, sign = case.split("-")
    offset, negate = int(off[4:]), sign == "minus"
    pb, st, lad = ladder(oracle, name, offset, negate, ANGLES)
    out = {}
    victims = (0, int(pb.rot_prior_frame[1]) if pb.rot_prior_frame.shape[0] else pb.n_frames // 2)  # a victim with a rotation prior, where there is one
    for victim in victims:
        for mode, ctx in ctxs.items():
            try:
                marg_compare.check_marginalize(ctx, oracle, victim, pbst=(lad, st))
            except AssertionError as e:
                raise AssertionError("linearize_mode %d, victim %d: %s" % (mode, victim, e)) from None
        out["roles_%d" % victim] = marg_compare.check_roles_agree(ctxs[1], ctxs[2], lad, st, victim)["info_matrix_rel"]
    # two iterations from the solved state, where the residuals ARE the ladder's
    _, _, lad2 = ladder(oracle, name, offset, negate, SOLVE_ANGLES)
    lad2.frame_state, lad2.lm_inv_depth, lad2.max_iterations = st.frame_state.copy(), st.lm_inv_depth.copy(), 2
    for mode, ctx in ctxs.items():
        try:
            out["solve_%d" % mode] = ba_compare.check_against_oracle(ctx, oracle, lad2)["worst_state_diff"]
        except AssertionError as e:
            raise AssertionError("linearize_mode %d, two iterations: %s" % (mode, e)) from None
    return out


# ---- contexts ----

@pytest.fixture(scope="module")
def emu_roles():
    subprocess.check_call(["make", "-s", "-C", EMU_DIR, "libpvio_hipemu.so"])
    lib = capi.load(os.path.join(EMU_DIR, "libpvio_hipemu.so"))
    ctxs = {m: HipContext(lib=lib, use_graph=True, linearize_mode=m) for m in (1, 2)}
    yield ctxs
    for c in ctxs.values():
        c.close()


@pytest.fixture(scope="module")
def gpu_roles():
    ctxs = {m: HipContext(device=0, use_graph=True, linearize_mode=m) for m in (0, 1, 2)}  # raises without a GPU: no fallback
    yield ctxs
    for c in ctxs.values():
        c.close()


@pytest.fixture(scope="module")
def gpu_eager():
    ctx = HipContext(device=0, use_graph=False)
    yield ctx
    ctx.close()


# ---- A ----

@pytest.mark.parametrize("case", A_CASES)
def test_variant_window_is_an_ordinary_problem(oracle, case):
    """on the oracle alone: a per-frame window terminates like its base window, takes at least as many successful steps and ends below its
    initial cost -- the solver takes ordinary steps on it and does not fight inconsistent data"""
    name, field = case.rsplit("-", 1)
    _, sm0 = _oracle_solve(oracle, base_window(oracle, name))
    pb = variant_window(oracle, name, field)
    _, sm = _oracle_solve(oracle, pb)
    assert sm.termination == sm0.termination
    assert sm.num_successful_steps >= sm0.num_successful_steps
    assert sm.final_cost < sm.initial_cost
    for f in _fields_of(field):  # the rewrite did what it says: no two frames share a value, the stored signs are as documented
        arr = getattr(pb, wv._ARRAY_OF[f])
        if f == "imu" and not pb.use_inertial:
            continue
        assert len(np.unique(arr, axis=0)) == pb.n_frames
    if field in ("cam", "all"):
        assert (pb.cam_extrinsic[1::2, 3] < 0).all() and (pb.cam_extrinsic[0::2, 3] > 0).all()
    if pb.use_inertial and field in ("imu", "all"):
        assert (pb.imu_extrinsic[0::2, 3] < 0).all() and (pb.imu_extrinsic[1::2, 3] > 0).all()
    if field in ("W", "all"):
        assert (pb.sqrt_inv_cov[:, 1] != pb.sqrt_inv_cov[:, 2]).all() and (pb.sqrt_inv_cov[:, 1:3] != 0).all()


@pytest.mark.parametrize("case", [c for c in A_CASES if c not in GPU_ONLY])
def test_emulated_per_frame_calibration(emu_roles, oracle, case):
    print(case, run_a(emu_roles, oracle, case))


@pytest.mark.gpu
@pytest.mark.parametrize("case", A_CASES)
def test_gpu_per_frame_calibration(gpu_roles, oracle, case):
    print(case, run_a(gpu_roles, oracle, case))


@pytest.mark.gpu
def test_gpu_per_frame_calibration_sharded_path(oracle):
    """the one-rank sharded path (test_gpu_ba.test_gpu_one_rank_communicator_runs_the_sharded_path) on the all-fields VIO window"""
    lib = capi.load()
    ctx = HipContext(device=0, rank=0, world_size=1, force_sharded=True)
    try:
        uid = (C.c_uint8 * 128)()
        assert lib.pvio_hip_comm_unique_id(uid) == 0
        assert lib.pvio_hip_comm_init(ctx.ctx, uid, 0, 1) == 0
        print(ba_compare.check_against_oracle(ctx, oracle, variant_window(oracle, "vio_prior", "all")))
    finally:
        ctx.close()


@pytest.mark.gpu
def test_gpu_per_frame_calibration_eager_equals_graph(gpu_roles, gpu_eager, oracle):
    pb = variant_window(oracle, "vio_prior", "all")
    st_a, _ = gpu_roles[0].solve(pb)
    st_b, _ = gpu_eager.solve(pb)
    assert (st_a.frame_state == st_b.frame_state).all() and (st_a.lm_inv_depth == st_b.lm_inv_depth).all()
    ba_compare.check_against_oracle(gpu_eager, oracle, pb)


# ---- B ----

B_CASES = ["%s-%s-%s" % (n, c, f) for n in ("vision", "vio_prior", "vio_plane") for c in ("cam", "W", "intr", "imu", "all") for f in _fields_of(c)
           if f != "imu" or BASE[n][0].get("use_inertial")]


@pytest.mark.parametrize("case", B_CASES)
def test_variants_discriminate(oracle, case):
    """With frame 0's value of one field in every frame the oracle's solve moves some state by more than 1e-3 (1000 x STATE_TOL) and the
    marginalization information matrix by more than 1e-3 of its largest entry.  The intrinsics enter neither (they scale the pixel errors
    of lm_quality and of the mean reprojection error, oracle_ba.cpp): there the states must not move at all, and it is lm_quality (1000 x
    check_against_oracle's 1e-5 px) and the reprojection error (relative 1e-3) that must.  The camera extrinsics of a VIO window reach the
    1e-3 in the states only, see below."""
    name, variant, field = case.split("-")
    pb = variant_window(oracle, name, variant)
    col = wv.collapse_to_frame0(pb, [field])
    assert (getattr(col, wv._ARRAY_OF[field]) == getattr(pb, wv._ARRAY_OF[field])[0]).all()
    st, _ = _oracle_solve(oracle, pb)
    stc, _ = _oracle_solve(oracle, col)
    moved = max(np.abs(stc.frame_state - st.frame_state).max(), np.abs(stc.lm_inv_depth - st.lm_inv_depth).max())
    victim = pb.n_frames // 2
    pbm, stm = marg_input(oracle, pb, victim)
    colm = wv.collapse_to_frame0(pbm, [field])
    IM, IMc = oracle.marginalize(pbm, stm, victim)[2], oracle.marginalize(colm, stm, victim)[2]
    info = np.abs(IMc - IM).max() / np.abs(IM).max()
    print(case, "states move by %.3e, information matrix by %.3e of its largest entry" % (moved, info))
    if field == "intr":
        assert moved == 0.0 and info == 0.0
        assert np.abs(stc.lm_quality - st.lm_quality).max() > 1e-2
        e, ec = oracle.reprojection_error(pb, st), oracle.reprojection_error(col, st)
        assert abs(ec - e) > 1e-3 * e
    elif field == "cam" and pb.use_inertial:
        # Measured: 2.3e-4 .. 9.9e-4.  The largest entry of a VIO window's new prior is the gyro-bias random-walk information of the IMU
        # factors (1 / (cov_bg dt), ~1e10), and ALL the reprojection information of 36 .. 60 landmarks is ~1e7: turning every camera by
        # 0.2 rad changes a fifth of that, and no camera perturbation of these windows changes more than all of it.  So the 1e-3 is held
        # by the vision window (3.9e-2, above); here the states carry it (0.5 .. 1.4 against 1e-3) and the matrix must move by 1000 x
        # check_marginalize's own absolute tolerance (1e-9 of the largest entry).
        assert moved > 1e-3, moved
        assert info > 1e-6, info
    else:
        assert moved > 1e-3, moved
        assert info > 1e-3, info


# ---- C ----

def test_moved_plane_factor_on_the_oracle(oracle):
    """move_gauge's plane convention on the oracle's factor: with t orthogonal to the normal the residual and its Jacobian (rotated) are
    those of the unmoved factor; with t along the normal the residual's own convention d + n . t leaves the regularization row behind"""
    from oracle import oracle_py
    L = oracle_py.lib()
    d = lambda a: a.ctypes.data_as(oracle_py.dp)  # noqa: E731
    pb = base_window(oracle, "vio_plane")
    k = 0
    b, e = pb.plane_obs_ptr[k], pb.plane_obs_ptr[k + 1]
    fr = pb.plane_obs_frame[b:e]

    def factor(q):
        r, J = np.zeros(1), np.zeros((e - b, 6))
        L.oracle_eval_plane(int(e - b), d(np.ascontiguousarray(q.frame_state[fr])), d(np.ascontiguousarray(q.cam_extrinsic[fr])), d(np.ascontiguousarray(q.plane_obs_z[b:e])),
                            d(np.ascontiguousarray(q.plane_normal[k])), float(q.plane_distance[k]), float(q.plane_sqrt_inv_cov), d(r), d(J))
        return r[0], J

    r0, J0 = factor(pb)
    moved, g = wv.move_gauge(pb, 1.0, translation(pb, 1.0, 50.0), False)
    assert abs(moved.plane_normal[k] @ g.t) < 1e-12 * 50.0 and moved.plane_distance[k] == pytest.approx(pb.plane_distance[k], abs=1e-12)
    r1, J1 = factor(moved)
    assert abs(r1 - r0) <= 1e-9 * max(1.0, abs(r0)), (r0, r1)
    # theta is a body-frame tangent (unchanged), p a world one (rotated by R)
    np.testing.assert_allclose(J1[:, 0:3], J0[:, 0:3], atol=1e-8 * np.abs(J0).max())
    np.testing.assert_allclose(J1[:, 3:6], J0[:, 3:6] @ g.R.T, atol=1e-8 * np.abs(J0).max())
    along, _ = wv.move_gauge(pb, 0.0, 0.5 * pb.plane_normal[k], False)
    assert along.plane_distance[k] == pytest.approx(pb.plane_distance[k] + 0.5)
    assert abs(factor(along)[0] - r0) > 1.0  # the regularization row wants n . x = -d: not the same function any more


@pytest.mark.parametrize("case", C_CASES)
def test_emulated_moved_gauge(emu_roles, oracle, case):
    print(case, run_c(emu_roles, oracle, case))


@pytest.mark.gpu
@pytest.mark.parametrize("case", C_CASES)
def test_gpu_moved_gauge(gpu_roles, oracle, case):
    print(case, run_c(gpu_roles, oracle, case))


# ---- D ----

def test_ladder_has_the_requested_residuals(oracle):
    """Log(q0^-1 q) at the solved state has the norm asked for (what the oracle's logmap makes of it), exactly zero for angle 0, both signs"""
    from oracle import oracle_py
    L = oracle_py.lib()
    for negate in (False, True):
        pb, st, lad = ladder(oracle, "vio_rot_prior", 0, negate, ANGLES)
        refs = [(lad.prior_lin_state[i, 0:4], st.frame_state[f, 0:4]) for i, f in enumerate(lad.prior_frames)]
        refs += [(lad.rot_prior_q0[k], st.frame_state[f, 0:4]) for k, f in enumerate(lad.rot_prior_frame)]
        for k, (q0, q) in enumerate(refs):
            e, out = np.ascontiguousarray(wv.qmul(wv.qconj(q0), q)), np.zeros(3)
            L.oracle_logmap(e.ctypes.data_as(oracle_py.dp), out.ctypes.data_as(oracle_py.dp))
            want = ANGLES[k % len(ANGLES)]
            assert (q0[3] < 0) == (negate != (q[3] < 0)) or want > 0.4
            if want == 0:
                assert (out == 0).all() and (q0 == (-q if negate else q)).all()
            else:
                assert abs(np.linalg.norm(out) - want) <= 1e-9 * want + 1e-15, (want, np.linalg.norm(out))


@pytest.mark.parametrize("case", D_CASES)
def test_emulated_rotation_residual_ladder(emu_roles, oracle, case):
    print(case, run_d(emu_roles, oracle, case))


@pytest.mark.gpu
@pytest.mark.parametrize("case", D_CASES)
def test_gpu_rotation_residual_ladder(gpu_roles, oracle, case):
    print(case, run_d(gpu_roles, oracle, case))
