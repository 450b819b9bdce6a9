"""marginalize_frame (bundle_adjustor.cpp:348-599) at its edges, through both landmark roles of k_linearize.

Every case is a window edited after the oracle's solve and marginalized by the oracle (oracle_ba.cpp) and by the C ABI: in the fiber
emulator (tests/hipemu) with linearize_mode 1 (register-tile role) and 2 (large-window role, ba_lin_tp.h), on the GPU (-m gpu) with
linearize_mode 0, 1 and 2.  Each C-ABI prior must be finite and match the oracle within marg_compare's tolerances, and the two roles must
match each other to rounding (marg_compare.check_roles_agree).

  a  tracks the victim does not observe with a non-finite or zero inverse depth: not evaluated (:453-461), the prior equals that of the
     window without them
  b  landmarks anchored in the victim with no observation: no landmark_info entry, 1 / H_ll not finite -> skipped (:537-538)
  c  IMU and prior indices at their edges (:369-450): victim 1, the last frame, a victim outside prior_frames, no prior, a prior over all frames
  d  use_inertial = 0 with the pre-integration present (marginalization forces it on) and missing IMU factors next to the victim
  e  FF_FIX_POSE on the victim and on another frame (marginalization ignores it)
  f  plane-distance factors and duplicate blocks (lm_multiplicity): neither enters the prior (include/pvio_hip.h)
  g  the large-window role's geometry: unsorted anchors, a victim anchoring several chunks, the frame counts at its compile-time switches"""
import os
import subprocess

import numpy as np
import pytest

import ba_compare
import marg_compare
from pvio_amd import BAState, BASummary, capi, synth
from pvio_amd.solver import HipContext

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu")


# ---- window edits ----

def _solved(oracle, prior=None, **kw):
    """the window of `kw` solved by the oracle; prior: None (synth's own), "regular" (marg_compare's, over synth's prior frames) or a frame list"""
    if prior == "regular":
        return marg_compare.solved_window(oracle, regular_prior=True, **kw)
    pb = ba_compare.make(oracle, **kw)
    if prior is not None:
        marg_compare.set_regular_prior(pb, prior)
    st, sm = BAState(pb), BASummary(pb)
    oracle.solve(pb, st, sm)
    return pb, st


def _with_landmarks(pb, st, order):
    """the window with its landmarks `order` (a subset or a permutation) at the solved state"""
    pb2 = synth.permute_landmarks(pb, order)
    st2 = BAState(pb2)
    st2.frame_state[:] = st.frame_state
    st2.lm_inv_depth = np.ascontiguousarray(st.lm_inv_depth[np.asarray(order, np.int64)])
    return pb2, st2


def _unseen_by(pb, victim):
    ptr = pb.lm_obs_ptr
    return [l for l in range(pb.n_landmarks) if pb.lm_anchor_frame[l] != victim and not (pb.obs_frame[ptr[l]:ptr[l + 1]] == victim).any()]


# ---- the cases: name -> builder(oracle) -> (problem, state, victim, expected oracle prior or None = the oracle on the same input) ----

def _case_a(value, victim):
    def build(oracle):
        pb, st = _solved(oracle, prior="regular" if victim else None, n_frames=6, n_landmarks=80, use_inertial=True, visibility=3, seed=41)
        unseen = _unseen_by(pb, victim)
        assert len(unseen) >= 6
        poisoned = [unseen[0], unseen[len(unseen) // 2], unseen[-1]]
        keep = [l for l in range(pb.n_landmarks) if l not in poisoned]
        expect = oracle.marginalize(*_with_landmarks(pb, st, keep), victim)
        st.lm_inv_depth[poisoned] = value
        return pb, st, victim, expect
    return build


def _case_b(victim):
    def build(oracle):
        pb, st = _solved(oracle, prior="regular" if victim else None, n_frames=6, n_landmarks=80, use_inertial=True, visibility=3, seed=42)
        expect = oracle.marginalize(pb, st, victim)
        M, k = pb.n_landmarks, 4
        pb._canon()
        # four landmarks anchored in the victim whose observation lists are empty (CSR rows b == e), listed among the others
        pb.lm_anchor_frame = np.r_[pb.lm_anchor_frame, np.full(k, victim)].astype(np.int32)
        pb.lm_anchor_z = np.r_[pb.lm_anchor_z, pb.lm_anchor_z[:k] + 0.01]
        pb.lm_obs_ptr = np.r_[pb.lm_obs_ptr, np.full(k, pb.lm_obs_ptr[-1])].astype(np.int32)
        pb.lm_inv_depth = np.r_[pb.lm_inv_depth, np.full(k, 0.4)]
        pb.truth_inv_depth = None
        st.lm_inv_depth = np.r_[st.lm_inv_depth, np.full(k, 0.4)]
        order = np.random.default_rng(7).permutation(M + k)
        pb2, st2 = _with_landmarks(pb, st, order)
        assert (pb2.lm_obs_ptr[1:] == pb2.lm_obs_ptr[:-1]).sum() == k
        return pb2, st2, victim, expect
    return build


def _case_c(what):
    def build(oracle):
        kw = dict(n_frames=6, n_landmarks=60, use_inertial=True, visibility=4, seed=43)
        if what == "victim_1":
            pb, st = _solved(oracle, prior="regular", **kw)
            return pb, st, 1, None
        if what == "last_frame":  # one IMU factor; synth's prior frames are 0 .. N-2: the victim has no prior rows
            pb, st = _solved(oracle, prior="regular", **kw)
            return pb, st, 5, None
        if what == "victim_not_in_prior":  # prior over frames 0, 2, 5 (not contiguous, not first), victim 3
            pb, st = _solved(oracle, prior=[0, 2, 5], **kw)
            return pb, st, 3, None
        if what == "prior_over_all_frames":
            pb, st = _solved(oracle, prior=list(range(6)), **kw)
            return pb, st, 2, None
        if what.startswith("no_prior_"):  # prior_n = 0
            pb, st = _solved(oracle, **kw)
            pb.prior_frames, pb.prior_S, pb.prior_s, pb.prior_lin_state = np.zeros(0, np.int32), np.zeros((0, 0)), np.zeros(0), np.zeros((0, 16))
            return pb, st, int(what.split("_")[-1]), None
        raise KeyError(what)
    return build


def _case_d(what):
    def build(oracle):
        pb, st = _solved(oracle, prior="regular", n_frames=6, n_landmarks=60, use_inertial=True, visibility=4, seed=44)
        victim = 2
        pb.use_inertial = False  # marginalization forces the IMU factors on (ba_solver.cpp), where they exist
        if what == "victim_factor_missing":
            pb.preint_valid[victim] = 0
        elif what == "next_factor_missing":
            pb.preint_valid[victim + 1] = 0
        return pb, st, victim, None
    return build


def _case_e(victim):
    def build(oracle):
        pb, st = _solved(oracle, prior="regular" if victim else None, n_frames=6, n_landmarks=60, use_inertial=True, visibility=4, seed=45)
        pb.frame_fixed[victim] = 1
        pb.frame_fixed[4] = 1
        return pb, st, victim, None
    return build


def _case_f(name, victim):
    def build(oracle):
        kw = ba_compare.CASES[name]
        if kw.get("use_inertial"):
            pb, st = _solved(oracle, prior="regular" if victim else None, **kw)
        else:  # a vision-only window has no IMU factor: a prior over every frame (set after the solve) keeps the victim's 15 x 15 block regular
            pb, st = _solved(oracle, **kw)
            marg_compare.set_regular_prior(pb, np.arange(pb.n_frames))
        assert pb.n_plane_factors > 0 or pb.lm_multiplicity is not None
        return pb, st, victim, None
    return build


def _case_g(what):
    def build(oracle):
        if what == "unsorted_anchors":
            pb, st = _solved(oracle, prior="regular", n_frames=7, n_landmarks=150, use_inertial=True, visibility=3, seed=46)
            pb2, st2 = _with_landmarks(pb, st, np.random.default_rng(3).permutation(pb.n_landmarks))
            assert (np.diff(pb2.lm_anchor_frame) != 0).sum() > 60
            return pb2, st2, 3, None
        if what.startswith("victim_anchors_many_chunks"):  # every landmark anchored in frame 0 (8 x 200: 1400 factors, chunks of <= 256)
            victim = int(what.split("_")[-1])
            pb, st = _solved(oracle, prior="regular" if victim else None, n_frames=8, n_landmarks=200, use_inertial=True, seed=47)
            assert (pb.lm_anchor_frame == 0).all() and pb.n_obs > 4 * 256
            return pb, st, victim, None
        n = int(what.split("_")[-1])  # test_emu_ba.py's frame counts at the role's geometry switches, with IMU factors
        kw = dict(n_frames=n, n_landmarks=30 + 2 * n, use_inertial=True, visibility=max(2, min(n, 3 + n // 4)), seed=300 + n, max_iterations=2)
        pb, st = _solved(oracle, prior="regular", **kw)
        return pb, st, n // 2, None
    return build


CASES = {}
for _v in (0, 3):
    for _name, _x in (("zero", 0.0), ("inf", np.inf), ("nan", np.nan)):
        CASES["a_unseen_inv_depth_%s_victim%d" % (_name, _v)] = _case_a(_x, _v)
    CASES["b_empty_tracks_anchored_in_victim%d" % _v] = _case_b(_v)
    CASES["e_fixed_victim%d_and_frame4" % _v] = _case_e(_v)
for _w in ("victim_1", "last_frame", "victim_not_in_prior", "prior_over_all_frames", "no_prior_2", "no_prior_5"):
    CASES["c_" + _w] = _case_c(_w)
for _w in ("both_factors", "victim_factor_missing", "next_factor_missing"):
    CASES["d_no_inertial_" + _w] = _case_d(_w)
for _name in ("plane", "vio_plane", "vio_duplicate_blocks"):
    for _v in (0, 2):
        CASES["f_%s_victim%d" % (_name, _v)] = _case_f(_name, _v)
for _w in ["unsorted_anchors", "victim_anchors_many_chunks_0", "victim_anchors_many_chunks_4"] + ["frames_%d" % n for n in (2, 3, 10, 11, 15, 16, 22, 23, 27, 28, 31, 32)]:
    CASES["g_" + _w] = _case_g(_w)


# the frame counts past 16 take 20-60 s each in the fiber emulator (the register-tile role's walk over 30 frames): GPU only
GPU_ONLY = {"g_frames_%d" % n for n in (22, 23, 27, 28, 31, 32)}


def run_case(ctxs, oracle, name):
    pb, st, victim, expect = CASES[name](oracle)
    if expect is not None:  # the oracle itself: what it was not supposed to look at does not change its prior
        S0, s0, IM0, iv0 = oracle.marginalize(pb, st, victim)
        marg_compare.assert_finite_prior(S0, s0, IM0, iv0, "oracle")
        np.testing.assert_allclose(IM0, expect[2], rtol=1e-12, atol=1e-14 * np.abs(expect[2]).max())
        np.testing.assert_allclose(iv0, expect[3], rtol=1e-12, atol=1e-14 * np.abs(expect[3]).max())
    out = {}
    for mode, ctx in ctxs.items():
        try:
            out[mode] = marg_compare.check_marginalize(ctx, oracle, victim, pbst=(pb, st), expect=expect)
        except AssertionError as e:
            raise AssertionError("linearize_mode %d: %s" % (mode, e)) from None
    out["roles"] = marg_compare.check_roles_agree(ctxs[1], ctxs[2], pb, st, victim)
    return out


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


@pytest.mark.parametrize("name", sorted(set(CASES) - GPU_ONLY))
def test_emulated_marg_edge(emu_roles, oracle, name):
    print(name, run_case(emu_roles, oracle, name))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_gpu_marg_edge(gpu_roles, oracle, name):
    print(name, run_case(gpu_roles, oracle, name))


def _failed_marginalization_leaves_no_window(ctx):
    """A marginalization that fails behind its upload ("singular victim block": a vision-only window without a prior has no information on the
    victim's velocity and biases) has used the uploaded window up like one that succeeds: a resident solve answers "no problem uploaded" instead
    of solving the marginalization's window, and a fresh upload solves as before."""
    from pvio_amd.solver import HipError
    pb = synth.make_window(n_frames=2, n_landmarks=8, use_inertial=False, visibility=2)
    assert pb.n_obs == 8 and len(pb.prior_frames) == 0
    st = ctx.upload(pb)
    first = ctx.solve_resident(BASummary(pb, trace=False))
    with pytest.raises(HipError, match=r"status -1 \(singular victim block\)"):
        ctx.marginalize(pb, st, 0)
    with pytest.raises(HipError, match=r"status -1 \(no problem uploaded\)"):  # PVIO_ERR_INVALID_ARGUMENT
        ctx.solve_resident(BASummary(pb, trace=False))
    ctx.upload(pb)
    again = ctx.solve_resident(BASummary(pb, trace=False))
    assert again.num_iterations == first.num_iterations and again.final_cost == first.final_cost


def test_emulated_failed_marginalization_leaves_no_window(emu_roles):
    _failed_marginalization_leaves_no_window(emu_roles[1])


@pytest.mark.gpu
def test_gpu_failed_marginalization_leaves_no_window(gpu_roles):
    _failed_marginalization_leaves_no_window(gpu_roles[0])


@pytest.mark.gpu
def test_gpu_marg_large_window_roles_agree(gpu_roles, oracle):
    """10 KF x 50 000 landmarks (bench.py's large-window row), marginalized at the initial state: both roles, and the oracle"""
    pb = ba_compare.make(oracle, n_frames=10, n_landmarks=50000, use_inertial=True, seed=48)
    marg_compare.set_regular_prior(pb, pb.prior_frames)
    st = BAState(pb)
    for victim in (0, 4):
        print(victim, marg_compare.check_roles_agree(gpu_roles[1], gpu_roles[2], pb, st, victim))
        marg_compare.check_marginalize(gpu_roles[2], oracle, victim, pbst=(pb, st))
