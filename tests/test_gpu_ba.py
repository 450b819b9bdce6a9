"""GPU parity tests: hand-written HIP path (through the C-ABI of libpvio_hip.so) vs the CPU oracle.

Tolerance: north_star asks for pose/landmark states within 1e-6 per trust-region iteration; all BA arithmetic is
FP64 on both sides, observed differences are ~1e-10 (conditioning of the Jacobi-scaled reduced system ~1e8)."""
import numpy as np
import pytest

import ba_compare
from pvio_amd import BAState, BASummary

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu_ctx():
    from pvio_amd.solver import HipContext
    ctx = HipContext(device=0, use_graph=True)  # raises if the library or the GPU is missing: no fallback
    yield ctx
    ctx.close()


@pytest.mark.parametrize("name", sorted(ba_compare.CASES))
def test_gpu_matches_oracle_small(gpu_ctx, oracle, name):
    pb = ba_compare.make(oracle, **ba_compare.CASES[name])
    info = ba_compare.check_against_oracle(gpu_ctx, oracle, pb)
    print(name, info)


@pytest.mark.parametrize("name", sorted(ba_compare.BIG_CASES))
def test_gpu_matches_oracle_metric_configs(gpu_ctx, oracle, name):
    pb = ba_compare.make(oracle, **ba_compare.BIG_CASES[name])
    info = ba_compare.check_against_oracle(gpu_ctx, oracle, pb)
    print(name, info)


def test_gpu_eager_equals_graph(gpu_ctx, oracle):
    from pvio_amd.solver import HipContext
    pb = ba_compare.make(oracle, **ba_compare.CASES["vio_partial"])
    eager = HipContext(device=0, use_graph=False)
    st_a, _ = gpu_ctx.solve(pb)
    st_b, _ = eager.solve(pb)
    assert (st_a.frame_state == st_b.frame_state).all() and (st_a.lm_inv_depth == st_b.lm_inv_depth).all()
    eager.close()


def test_gpu_is_deterministic_and_resident_solve_repeats(gpu_ctx, oracle):
    pb = ba_compare.make(oracle, **ba_compare.BIG_CASES["metric_10x1000_vio"])
    gpu_ctx.upload(pb)
    outs = []
    for _ in range(3):
        sm = BASummary(pb, trace=False)
        gpu_ctx.solve_resident(sm)
        st = BAState(pb)
        gpu_ctx.download(st)
        outs.append((st.frame_state.copy(), st.lm_inv_depth.copy(), sm.num_iterations))
    for o in outs[1:]:
        assert (o[0] == outs[0][0]).all() and (o[1] == outs[0][1]).all() and o[2] == outs[0][2]


def test_gpu_large_window_properties(gpu_ctx, oracle):
    """BASELINE.json configs[4] size on one GPU (30 KF x 50k landmarks is too slow for the oracle in a test):
    size-independent properties instead -- cost decreases monotonically over accepted steps, the result is usable,
    reprojection quality ~ the injected pixel noise, landmark-shard sums equal the unsharded solve."""
    from pvio_amd import synth
    pb = synth.make_window(n_frames=30, n_landmarks=20000)
    st, sm = gpu_ctx.solve(pb)
    assert sm.is_usable == 1
    costs = [t["cost"] for t in sm.trace() if t["step_is_successful"]]
    assert len(costs) >= 3 and all(b < a for a, b in zip(costs, costs[1:]))
    assert sm.final_cost < 0.5 * sm.initial_cost
    assert (st.lm_valid == 1).all()
    assert 0.5 < st.lm_quality.mean() < 1.5
    err = gpu_ctx.reprojection_error(pb, st)
    np.testing.assert_allclose(err, st.lm_quality.mean(), rtol=1e-9)


def test_gpu_reprojection_error_matches_oracle(gpu_ctx, oracle):
    pb = ba_compare.make(oracle, **ba_compare.CASES["config1_10x200"])
    st = BAState(pb)
    np.testing.assert_allclose(gpu_ctx.reprojection_error(pb, st), oracle.reprojection_error(pb, st), rtol=1e-10)


@pytest.mark.parametrize("victim", [0, 3, 9])
def test_gpu_marginalize_matches_oracle(gpu_ctx, oracle, victim):
    import marg_compare
    print(marg_compare.check_marginalize(gpu_ctx, oracle, victim, n_frames=10, n_landmarks=300, use_inertial=True, visibility=6))


# rarely taken solver paths (failed factorization -> mu escalation + re-linearization, invalid steps, solver failure), forced
# by fault injection on both sides; includes the metric-size window so that the register-resident dense path is the one hit
@pytest.mark.parametrize("victim", [2, 5])
def test_gpu_marginalize_folds_the_victims_rotation_prior(gpu_ctx, oracle, victim):
    import marg_compare
    marg_compare.check_marginalize(gpu_ctx, oracle, victim, n_frames=10, n_landmarks=300, use_inertial=True, visibility=6, rot_prior_frames=(2, 5, 9))


@pytest.mark.parametrize("fail", [1, 3, 8])
def test_gpu_negative_pivot_is_detected_like_an_injected_failure(oracle, fail):
    """the metric window with 1000 + n: the next n factorizations meet a genuinely negative pivot (see tests/test_emu_ba.py)"""
    import ctypes as C

    from oracle import oracle_py
    from pvio_amd.solver import HipContext

    pb = ba_compare.make(oracle, **ba_compare.BIG_CASES["metric_10x1000_vio"])
    L = oracle_py.lib()
    L.oracle_debug_fault_injection(C.c_int32(fail), C.c_int32(0))
    ctx = HipContext(device=0, debug_fail_factorizations=1000 + fail)
    try:
        print(fail, ba_compare.check_against_oracle(ctx, oracle, pb))
    finally:
        L.oracle_debug_fault_injection(C.c_int32(0), C.c_int32(0))
        ctx.close()


@pytest.mark.parametrize("fail,invalid", [(1, 0), (3, 0), (0, 1), (0, 2), (0, 5), (8, 0)])
@pytest.mark.parametrize("case", ["vio_small", "metric_10x1000_vio"])
def test_gpu_fault_paths_match_oracle(oracle, fail, invalid, case):
    import ctypes as C

    from oracle import oracle_py
    from pvio_amd.solver import HipContext

    kw = ba_compare.CASES.get(case) or ba_compare.BIG_CASES[case]
    pb = ba_compare.make(oracle, **kw)
    L = oracle_py.lib()
    L.oracle_debug_fault_injection(C.c_int32(fail), C.c_int32(invalid))
    ctx = HipContext(device=0, debug_fail_factorizations=fail, debug_invalid_steps=invalid)
    try:
        print(case, fail, invalid, ba_compare.check_against_oracle(ctx, oracle, pb))
    finally:
        L.oracle_debug_fault_injection(C.c_int32(0), C.c_int32(0))
        ctx.close()


# ---- large windows: workgroups walk many chunks, the Schur complement accumulates on the matrix cores ----
LARGE_CASES = {
    "vio_30x4000_vis12": dict(n_frames=30, n_landmarks=4000, use_inertial=True, visibility=12),   # anchors change inside a workgroup's range
    "vision_10x20000": dict(n_frames=10, n_landmarks=20000),
    "vio_plane_20x6000": dict(n_frames=20, n_landmarks=6000, use_inertial=True, plane_fraction=0.2, visibility=10),
}


@pytest.mark.parametrize("name", sorted(LARGE_CASES))
def test_gpu_large_window_matches_oracle(gpu_ctx, oracle, name):
    pb = ba_compare.make(oracle, **LARGE_CASES[name])
    print(name, ba_compare.check_against_oracle(gpu_ctx, oracle, pb))


@pytest.mark.parametrize("name", ["metric_10x1000_vio", "vio_plane_10x600"])
def test_gpu_mfma_tiles_forced_on_small_windows(oracle, name):
    """linearize_mode = 2: the large-window accumulation on windows that would use the register tiles."""
    from pvio_amd.solver import HipContext
    ctx = HipContext(device=0, linearize_mode=2)
    pb = ba_compare.make(oracle, **ba_compare.BIG_CASES[name])
    print(name, ba_compare.check_against_oracle(ctx, oracle, pb))
    ctx.close()


# ---- round 6: the large-window landmark role (csrc/ba_lin_tp.h), forced on windows the oracle finishes in seconds ----
@pytest.fixture(scope="module")
def gpu_ctx_tp():
    from pvio_amd.solver import HipContext
    ctx = HipContext(device=0, linearize_mode=2)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("name", ["vio_duplicate_blocks", "vision_30x90_two_direct_tasks_per_thread", "vio_8x400_full_chunks", "vio_10x200_anchor_changes",
                                  "vision_16x120_twelve_tiles_per_wave", "vio_4x150", "vision_32x70_partial_visibility", "vio_32x60_partial_visibility"])
def test_gpu_large_window_role_matches_oracle(gpu_ctx_tp, oracle, name):
    """the emulator's cases of tests/test_emu_ba.py (duplicate blocks; 30 frames: two direct tasks per thread, twenty tiles per wave; chunks of 64
    landmarks; anchor flushes; ...) on the GPU, per iteration against the oracle"""
    kw = {"vio_duplicate_blocks": ba_compare.CASES["vio_duplicate_blocks"], "vision_30x90_two_direct_tasks_per_thread": dict(n_frames=30, n_landmarks=90, visibility=11),
          "vio_8x400_full_chunks": dict(n_frames=8, n_landmarks=400, use_inertial=True, visibility=3),
          "vio_10x200_anchor_changes": dict(n_frames=10, n_landmarks=200, use_inertial=True, visibility=5),
          "vision_16x120_twelve_tiles_per_wave": dict(n_frames=16, n_landmarks=120, visibility=9), "vio_4x150": dict(n_frames=4, n_landmarks=150, use_inertial=True, visibility=3),
          # 32 frames: every bit of a landmark's frame mask in use (tests/test_emu_ba.py: the unseen-frame walk once shifted by 32)
          "vision_32x70_partial_visibility": dict(n_frames=32, n_landmarks=70, visibility=10), "vio_32x60_partial_visibility": dict(n_frames=32, n_landmarks=60, use_inertial=True, visibility=8)}[name]
    print(name, ba_compare.check_against_oracle(gpu_ctx_tp, oracle, ba_compare.make(oracle, **kw)))


def test_gpu_large_window_role_unsorted_anchors_fixed_frame_and_marginalization(gpu_ctx_tp, oracle):
    """landmarks in RANDOM anchor order (a chunk per few landmarks, an anchor flush in front of most, anchors coming back), a fixed frame, and
    marginalize_frame through the same role (un-robustified blocks of the victim's tracks only)"""
    import marg_compare
    from pvio_amd import synth
    pb = ba_compare.make(oracle, n_frames=7, n_landmarks=150, use_inertial=True, visibility=3)
    pb2 = synth.permute_landmarks(pb, np.random.default_rng(3).permutation(pb.n_landmarks))
    assert (np.diff(pb2.lm_anchor_frame) != 0).sum() > 60
    ba_compare.check_against_oracle(gpu_ctx_tp, oracle, pb2)
    pb3 = ba_compare.make(oracle, n_frames=6, n_landmarks=120, visibility=4)
    pb3.frame_fixed[2] = 1
    ba_compare.check_against_oracle(gpu_ctx_tp, oracle, pb3)
    for victim in (0, 3):
        marg_compare.check_marginalize(gpu_ctx_tp, oracle, victim, n_frames=8, n_landmarks=500, use_inertial=True, visibility=5)


@pytest.mark.parametrize("seed", list(range(0, 60, 5)))
def test_gpu_large_window_role_on_the_random_sweep(gpu_ctx_tp, oracle, seed):
    """every fifth window of the random-shape sweep (2-32 frames, planes, IMU or not, fixed frames) through the large-window role"""
    kw, pb = ba_compare.sweep_window(oracle, seed)
    r = ba_compare.check_against_oracle_within_spread(gpu_ctx_tp, oracle, pb)
    print(seed, kw, r)
    if "skipped" in r:
        pytest.skip("window %d: %s" % (seed, r["skipped"]))


def test_gpu_large_window_role_is_deterministic_and_reads_nothing_stale(gpu_ctx_tp, oracle):
    """a 10 x 5000 window (two workgroups per CU, several chunks per workgroup): twenty resident re-solves bit-identical, also with every CU's LDS and
    registers left full of NaN / 1e300 by another kernel in between (the role clears nothing per chunk: every U cell it reads must have been written)"""
    import struct
    L, R = _poison_libs()
    pb = ba_compare.make(oracle, n_frames=10, n_landmarks=5000, use_inertial=True, visibility=7)
    gpu_ctx_tp.upload(pb)
    ref = None
    for k in range(20):
        if k % 5 == 4:
            pat = struct.unpack("<Q", struct.pack("<d", float("nan") if k % 10 == 4 else 1e300))[0]
            assert L.lds_poison(pat) == 0 and R.reg_poison(pat) == 0
        sm = BASummary(pb, trace=False)
        gpu_ctx_tp.solve_resident(sm)
        st = BAState(pb)
        gpu_ctx_tp.download(st)
        cur = (st.frame_state.copy(), st.lm_inv_depth.copy(), sm.final_cost, sm.num_iterations)
        ref = ref or cur
        assert (cur[0] == ref[0]).all() and (cur[1] == ref[1]).all() and cur[2:] == ref[2:], k
    st0, sm0 = BAState(pb), BASummary(pb)
    oracle.solve(pb, st0, sm0)
    assert sm0.num_iterations == ref[3]
    np.testing.assert_allclose(ref[0], st0.frame_state, rtol=0, atol=1e-6)
    np.testing.assert_allclose(ref[1], st0.lm_inv_depth, rtol=0, atol=1e-6)


def test_gpu_large_window_role_for_every_frame_count(oracle):
    """2 .. 32 frames through the large-window role: every class of its compile-time geometry (accumulator tiles per wave 3 / 6 / 12 / 17 / 20 / 23, one or two direct
    tasks per thread, U rows of 16 .. 208 doubles, one or two workgroups per CU) and every LDS size it asks for must launch and agree with the register-tile role
    (the 32-frame case once hung: see tests/test_emu_ba.py MM_CASES)."""
    from pvio_amd.solver import HipContext
    c1, c2 = HipContext(device=0, linearize_mode=1), HipContext(device=0, linearize_mode=2)
    for n in range(2, 33):
        vio = n % 3 != 0
        pb = ba_compare.make(oracle, n_frames=n, n_landmarks=60 + 5 * n, use_inertial=vio, visibility=max(2, min(n, 3 + n // 3)), seed=100 + n)
        (s1, m1), (s2, m2) = c1.solve(pb), c2.solve(pb)
        t1, t2 = m1.trace(), m2.trace()
        assert len(t1) == len(t2) and all((a["step_is_valid"], a["step_is_successful"]) == (b["step_is_valid"], b["step_is_successful"]) for a, b in zip(t1, t2)), n
        np.testing.assert_allclose(s2.frame_state, s1.frame_state, rtol=0, atol=1e-7, err_msg="%d frames" % n)
        np.testing.assert_allclose(s2.lm_inv_depth, s1.lm_inv_depth, rtol=0, atol=1e-7, err_msg="%d frames" % n)
    c1.close(), c2.close()


def test_gpu_both_linearize_modes_agree_on_a_large_window(oracle):
    from pvio_amd.solver import HipContext
    pb = ba_compare.make(oracle, n_frames=24, n_landmarks=8000, use_inertial=True, visibility=9)
    out = []
    for mode in (1, 2):
        ctx = HipContext(device=0, linearize_mode=mode)
        st, sm = ctx.solve(pb)
        out.append((st.frame_state.copy(), st.lm_inv_depth.copy(), sm.num_iterations, sm.final_cost))
        ctx.close()
    assert out[0][2] == out[1][2]
    np.testing.assert_allclose(out[0][0], out[1][0], rtol=0, atol=1e-7)
    np.testing.assert_allclose(out[0][1], out[1][1], rtol=0, atol=1e-7)
    np.testing.assert_allclose(out[0][3], out[1][3], rtol=1e-9)


@pytest.mark.parametrize("shape,sharded", [((30, 50000), False), ((10, 50000), False), ((10, 50000), True)], ids=["30x50000", "10x50000", "10x50000_one_rank_sharded"])
def test_gpu_full_size_window_matches_the_oracle_golden(oracle, shape, sharded):
    """BASELINE.json configs[4] (30 KF x 50 000) and the window north_star states the multi-GPU target on (10 KF x 50 000, what
    `bench.py --gpus N` shards) at full size against the oracle's states: the oracle's solves of the same (regenerated,
    fingerprinted) windows were run once offline and frozen in tests/golden/ba_vio_<shape>.npz (make_golden_large.py): same
    accept / reject trace and termination, costs and trust-region radii, frame states after EVERY iteration and the final
    50 000 inverse depths within the 1e-6 bar of north_star.  The 10 x 50 000 window also goes through the landmark-sharded
    code path (one-rank RCCL communicator, graph-captured collectives) -- the multi-GPU headline's path minus a second rank."""
    import ctypes as C
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_golden_large
    from pvio_amd import capi
    from pvio_amd.solver import HipContext
    n_frames, n_landmarks = shape
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ba_vio_%dx%d.npz" % shape))
    pb = ba_compare.make(oracle, n_frames=n_frames, n_landmarks=n_landmarks, use_inertial=True)
    assert make_golden_large.fingerprint(pb) == str(g["inputs_sha256"]), "the regenerated window is not the one the golden was computed on"
    if sharded:
        lib = capi.load()
        ctx = HipContext(device=0, rank=0, world_size=1, force_sharded=True)
        uid = (C.c_uint8 * 128)()
        assert lib.pvio_hip_comm_unique_id(uid) == 0 and lib.pvio_hip_comm_init(ctx.ctx, uid, 0, 1) == 0
    else:
        ctx = HipContext(device=0)
    try:
        st, sm = ctx.solve(pb)
    finally:
        ctx.close()
    tr = sm.trace()
    assert sm.termination == int(g["termination"]) and sm.num_iterations == int(g["num_iterations"]) and len(tr) == len(g["costs"])
    assert ([t["step_is_successful"] for t in tr] == g["successful"]).all()
    np.testing.assert_allclose([t["cost"] for t in tr], g["costs"], rtol=1e-7)
    np.testing.assert_allclose([t["trust_region_radius"] for t in tr], g["radius"], rtol=1e-6)
    nfs = pb.n_frames * 16
    worst = 0.0
    for k in range(len(tr)):
        d = np.abs(sm.trace_states[k][:nfs] - g["frame_states"][k]).max()
        worst = max(worst, float(d))
        assert d <= ba_compare.STATE_TOL, (k, d)
    np.testing.assert_allclose(st.frame_state, g["final_frame_state"], rtol=0, atol=ba_compare.STATE_TOL)
    np.testing.assert_allclose(st.lm_inv_depth, g["final_inv_depth"], rtol=0, atol=ba_compare.STATE_TOL)
    print("%dx%d%s vs the oracle golden: max frame-state difference over all iterations %.2e, inverse depths %.2e"
          % (n_frames, n_landmarks, " (sharded path, one rank)" if sharded else "", worst, np.abs(st.lm_inv_depth - g["final_inv_depth"]).max()))


def test_gpu_full_size_window_properties(oracle):
    """BASELINE.json configs[4] (30 KF x 50 000 landmarks, 1.45 M factors, full VIO factor set) at full size, through
    properties that do not need the oracle's solve: the cost the solver reports for its final state is the cost the
    oracle's evaluator computes for that state; accepted steps decrease the cost; the two accumulation forms of
    k_linearize agree; iterating again from the result does not move it (the solve has converged or hit the cap)."""
    from pvio_amd.solver import HipContext
    pb = ba_compare.make(oracle, n_frames=30, n_landmarks=50000, use_inertial=True)
    res = {}
    for mode in (2, 1):
        ctx = HipContext(device=0, linearize_mode=mode)
        st, sm = ctx.solve(pb)
        res[mode] = (st, sm)
        ctx.close()
    st, sm = res[2]
    assert sm.is_usable == 1 and sm.final_cost < 0.7 * sm.initial_cost
    costs = [t["cost"] for t in sm.trace() if t["step_is_successful"]]
    assert all(b < a for a, b in zip(costs, costs[1:]))
    # the IMU factors read the biases of the user state live (preintegration_error_cost.h:57-58); the accepted candidate was
    # evaluated while the user state still was the previous iterate
    tr = sm.trace()
    k_last = max(k for k, t in enumerate(tr) if t["step_is_successful"])
    nfs = pb.n_frames * 16
    user = sm.trace_states[k_last - 1][:nfs].reshape(pb.n_frames, 16)
    c = oracle.cost(pb, st.frame_state, st.lm_inv_depth, user=user)
    np.testing.assert_allclose(sm.final_cost, c, rtol=1e-9)
    np.testing.assert_allclose(oracle.cost(pb, pb.frame_state, pb.lm_inv_depth), sm.initial_cost, rtol=1e-9)
    st1, sm1 = res[1]
    assert sm1.num_iterations == sm.num_iterations
    np.testing.assert_allclose(sm1.final_cost, sm.final_cost, rtol=1e-9)
    np.testing.assert_allclose(st1.frame_state, st.frame_state, rtol=0, atol=1e-7)
    np.testing.assert_allclose(st1.lm_inv_depth, st.lm_inv_depth, rtol=0, atol=1e-7)


@pytest.mark.parametrize("name", ["vio_partial", "vio_plane", "metric_10x1000_vio", "vio_13_frames_global_matrix", "vio_duplicate_blocks"])
def test_gpu_one_rank_communicator_runs_the_sharded_path(oracle, name):
    """The landmark-sharded code path on the one GPU there is: a ONE-rank RCCL communicator (ncclCommInitRank with nranks = 1)
    carries the real all-reduces on the solver's stream, launches are eager, the reduced system is assembled from the
    all-reduced buffer -- everything the multi-GPU run does except a second rank.  Results must equal the oracle's."""
    import ctypes as C
    from pvio_amd import capi
    from pvio_amd.solver import HipContext
    lib = capi.load()
    ctx = HipContext(device=0, rank=0, world_size=1, force_sharded=True)
    try:
        uid = (C.c_uint8 * 128)()
        assert lib.pvio_hip_comm_unique_id(uid) == 0
        assert lib.pvio_hip_comm_init(ctx.ctx, uid, 0, 1) == 0
        pb = ba_compare.make(oracle, **{**ba_compare.CASES, **ba_compare.BIG_CASES}[name])
        print(name, ba_compare.check_against_oracle(ctx, oracle, pb))
    finally:
        ctx.close()


def test_gpu_sharded_path_without_communicator_fails_loudly(oracle):
    from pvio_amd.solver import HipContext, HipError
    ctx = HipContext(device=0, force_sharded=True)
    try:
        with pytest.raises(HipError):
            ctx.solve(ba_compare.make(oracle, **ba_compare.CASES["vision_small"]))
    finally:
        ctx.close()


@pytest.mark.parametrize("seed", list(range(12)))
def test_gpu_random_windows_match_oracle(gpu_ctx, oracle, seed):
    """Windows of random shape (frames, landmarks, visibility, plane share, inertial or not, fixed frames) beyond the named
    cases: same iteration-by-iteration agreement with the oracle."""
    import numpy as np
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.integers(3, 15))
    kw = dict(n_frames=n, n_landmarks=int(rng.integers(20, 500)), use_inertial=bool(rng.integers(0, 2)), visibility=int(rng.integers(2, n + 1)),
              plane_fraction=float(rng.choice([0.0, 0.0, 0.3, 0.6])), seed=int(rng.integers(1, 10000)))
    pb = ba_compare.make(oracle, **kw)
    if rng.random() < 0.4:
        pb.frame_fixed[int(rng.integers(0, n))] = 1
    print(kw, ba_compare.check_against_oracle(gpu_ctx, oracle, pb))


_SWEEP = {"run": 0, "skipped": []}  # windows of the two spread-tolerance sweeps that were run / not compared (decision-boundary windows)


@pytest.mark.parametrize("seed", list(range(60)))
def test_gpu_window_sweep_within_oracle_spread(gpu_ctx, oracle, seed):
    """The 60-window sweep of profiles/r*_sweep_random_windows.txt as a bounded test: 2-32 frames, 10-1500 landmarks,
    incl. the many-frame two-view windows.  Tolerance per window: north_star's 1e-6, or -- where the ORACLE'S OWN reorderings of the sums over
    landmarks differ by more (computed in the test: ba_compare.oracle_spread; windows 15, 20, 37: 2.6e-4, 6.9e-6, 6.4e-7 in the states,
    8.5e-5 px in the quality of #37) -- four times that spread."""
    kw, pb = ba_compare.sweep_window(oracle, seed)
    r = ba_compare.check_against_oracle_within_spread(gpu_ctx, oracle, pb)
    print(seed, kw, r)
    _SWEEP["run"] += 1
    if "skipped" in r:  # a window that is not compared shows as SKIPPED, is counted, and the count is bounded below
        assert seed not in (15, 20, 37)  # (the three ill-conditioned windows are not decision-boundary cases)
        _SWEEP["skipped"].append(("sweep", seed))
        pytest.skip("window %d: %s" % (seed, r["skipped"]))


@pytest.mark.parametrize("case", range(len(ba_compare.TWO_VIEW_CASES)))
def test_gpu_many_frame_two_view_windows(gpu_ctx, oracle, case):
    """15-31 frames, every landmark seen by exactly two of them, vision only (no gauge): the class the sweep's three outliers belong to"""
    pb = ba_compare.make(oracle, **ba_compare.TWO_VIEW_CASES[case])
    r = ba_compare.check_against_oracle_within_spread(gpu_ctx, oracle, pb)
    print(ba_compare.TWO_VIEW_CASES[case], r)
    _SWEEP["run"] += 1
    if "skipped" in r:
        _SWEEP["skipped"].append(("two_view", case))
        pytest.skip("two-view window %d: %s" % (case, r["skipped"]))


def test_gpu_window_sweep_compares_nearly_every_window():
    """a window on which the oracle's own summation orders disagree about a step's acceptance is skipped, not compared; at most 2
    of the 66 windows of the two sweeps above may go that way (none does at the time of writing: profiles/r6_pytest_gpu.txt)."""
    print("windows run %d, skipped %s" % (_SWEEP["run"], _SWEEP["skipped"]))
    assert len(_SWEEP["skipped"]) <= 2, _SWEEP["skipped"]


def poison_device_memory(poison):
    """4 GB of device memory filled with `poison` and handed back to the driver: what a context created next allocates is carved from them
    (also used by tests/test_solver_exits.py)"""
    import torch
    xs = [torch.full((64 * 1024 * 1024,), poison, dtype=torch.float64, device="cuda") for _ in range(8)]
    torch.cuda.synchronize()
    del xs
    torch.cuda.empty_cache()
    torch.cuda.synchronize()


@pytest.mark.parametrize("poison", [float("nan"), 1e300], ids=["nan", "1e300"])
def test_gpu_solver_reads_nothing_it_did_not_write(oracle, poison):
    """A fresh context on device memory that a previous owner left full of NaN (or 1e300): 4 GB are filled and handed back to the
    driver right before the solver allocates, so that its buffers are carved from them.  Any scratch / padding / second-buffer
    word read before it is written would end in a different trace; the solves must equal the oracle's as usual.  (Fresh pages
    from the driver are zeroed, which is the other thing a first solve may meet: every other GPU test starts that way.)"""
    from pvio_amd.solver import HipContext
    for name in ("vio_small", "vision_partial", "vio_plane"):
        pb = ba_compare.make(oracle, **ba_compare.CASES[name])
        poison_device_memory(poison)
        ctx = HipContext(device=0)
        try:
            ba_compare.check_against_oracle(ctx, oracle, pb)
        finally:
            ctx.close()


def test_gpu_dense_hundred_repeats_are_bit_identical(gpu_ctx, oracle):
    """the 10 x 1000 VIO window solved a hundred times over from the same resident state -- every solve bit-identical to
    the first (a timing-dependent variant of the dense kernel -- a race between its waves, in the look-ahead form the counters that
    replaced its barriers -- would show up as a difference) and the first one equal to the oracle's."""
    pb = ba_compare.make(oracle, **ba_compare.BIG_CASES["metric_10x1000_vio"])
    ba_compare.check_against_oracle(gpu_ctx, oracle, pb)
    gpu_ctx.upload(pb)
    ref = None
    for k in range(100):
        sm = BASummary(pb, trace=False)
        gpu_ctx.solve_resident(sm)
        st = BAState(pb)
        gpu_ctx.download(st)
        cur = (st.frame_state.tobytes(), st.lm_inv_depth.tobytes(), sm.num_iterations, sm.final_cost)
        if ref is None:
            ref = cur
        assert cur == ref, "solve %d differs from the first" % k


def _poison_libs():
    import ctypes as C
    import os
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "micro")
    lds, reg = os.path.join(d, "liblds_poison.so"), os.path.join(d, "libreg_poison.so")
    if not (os.path.exists(lds) and os.path.exists(reg)):
        pytest.skip("tests/micro/lib{lds,reg}_poison.so not built (build() makes them)")
    L, R = C.CDLL(lds), C.CDLL(reg)
    L.lds_poison.argtypes, R.reg_poison.argtypes = [C.c_uint64], [C.c_uint64]
    return L, R


@pytest.mark.parametrize("name", ["vision_small", "vio_partial", "config1_10x200"])
def test_gpu_solver_reads_no_stale_lds_or_registers(gpu_ctx, oracle, name):
    """LDS and registers are not cleared between kernels: a kernel that reads what it has not written sees the leftovers of whatever ran
    before on that CU / SIMD.  Every CU's LDS and every SIMD's VGPRs / AGPRs / SGPRs are filled with NaN, then 1e300, then zero
    (tests/micro/{lds,reg}_poison.hip) in front of a solve: the result must not move.  (Device MEMORY pre-filled the same way:
    test_gpu_solver_reads_nothing_it_did_not_write.)"""
    import struct
    L, R = _poison_libs()
    pb = ba_compare.make(oracle, **ba_compare.CASES[name])
    base = ba_compare.check_against_oracle(gpu_ctx, oracle, pb)
    st0, _ = gpu_ctx.solve(pb)
    for val in (float("nan"), 1e300, 0.0):
        pat = struct.unpack("<Q", struct.pack("<d", val))[0]
        assert L.lds_poison(pat) == 0 and R.reg_poison(pat) == 0
        st1, _ = gpu_ctx.solve(pb)
        assert (st1.frame_state == st0.frame_state).all() and (st1.lm_inv_depth == st0.lm_inv_depth).all(), (name, val, base)


# ---- pvio_hip_opts::reuse_identical_candidates -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu_ctx_reuse():
    from pvio_amd.solver import HipContext
    ctx = HipContext(device=0, use_graph=True, reuse_identical_candidates=True)
    yield ctx
    ctx.close()


# (the adapter's default is ON, so the whole case matrix runs with it, not a selection)
@pytest.mark.parametrize("name,saved", [(n, {"vio_partial": 2, "vio_zero_bias_quirk": 4, "vio_plane": 1, "vision_partial": 0}.get(n)) for n in sorted(ba_compare.CASES)] +
                         [(n, None) for n in sorted(ba_compare.BIG_CASES)])
def test_gpu_identical_candidates_are_not_evaluated_twice(gpu_ctx_reuse, oracle, name, saved):
    """a candidate that is bit-identical to the one just rejected is not evaluated again: same iterations, records and per-iteration states as the
    oracle, which -- like Ceres -- evaluates every candidate"""
    pb = ba_compare.make(oracle, **(ba_compare.CASES.get(name) or ba_compare.BIG_CASES[name]))
    print(name, ba_compare.check_against_oracle(gpu_ctx_reuse, oracle, pb), "evaluations saved:", gpu_ctx_reuse.last_candidate_repeats())
    if saved is not None:
        assert gpu_ctx_reuse.last_candidate_repeats() == saved


def test_gpu_identical_candidates_metric_window_and_resident_repeats(gpu_ctx_reuse, gpu_ctx, oracle):
    """the metric window: three of its ten candidate evaluations are repeats; resident re-solves are bit-identical to each other and to the solves of
    a context that evaluates everything"""
    pb = ba_compare.make(oracle, **ba_compare.BIG_CASES["metric_10x1000_vio"])
    ba_compare.check_against_oracle(gpu_ctx_reuse, oracle, pb)
    assert gpu_ctx_reuse.last_candidate_repeats() == 3
    outs = []
    for ctx in (gpu_ctx, gpu_ctx_reuse):
        ctx.upload(pb)
        for _ in range(5):
            sm = BASummary(pb, trace=False)
            ctx.solve_resident(sm)
            st = BAState(pb)
            ctx.download(st)
            outs.append((st.frame_state.copy(), st.lm_inv_depth.copy(), sm.final_cost, sm.num_iterations))
    for o in outs[1:]:
        assert (o[0] == outs[0][0]).all() and (o[1] == outs[0][1]).all() and o[2] == outs[0][2] and o[3] == outs[0][3]
