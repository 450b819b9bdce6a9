"""Shared parity check: a C-ABI solve (real GPU library or the emulated test build) against the CPU oracle."""
import numpy as np

from pvio_amd import BAState, BASummary, synth

# north_star: "pose/landmark states within 1e-6 per LM iteration"
STATE_TOL = 1e-6

CASES = {
    "vision_small": dict(n_frames=4, n_landmarks=30),
    "vio_five_landmarks": dict(n_frames=4, n_landmarks=5, use_inertial=True),  # sharded over 8 ranks: three ranks without a landmark
    "vision_partial": dict(n_frames=6, n_landmarks=40, visibility=3),
    "vio_small": dict(n_frames=4, n_landmarks=30, use_inertial=True),
    "vio_partial": dict(n_frames=6, n_landmarks=40, use_inertial=True, visibility=4),
    "plane": dict(n_frames=5, n_landmarks=60, plane_fraction=0.5),
    "vio_plane": dict(n_frames=5, n_landmarks=60, plane_fraction=0.4, use_inertial=True),
    # RotationPriorFactor (BASELINE.json north_star; no reference counterpart): on free frames, on the fixed frame 0 of a
    # vision-only window (a constant block, dropped), next to IMU factors and the gauge prior
    "vision_rot_prior": dict(n_frames=5, n_landmarks=40, visibility=4, rot_prior_frames=(0, 2, 4)),
    "vio_rot_prior": dict(n_frames=5, n_landmarks=40, use_inertial=True, visibility=4, rot_prior_frames=(1, 3, 4)),
    "vio_zero_bias_quirk": dict(n_frames=4, n_landmarks=30, use_inertial=True, bias_init="zero", perturb_scale=1.0),
    # duplicate residual blocks (bundle_adjustor.cpp:165-179): tracks of planes with fewer than 20 members are listed twice / three times
    "vision_duplicate_blocks": dict(n_frames=5, n_landmarks=50, visibility=4, duplicate_fraction=0.4),
    "vio_duplicate_blocks": dict(n_frames=6, n_landmarks=70, use_inertial=True, visibility=4, duplicate_fraction=0.3),
    # BASELINE.json configs[1]: 10 KF x 200 landmarks, reprojection factors only
    "config1_10x200": dict(n_frames=10, n_landmarks=200),
    "vio_11_frames_lds_limit": dict(n_frames=11, n_landmarks=80, use_inertial=True, visibility=6),   # reduced system 165: largest that stays in LDS
    "vio_13_frames_global_matrix": dict(n_frames=13, n_landmarks=80, use_inertial=True, visibility=6),  # 195: matrix in HBM
    # matrix in HBM, factored in LDS-resident panels: 300 rows = nine 32-column panels + one of 16; 480 rows = 16-column panels
    # (a 32-column panel of 496 rows does not fit the LDS); the 13-frame window above ends in an 8-column panel
    "vio_20_frames_panels": dict(n_frames=20, n_landmarks=120, use_inertial=True, visibility=7),
    "vio_32_frames_narrow_panels": dict(n_frames=32, n_landmarks=160, use_inertial=True, visibility=8),
}
# (these were too slow for the fiber emulator while it switched fibers with swapcontext(): GPU only, rounds 1-2)
GPU_ONLY = set()  # (round 3: the emulator switches fibers without system calls; the 20- and 32-frame windows take 4 s and 8 s in it)
BIG_CASES = {
    # the configuration the metric is quoted on (10 KF x 1000 landmarks), vision-only and full VIO
    "metric_10x1000_vision": dict(n_frames=10, n_landmarks=1000),
    "metric_10x1000_vio": dict(n_frames=10, n_landmarks=1000, use_inertial=True),
    "vio_plane_10x600": dict(n_frames=10, n_landmarks=600, use_inertial=True, plane_fraction=0.4, visibility=6),
    "vio_rot_prior_10x1000": dict(n_frames=10, n_landmarks=1000, use_inertial=True, rot_prior_frames=(2, 5, 9)),
    "vio_duplicates_10x1000": dict(n_frames=10, n_landmarks=1000, use_inertial=True, duplicate_fraction=0.1),
}


def sweep_window(oracle, seed):
    """window `seed` of the random-shape sweep (tests/sweep_random_windows.py, profiles/r*_sweep_random_windows.txt): 2-32 frames, 10-1500
    landmarks, visibility 2..n, plane share, inertial or not, sometimes a fixed frame"""
    rng = np.random.default_rng(5000 + seed)
    n = int(rng.integers(2, 33))
    kw = dict(n_frames=n, n_landmarks=int(rng.integers(10, 1500)), use_inertial=bool(rng.integers(0, 2)), visibility=int(rng.integers(2, n + 1)),
              plane_fraction=float(rng.choice([0.0, 0.0, 0.3, 0.6])), seed=int(rng.integers(1, 10000)))
    pb = make(oracle, **kw)
    if rng.random() < 0.4:
        pb.frame_fixed[int(rng.integers(0, n))] = 1
    return kw, pb


# many-frame windows whose landmarks are seen by exactly two frames, vision only: the class the three sweep windows that miss 1e-6 belong to
TWO_VIEW_CASES = [dict(n_frames=n, n_landmarks=m, visibility=2, plane_fraction=pf, seed=sd)
                  for n, m, pf, sd in ((15, 300, 0.0, 11), (19, 700, 0.0, 12), (24, 500, 0.3, 13), (28, 1200, 0.0, 14), (31, 469, 0.0, 2364), (17, 816, 0.6, 8707))]


def make(oracle, **kw):
    if kw.get("use_inertial"):
        kw = dict(kw, preintegrate=oracle.preintegrate)
    return synth.make_window(**kw)


def oracle_spread(oracle, pb):
    """What a REORDERING of the sums over landmarks does to the oracle's own result on this window: the oracle under
    its three other summation orders (oracle_debug_sum_order) against its default order -- worst state difference over every iterate of
    the trace, worst relative cost difference, and whether every order takes the same accept / reject decisions.  The kernels sum in yet
    another order (chunks of landmarks per workgroup, a tree inside); on a well-conditioned window all of this is 1e-14, on a vision-only
    window whose landmarks are seen by two frames each (no gauge, depths barely observable) it reaches 1e-4."""
    runs = []
    try:
        for order in (0, 1, 2, 3):
            oracle.set_sum_order(order)
            st, sm = BAState(pb), BASummary(pb)
            oracle.solve(pb, st, sm)
            t = sm.trace()
            runs.append((t, [x.copy() for x in sm.trace_states[:len(t)]], st.lm_quality.copy()))
    finally:
        oracle.set_sum_order(0)
    t0, x0, q0 = runs[0]
    state, cost, quality, same = 0.0, 0.0, 0.0, True
    for t, x, q in runs[1:]:
        if len(t) != len(t0) or any((a["step_is_valid"], a["step_is_successful"]) != (b["step_is_valid"], b["step_is_successful"]) for a, b in zip(t0, t)):
            same = False
            continue
        state = max([state] + [float(np.abs(a - b).max()) for a, b in zip(x0, x)])
        cost = max([cost] + [abs(a["cost"] - b["cost"]) / abs(a["cost"]) for a, b in zip(t0, t) if a["cost"] != 0])
        quality = max(quality, float(np.abs(q - q0).max()))
    return dict(state=state, cost_rel=cost, quality=quality, same_decisions=same)


def check_against_oracle_within_spread(ctx, oracle, pb, c=4.0):
    """check_against_oracle with north_star's 1e-6 -- widened, where the oracle's OWN reorderings differ by more than that, to c times
    their spread (computed here, on this window).  A window on which the oracle's orders disagree about a step's acceptance sits on a
    decision boundary: it is reported and not compared (no summation order is the reference's there)."""
    sp = oracle_spread(oracle, pb)
    if not sp["same_decisions"]:
        return dict(sp, skipped="the oracle's own summation orders take different accept / reject decisions on this window")
    # the widening is capped -- a spread beyond twice the worst window known (#15: 2.6e-4 in the states, 0.022 px in one landmark's quality) is a
    # finding about the oracle, not a tolerance
    assert sp["state"] <= 5e-4 and sp["quality"] <= 0.05, sp
    tol = max(STATE_TOL, c * sp["state"])
    r = check_against_oracle(ctx, oracle, pb, state_tol=tol, cost_rtol=max(1e-7, c * sp["cost_rel"]), trace_scale=tol / STATE_TOL,
                             quality_atol=max(1e-5, c * sp["quality"]))
    return dict(r, spread=sp["state"], tol=tol)


def check_against_oracle(ctx, oracle, pb, state_tol=STATE_TOL, cost_rtol=1e-7, trace_scale=1.0, quality_atol=1e-5, cost_atol_rel=0.0):
    """cost_atol_rel (default 0: costs are compared relatively, to cost_rtol) adds an absolute term cost_atol_rel * initial_cost to the cost
    comparisons of the trace and of the final cost.  A solve that converges on noise-free data ends 10 to 14 orders of magnitude below the
    cost it started from: what is left is the rounding residue of sums whose terms were of the size of the initial cost, and two correct
    evaluations of it in different summation orders agree to ~1e-16 of THAT, not to 1e-7 of the residue (seen: every decision equal, every
    state within 1e-10, final costs 3.7e-15 apart = 1.3e-7 of the residue).  The tests of such windows pass cost_atol_rel = cost_rtol: the
    same 1e-7, at the scale of the solve.  Everything else -- termination, iteration and step counts, trace length, accept / reject flags,
    mu, the states -- is compared as without it."""
    st0, sm0 = BAState(pb), BASummary(pb)
    oracle.solve(pb, st0, sm0)
    st1, sm1 = ctx.solve(pb)
    t0, t1 = sm0.trace(), sm1.trace()
    cost_atol = cost_atol_rel * sm0.initial_cost
    assert sm1.termination == sm0.termination
    assert sm1.num_iterations == sm0.num_iterations
    assert sm1.num_successful_steps == sm0.num_successful_steps
    assert len(t1) == len(t0)
    for a, b in zip(t0, t1):
        assert a["iteration"] == b["iteration"]
        assert a["step_is_valid"] == b["step_is_valid"], (a, b)
        assert a["step_is_successful"] == b["step_is_successful"], (a, b)
        np.testing.assert_allclose(b["cost"], a["cost"], rtol=cost_rtol, atol=cost_atol)
        ts = trace_scale  # (1 unless the caller widened the state tolerance to the oracle's own spread)
        np.testing.assert_allclose(b["trust_region_radius"], a["trust_region_radius"], rtol=1e-6 * ts)
        np.testing.assert_allclose(b["mu"], a["mu"], rtol=1e-12)
        np.testing.assert_allclose(b["step_norm"], a["step_norm"], rtol=1e-5 * ts, atol=1e-9 * ts)
        np.testing.assert_allclose(b["relative_decrease"], a["relative_decrease"], rtol=1e-4 * ts, atol=1e-6 * ts)
        np.testing.assert_allclose(b["gradient_max_norm"], a["gradient_max_norm"], rtol=1e-5 * ts, atol=1e-7 * ts)
    for k in range(len(t0)):  # states after EVERY iteration
        np.testing.assert_allclose(sm1.trace_states[k], sm0.trace_states[k], rtol=0, atol=state_tol)
    np.testing.assert_allclose(st1.frame_state, st0.frame_state, rtol=0, atol=state_tol)
    np.testing.assert_allclose(st1.lm_inv_depth, st0.lm_inv_depth, rtol=0, atol=state_tol)
    np.testing.assert_allclose(sm1.initial_cost, sm0.initial_cost, rtol=1e-8)
    np.testing.assert_allclose(sm1.final_cost, sm0.final_cost, rtol=cost_rtol, atol=cost_atol)
    assert (st1.lm_valid == st0.lm_valid).all()
    np.testing.assert_allclose(st1.lm_quality, st0.lm_quality, rtol=0, atol=quality_atol)
    worst = max(np.abs(sm1.trace_states[k] - sm0.trace_states[k]).max() for k in range(len(t0)))
    return dict(worst_state_diff=worst, iterations=sm1.num_iterations, device_seconds=sm1.device_seconds)


def check_against_reference(ctx, ref, pb, state_tol=STATE_TOL):
    """A C-ABI solve against the REFERENCE'S OWN BundleAdjustorSolver::solve (oracle/_ref: bundle_adjustor.cpp + cost functions +
    map layer compiled unedited, mini-Ceres loop underneath): same accept / reject / termination trace, states after every
    iteration within north_star's 1e-6, landmark validity and quality of the post-solve pass."""
    fs, trk, rs = ref.solve(pb)
    st1, sm1 = ctx.solve(pb)
    M, N16 = pb.n_landmarks, 16 * pb.n_frames
    t0, t1 = rs.trace(), sm1.trace()
    assert (sm1.termination, sm1.num_iterations, sm1.num_successful_steps) == (rs.termination, rs.num_iterations, rs.num_successful_steps)
    assert len(t1) == len(t0)
    np.testing.assert_allclose(t1[0]["cost"], t0[0]["cost"], rtol=1e-12)  # same problem: the initial cost at rounding level
    worst = 0.0
    for k, (a, b) in enumerate(zip(t0, t1)):
        assert (a["step_is_valid"], a["step_is_successful"]) == (b["step_is_valid"], b["step_is_successful"]), (k, a, b)
        np.testing.assert_allclose(b["cost"], a["cost"], rtol=1e-5)
        np.testing.assert_allclose(b["trust_region_radius"], a["trust_region_radius"], rtol=1e-5)
        assert a["mu"] == b["mu"]
        worst = max(worst, np.abs(sm1.trace_states[k][:N16] - rs.trace_states[k][:N16]).max(),
                    np.abs(sm1.trace_states[k][N16:] - rs.trace_states[k][N16:N16 + M]).max() if M else 0.0)
    assert worst <= state_tol, worst
    np.testing.assert_allclose(st1.frame_state, fs, rtol=0, atol=state_tol)
    np.testing.assert_allclose(st1.lm_inv_depth, trk.inv_depth[:M], rtol=0, atol=state_tol)
    assert (st1.lm_valid == trk.valid[:M]).all()
    ok = st1.lm_valid.astype(bool)
    np.testing.assert_allclose(st1.lm_quality[ok], trk.quality[:M][ok], rtol=0, atol=1e-5)
    return dict(worst_state_diff=worst, iterations=sm1.num_iterations)
