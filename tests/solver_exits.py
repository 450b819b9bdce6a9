"""Windows that leave the trust-region loop through each of its exits (tests/test_solver_exits.py), next to ba_compare.py and window_variants.py.

Every window of ba_compare.CASES / BIG_CASES and of the random sweep runs into max_iterations = 10.  A sliding-window estimator in steady state
converges before its limit most of the time; the rows below reach

  limit          iteration >= max_iterations, at the top of the loop -- also from inside the invalid-step replay (a failed factorization or an invalid
                 step sends the loop back to its top without a candidate), which at max_iterations = 10 the five-strikes rule always pre-empts
  gradient       the gradient max-norm of an ACCEPTED iterate <= 1e-10 (at iteration 0: of the initial point)
  parameter      step norm <= 1e-8 (|x| + 1e-8): ends the solve inside an iteration, no trace record for it, the candidate is not applied
  function       |cost change| <= 1e-6 cost: the same
  invalid_steps  five invalid steps in a row (FAILURE), by fault injection only

np_reference's sixth exit, the minimum trust-region radius (1e-32), has no row: it needs about 150 consecutive rejections, each with a step that is
still above the parameter tolerance, and the parameter tolerance fires near radius 1e-5 on every valid input tried.  It is unreachable and untested.

Sizes: 25 / 30 landmarks take k_dense's fused back-substitution, 300 (> PVIO_HIP_FUSE_BACKSUB_MAX = 256) the split finalize of k_backsub; 13
inertial frames put the reduced matrix in HBM.

A row must not sit on a decision boundary (the kernels sum in another order than the oracle): tests/test_solver_exits.py checks every row on the
CPU -- np_reference gives the reason listed here, np_reference and the oracle agree on termination / iterations / trace length, the oracle's four
summation orders agree with each other, and the quantity that ends the solve clears its threshold by a factor of two.  noise_free(4 x 300,
perturb=True) with the weights scaled by 1e-3 fails that (gradient 8.8e-11 against 1e-10) and is not here; at 1e-4 it is (8.8e-13).

REJECTION TAILS.  The inertial windows of ba_compare.CASES at max_iterations = 60 end on the parameter tolerance after about 30 rejected steps in a
row (the live-bias quirk).  A rejection leaves x, and with it the threshold 1e-8 (|x| + 1e-8), where it is and halves the radius; the step of such a
tail is the scaled gradient cut to the radius, so its norm halves exactly from one iteration to the next (seen: 2 to nine digits on all five; asserted to six).  The norm v
that ends the solve therefore follows a norm 2 v that did not: thr / 2 < v <= thr, and NO such row can clear its threshold by a factor of two -- the
best a tail can do is a factor sqrt(2) on both sides.  These rows (Case.tail) are the only ones that take the device through a long run of rejections
into a convergence exit, so they stay, marked, with the check that can be made of them: check_against_oracle holds the device's step norms to 1e-5
of the oracle's, and a tail row must keep 1000 times that, 1 %, between its threshold and BOTH the norm that ends the solve and the one before it
(measured: 1.3 % .. 93 % below, 3.6 % .. 97 % above).  Every other row is held to the factor of two."""
import contextlib
import ctypes as C

import ba_compare
from np_reference import FUNCTION, GRADIENT, INVALID_STEPS, LIMIT, PARAMETER
from pvio_amd import BAState, BASummary, synth

REACHABLE = {LIMIT, GRADIENT, PARAMETER, FUNCTION, INVALID_STEPS}
NEGATIVE_PIVOT = 1000  # pvio_hip_opts::debug_fail_factorizations = 1000 + n: the factorizations MEET a negative pivot (tests/test_emu_ba.py)


def noise_free(pb, perturb):
    """pb with every observation and every anchor bearing re-projected from the truth geometry (in place; returns pb).  perturb = False: pb was made
    with make_window(perturb=False) -- the initial guess is the truth, the inverse depths become the exact ones: zero residual, a fixed point.
    perturb = True: the perturbed initial guess stays, the solve converges to zero cost."""
    pts = pb.meta["points"]
    R_bc = synth.qmat(pb.cam_extrinsic[0, :4])

    def bearing(f, l):
        Rw = synth.qmat(pb.truth_frame_state[f, :4]) @ R_bc
        pw = pb.truth_frame_state[f, 4:7] + synth.qmat(pb.truth_frame_state[f, :4]) @ pb.cam_extrinsic[f, 4:7]
        return Rw.T @ (pts[l] - pw)

    for l in range(pb.n_landmarks):
        for o in range(pb.lm_obs_ptr[l], pb.lm_obs_ptr[l + 1]):
            y = bearing(pb.obs_frame[o], l)
            pb.obs_z[o] = y[:2] / y[2]
        y = bearing(pb.lm_anchor_frame[l], l)
        pb.lm_anchor_z[l] = y[:2] / y[2]
        if not perturb:
            pb.lm_inv_depth[l] = 1.0 / y[2]
    return pb


def scale_weights(pb, s):
    pb.sqrt_inv_cov *= s
    return pb


def _named(name):
    return lambda oracle: ba_compare.make(oracle, **ba_compare.CASES[name])


def _noise_free(perturb, scale, **kw):
    return lambda oracle: scale_weights(noise_free(synth.make_window(perturb=perturb, **kw), perturb), scale)


def _vision(seed, **kw):
    return lambda oracle: synth.make_window(seed=seed, **kw)


def _fault_window(n_landmarks):
    return lambda oracle: ba_compare.make(oracle, n_frames=4, n_landmarks=n_landmarks, use_inertial=True)


class Case:
    def __init__(self, name, build, max_iterations, reason, fail=0, invalid=0, hook=False, tail=False):
        self.name, self.build, self.max_iterations, self.reason, self.tail = name, build, max_iterations, reason, tail
        self.fail, self.invalid, self.hook = fail, invalid, hook  # fault injection; hook: the device meets a negative pivot instead of discarding a result

    @property
    def device_fail(self):
        return self.fail + (NEGATIVE_PIVOT if self.hook else 0)

    @property
    def faulty(self):
        return bool(self.fail or self.invalid)


_NF = {"4x25": dict(n_frames=4, n_landmarks=25), "4x300": dict(n_frames=4, n_landmarks=300), "13x300": dict(n_frames=13, n_landmarks=300, visibility=5)}

_ROWS = []
# vision-only windows of make_window's other seeds: 13, 25 and 22 iterations, |cost change| at 1 / 2.66, 1 / 2.26 and 1 / 2.48 of its threshold at the exit.
# (ba_compare's vision_small and vision_rot_prior at 60 iterations end on the function tolerance too, after 17 and 38 iterations -- at 1 / 1.19 and
# 1 / 1.32: inside the factor of two, so they are not rows.  Of 15 seeds each of six shapes these three and one at 2.09 clear it.)
_ROWS += [Case("function-%s" % n, _vision(seed, **kw), 60, FUNCTION) for n, seed, kw in (
    ("4x30", 11, dict(n_frames=4, n_landmarks=30)), ("4x300", 2, dict(n_frames=4, n_landmarks=300)), ("6x300", 14, dict(n_frames=6, n_landmarks=300, visibility=3)))]
# after about 30 rejected steps (the live-bias quirk: all but two steps are rejected) -- see REJECTION TAILS above
_ROWS += [Case("parameter_rejections-%s" % n, _named(n), 60, PARAMETER, tail=True)
          for n in ("vio_small", "vio_partial", "vio_plane", "vio_rot_prior", "vio_13_frames_global_matrix")]
_ROWS += [Case("parameter_at_1-%s" % n, _noise_free(False, 1.0, **_NF[n]), 60, PARAMETER) for n in ("4x25", "4x300")]
_ROWS += [Case("parameter_accepted-%s" % n, _noise_free(True, 1.0, **_NF[n]), 60, PARAMETER) for n in ("4x25", "4x300", "13x300")]
_ROWS += [Case("gradient_at_0-%s" % n, _noise_free(False, 1e-2, **_NF[n]), 60, GRADIENT) for n in ("4x25", "4x300", "13x300")]
_ROWS += [Case("gradient_accepted-%s" % n, _noise_free(True, 1e-4, **_NF[n]), 60, GRADIENT) for n in ("4x25", "4x300", "13x300")]
_ROWS += [Case("limit_%d-%s" % (k, n), _named(n), k, LIMIT) for n in ("vision_small", "vio_small", "vio_13_frames_global_matrix") for k in (0, 1, 3)]
_ROWS += [Case("limit_60-plane", _named("plane"), 60, LIMIT)]
# the limit from inside the invalid-step replay; at 6 the fifth strike comes first
for _m in (30, 300):
    for _k in (1, 2, 3, 4, 6):
        _ROWS += [Case("fail8_limit_%d-4x%d" % (_k, _m), _fault_window(_m), _k, LIMIT if _k < 6 else INVALID_STEPS, fail=8),
                  Case("invalid5_limit_%d-4x%d" % (_k, _m), _fault_window(_m), _k, LIMIT if _k < 6 else INVALID_STEPS, invalid=5)]
    for _k in (1, 3):
        _ROWS += [Case("fail3_limit_%d-4x%d" % (_k, _m), _fault_window(_m), _k, LIMIT, fail=3), Case("invalid2_limit_%d-4x%d" % (_k, _m), _fault_window(_m), _k, LIMIT, invalid=2)]
# (the 30-landmark form of k_dense has no negative-pivot hook: tests/test_emu_ba.py)
_ROWS += [Case("pivot8_limit_%d-4x300" % k, _fault_window(300), k, LIMIT if k < 6 else INVALID_STEPS, fail=8, hook=True) for k in (1, 2, 3, 4, 6)]

CASES = {c.name: c for c in _ROWS}
assert len(CASES) == len(_ROWS)

_cache = {}


def window(oracle, name):
    """the row's problem with its max_iterations; built once, never edited"""
    if name not in _cache:
        pb = CASES[name].build(oracle)
        pb.max_iterations = CASES[name].max_iterations
        _cache[name] = pb
    return _cache[name]


def with_limit(oracle, name, max_iterations):
    """the window of ba_compare.CASES[name] at another iteration limit (the many-exits sequence)"""
    key = ("limit", name, max_iterations)
    if key not in _cache:
        pb = ba_compare.make(oracle, **ba_compare.CASES[name])
        pb.max_iterations = max_iterations
        _cache[key] = pb
    return _cache[key]


def window_shape(name):
    """(frames, landmarks) of a row, from its name or its ba_compare entry -- without building it"""
    tail = name.rsplit("-", 1)[1]
    if tail in ba_compare.CASES:
        return ba_compare.CASES[tail]["n_frames"], ba_compare.CASES[tail]["n_landmarks"]
    n, m = tail.split("x")
    return int(n), int(m)


@contextlib.contextmanager
def oracle_faults(case):
    """the oracle with the row's fault injection (oracle_debug_fault_injection: re-armed at every solve)"""
    from oracle import oracle_py
    L = oracle_py.lib()
    L.oracle_debug_fault_injection(C.c_int32(case.fail), C.c_int32(case.invalid))
    try:
        yield
    finally:
        L.oracle_debug_fault_injection(C.c_int32(0), C.c_int32(0))


def oracle_outcomes(oracle, case, pb):
    """(termination, iterations, trace length, accept / reject sequence) of the oracle under each of its four summation orders"""
    out = []
    with oracle_faults(case):
        try:
            for order in (0, 1, 2, 3):
                oracle.set_sum_order(order)
                st, sm = BAState(pb), BASummary(pb)
                oracle.solve(pb, st, sm)
                t = sm.trace()
                out.append((sm.termination, sm.num_iterations, len(t), tuple((x["step_is_valid"], x["step_is_successful"]) for x in t)))
        finally:
            oracle.set_sum_order(0)
    return out


# one context, many exits in sequence: (window of ba_compare.CASES or a row of CASES, max_iterations or None for the row's own)
SEQUENCE = [("vio_small", 10), ("vio_small", 60), ("vio_small", 3), ("vision_small", 60), ("vision_small", 0), ("vio_partial", 10),
            ("gradient_at_0-4x25", None), ("vision_small", 60), ("vio_small", 1), ("vio_small", 60)]


def sequence_window(oracle, entry):
    name, k = entry
    return window(oracle, name) if k is None else with_limit(oracle, name, k)
