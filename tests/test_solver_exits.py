"""Every exit of the trust-region loop (tests/solver_exits.py), not only the iteration limit: the C ABI -- in the fiber emulator and on the GPU (-m gpu) --
against the oracle, through the default context, linearize_mode = 2, reuse_identical_candidates, eager launches and the one-rank sharded path; one
context solving windows whose limits and exits differ from solve to solve; repeated resident solves of a window that converges; a poisoned device pool
under the split finalize's early stop.

  table   (oracle only) every row reaches the exit it is listed for and does not sit on a decision boundary
  rows    every row against the oracle, per form
  many    one context, ten solves with different limits and exits in sequence
  stale   (GPU) resident re-solves after a convergence exit; nothing read that an early stop left unwritten"""
import ctypes as C
import os
import subprocess
import time

import pytest

import ba_compare
import np_reference
import solver_exits as se
from pvio_amd import BAState, BASummary, capi
from pvio_amd.solver import HipContext

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu")
COST_RTOL = 1e-7  # check_against_oracle's own; also passed as cost_atol_rel (ba_compare: the same 1e-7 at the scale of the solve)

FORMS = {"default": dict(), "large_window_role": dict(linearize_mode=2), "reuse": dict(reuse_identical_candidates=True), "eager": dict(use_graph=False)}
ROWS = sorted(se.CASES)
FOUR_FRAME_ROWS = [n for n in ROWS if se.window_shape(n)[0] == 4]
# the 13-frame rows take 3 to 7 s each in the emulator: four of them on the CPU (one per exit that has a 13-frame row), the rest on the GPU only
GPU_ONLY = {n for n in ROWS if se.window_shape(n)[0] == 13} - {"parameter_rejections-vio_13_frames_global_matrix", "parameter_accepted-13x300",
                                                              "gradient_at_0-13x300", "gradient_accepted-13x300"}
# one row per exit through the sharded path (always the split finalize), the limit also from inside the invalid-step replay
SHARDED_ROWS = ["function-4x30", "parameter_accepted-4x25", "parameter_rejections-vio_partial", "gradient_at_0-4x25", "gradient_accepted-4x300", "limit_3-vio_small",
                "limit_0-vision_small", "fail8_limit_2-4x30", "invalid5_limit_6-4x300"]
TERMINATION = {np_reference.LIMIT: 1, np_reference.GRADIENT: 0, np_reference.PARAMETER: 0, np_reference.FUNCTION: 0, np_reference.INVALID_STEPS: 2}


class Contexts:
    """the four forms of a context on one library or device; a row with fault injection gets a context of its own (pvio_hip_opts::debug_* are set at
    creation), closed when the row is done"""

    def __init__(self, **base):
        self.base, self.plain = base, {}

    def make(self, form, case=None, **kw):
        return HipContext(**{**self.base, **FORMS[form], **kw}, debug_fail_factorizations=case.device_fail if case else 0, debug_invalid_steps=case.invalid if case else 0)

    def run(self, form, case, fn):
        if case.faulty:
            ctx = self.make(form, case)
            try:
                return fn(ctx)
            finally:
                ctx.close()
        if form not in self.plain:
            self.plain[form] = self.make(form)
        return fn(self.plain[form])

    def close(self):
        for c in self.plain.values():
            c.close()
        self.plain = {}


def check_row(ctxs, oracle, name, form):
    case, pb = se.CASES[name], se.window(oracle, name)
    with se.oracle_faults(case):
        return ctxs.run(form, case, lambda ctx: ba_compare.check_against_oracle(ctx, oracle, pb, cost_rtol=COST_RTOL, cost_atol_rel=COST_RTOL))


def check_sequence(ctx, oracle):
    out = []
    for entry in se.SEQUENCE:
        try:
            out.append(ba_compare.check_against_oracle(ctx, oracle, se.sequence_window(oracle, entry), cost_rtol=COST_RTOL, cost_atol_rel=COST_RTOL)["iterations"])
        except AssertionError as e:
            raise AssertionError("solve %d of the sequence, %r: %s" % (len(out), entry, e)) from None
    return out


def check_sharded(ctx, lib, oracle, name):
    case, pb = se.CASES[name], se.window(oracle, name)
    uid = (C.c_uint8 * 128)()
    assert lib.pvio_hip_comm_unique_id(uid) == 0 and lib.pvio_hip_comm_init(ctx.ctx, uid, 0, 1) == 0
    with se.oracle_faults(case):
        return ba_compare.check_against_oracle(ctx, oracle, pb, cost_rtol=COST_RTOL, cost_atol_rel=COST_RTOL)


def solved(ctx, pb):
    """everything a solve returns that must not depend on how it was launched or on what the device held before"""
    st, sm = ctx.solve(pb)
    t = sm.trace()
    return (st.frame_state.tobytes(), st.lm_inv_depth.tobytes(), st.lm_quality.tobytes(), st.lm_valid.tobytes(), sm.termination, sm.num_iterations, sm.num_successful_steps,
            sm.final_cost, tuple((x["cost"], x["step_is_valid"], x["step_is_successful"], x["trust_region_radius"], x["gradient_max_norm"]) for x in t),
            sm.trace_states[:len(t)].tobytes())


# ---- contexts ----

@pytest.fixture(scope="module")
def emu_lib():
    subprocess.check_call(["make", "-s", "-C", EMU_DIR, "libpvio_hipemu.so"])
    return capi.load(os.path.join(EMU_DIR, "libpvio_hipemu.so"))


@pytest.fixture(scope="module")
def emu(emu_lib):
    ctxs = Contexts(lib=emu_lib)
    yield ctxs
    ctxs.close()


@pytest.fixture(scope="module")
def gpu():
    ctxs = Contexts(device=0)  # raises without a GPU: no fallback
    yield ctxs
    ctxs.close()


# ---- table ----

_reference = {}
_table_seconds = [0.0]


def reference(oracle, name):
    """np_reference's solve of a row, once"""
    if name not in _reference:
        t_start = time.time()
        case = se.CASES[name]
        _reference[name] = np_reference.solve(se.window(oracle, name), oracle, fail_factorizations=case.fail, invalid_steps=case.invalid)
        _table_seconds[0] += time.time() - t_start
    return _reference[name]


@pytest.mark.parametrize("name", ROWS)
def test_row_reaches_its_exit_away_from_any_decision_boundary(oracle, name):
    """np_reference (independent of the oracle's loop) reports the listed reason; it and the oracle agree on termination, iterations and trace length; the
    oracle's four summation orders agree on those and on every accept / reject flag; the quantity that ends the solve clears its threshold by a factor of
    two (rejection tails: by 1 % on both sides, solver_exits' docstring says why no more can be asked of them)."""
    case, pb = se.CASES[name], se.window(oracle, name)
    r = reference(oracle, name)
    trace, _, _, term, iters = r
    assert r.reason == case.reason and term == TERMINATION[case.reason], (r.reason, term)
    orders = se.oracle_outcomes(oracle, case, pb)
    assert orders[0][:3] == (term, iters, len(trace)), (orders[0][:3], (term, iters, len(trace)))
    assert orders[0][3] == tuple((t["step_is_valid"], t["step_is_successful"]) for t in trace)
    assert all(o == orders[0] for o in orders[1:]), [o[:3] for o in orders]
    if r.deciding is not None:
        value, threshold = r.deciding
        print("%s: %s after %d iterations, %d records: %.3e against %.3e (1 / %.3g)" % (name, r.reason, iters, len(trace), value, threshold, threshold / max(value, 1e-300)))
        if case.tail:
            before = trace[-1]["step_norm"]  # the last step that did NOT end the solve: same x, same threshold
            assert not trace[-1]["step_is_successful"] and not trace[-2]["step_is_successful"], "not a rejection tail"
            assert abs(before / value - 2.0) < 1e-6, before / value
            assert value * 1.01 <= threshold and threshold * 1.01 <= before, (value, threshold, before)
        else:
            assert 2.0 * value <= threshold, (value, threshold)
    else:
        assert case.reason in (np_reference.LIMIT, np_reference.INVALID_STEPS)
        print("%s: %s after %d iterations, %d records" % (name, r.reason, iters, len(trace)))


def test_table_reaches_every_reachable_exit_on_both_sides_of_the_split(oracle):
    """exactly {limit, gradient, parameter, function, five invalid steps}; each of them with at most and with more than 256 landmarks (fused back-substitution
    | split finalize); gradient and parameter also on a 13-frame window.  (A change of synth that moves a row elsewhere fails here or in the row's own test.)"""
    _reached = {n: reference(oracle, n).reason for n in ROWS}
    print("np_reference on the %d rows: %.1f s" % (len(ROWS), _table_seconds[0]))
    assert set(_reached.values()) == se.REACHABLE
    for reason in se.REACHABLE:
        sizes = [se.window_shape(n)[1] for n in ROWS if _reached[n] == reason]
        assert min(sizes) <= 256 < max(sizes), (reason, sizes)
    for reason in (np_reference.GRADIENT, np_reference.PARAMETER):
        assert any(se.window_shape(n)[0] == 13 for n in ROWS if _reached[n] == reason), reason


# ---- rows, emulator ----

@pytest.mark.parametrize("name", [n for n in ROWS if n not in GPU_ONLY])
def test_emulated_row_matches_oracle(emu, oracle, name):
    print(name, check_row(emu, oracle, name, "default"))


@pytest.mark.parametrize("form", ["large_window_role", "reuse", "eager"])
@pytest.mark.parametrize("name", FOUR_FRAME_ROWS)
def test_emulated_four_frame_row_in_every_form(emu, oracle, name, form):
    print(name, form, check_row(emu, oracle, name, form))


@pytest.mark.parametrize("name", [n for n in SHARDED_ROWS if n not in GPU_ONLY])
def test_emulated_row_on_the_one_rank_sharded_path(emu_lib, oracle, name):
    """as test_emu_ba.test_emulated_one_rank_sharded_path: force_sharded with an identity all-reduce"""
    proto = C.CFUNCTYPE(C.c_int, C.POINTER(C.c_double), C.c_long, C.c_int)
    identity = proto(lambda buf, n, op_max: 0)
    emu_lib.hipemu_set_allreduce(identity)
    case = se.CASES[name]
    ctx = HipContext(lib=emu_lib, force_sharded=True, debug_fail_factorizations=case.device_fail, debug_invalid_steps=case.invalid)
    try:
        print(name, check_sharded(ctx, emu_lib, oracle, name))
    finally:
        ctx.close()
        emu_lib.hipemu_set_allreduce(C.cast(None, proto))


@pytest.mark.parametrize("form", sorted(FORMS))
def test_emulated_one_context_many_exits(emu, oracle, form):
    ctx = emu.make(form)
    try:
        print(form, check_sequence(ctx, oracle))
    finally:
        ctx.close()


# ---- rows, GPU ----

@pytest.mark.gpu
@pytest.mark.parametrize("form", ["default", "large_window_role", "reuse"])
@pytest.mark.parametrize("name", ROWS)
def test_gpu_row_matches_oracle(gpu, oracle, name, form):
    """(reuse: the iterations, the trace and the states are the oracle's, which evaluates every candidate)"""
    print(name, form, check_row(gpu, oracle, name, form))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ROWS)
def test_gpu_row_eager_equals_graph(gpu, oracle, name):
    """eager launches: against the oracle, and bit-identical to the replay of the captured graph -- whose slots past the exit are no-ops"""
    case, pb = se.CASES[name], se.window(oracle, name)
    print(name, check_row(gpu, oracle, name, "eager"))
    a = gpu.run("default", case, lambda ctx: solved(ctx, pb))
    b = gpu.run("eager", case, lambda ctx: solved(ctx, pb))
    assert a == b


@pytest.mark.gpu
@pytest.mark.parametrize("name", SHARDED_ROWS)
def test_gpu_row_on_the_one_rank_communicator(oracle, name):
    """as test_gpu_ba.test_gpu_one_rank_communicator_runs_the_sharded_path: a one-rank RCCL communicator carries the all-reduces"""
    lib = capi.load()
    case = se.CASES[name]
    ctx = HipContext(device=0, rank=0, world_size=1, force_sharded=True, debug_fail_factorizations=case.device_fail, debug_invalid_steps=case.invalid)
    try:
        print(name, check_sharded(ctx, lib, oracle, name))
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", sorted(FORMS))
def test_gpu_one_context_many_exits(gpu, oracle, form):
    """re-capture when max_iterations changes, k_reset of a control block that a convergence exit left done, the reuse state after an early stop"""
    ctx = gpu.make(form)
    try:
        print(form, check_sequence(ctx, oracle))
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["gradient_accepted-4x300", "gradient_accepted-4x25", "parameter_accepted-4x300", "function-4x30", "gradient_at_0-13x300"])
def test_gpu_resident_solve_repeats_after_a_convergence_exit(gpu, oracle, name):
    """upload once, solve three times: each solve starts from a control block the one before left done by a convergence exit, not by the limit"""
    pb = se.window(oracle, name)
    ctx = gpu.make("default")
    try:
        st1, sm1 = ctx.solve(pb)
        assert sm1.termination == 0 and sm1.num_iterations < pb.max_iterations
        ctx.upload(pb)
        for k in range(3):
            sm = BASummary(pb, trace=False)
            ctx.solve_resident(sm)
            st = BAState(pb)
            ctx.download(st)
            assert (sm.termination, sm.num_iterations, sm.num_successful_steps, sm.final_cost) == (sm1.termination, sm1.num_iterations, sm1.num_successful_steps, sm1.final_cost), k
            assert (st.frame_state == st1.frame_state).all() and (st.lm_inv_depth == st1.lm_inv_depth).all(), k
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("poison", [float("nan"), 1e300], ids=["nan", "1e300"])
@pytest.mark.parametrize("name", ["gradient_accepted-4x300", "parameter_accepted-4x300"])
def test_gpu_early_stop_reads_nothing_stale(oracle, name, poison):
    """backsub_finalize's gradient exit sets done while the landmark workgroups of its launch run: nothing may read back_part (or anything else the stopped
    iteration did not write) afterwards.  A fresh context on a device pool left full of NaN / 1e300 (test_gpu_ba's mechanism): bit-identical to a solve on
    clean memory, and the oracle's."""
    from test_gpu_ba import poison_device_memory
    pb = se.window(oracle, name)
    ctx = HipContext(device=0)
    try:
        clean = solved(ctx, pb)
    finally:
        ctx.close()
    poison_device_memory(poison)
    ctx = HipContext(device=0)
    try:
        assert solved(ctx, pb) == clean
    finally:
        ctx.close()
    poison_device_memory(poison)
    ctx = HipContext(device=0)
    try:
        ba_compare.check_against_oracle(ctx, oracle, pb, cost_rtol=COST_RTOL, cost_atol_rel=COST_RTOL)
    finally:
        ctx.close()
