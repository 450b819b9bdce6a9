"""pvio_hip_plane_ransac (include/pvio_hip.h; kernels in pvio_amd/csrc/ba_plane.hip, arithmetic in pv_plane.h) against the numpy restatement of
plane_compare.py: in the fiber emulator (tests/hipemu) and on the GPU (-m gpu).

Strict cases (plane_compare.margin >= 1e-9 from the restatement alone, asserted on the CPU): n = 3 (the third draw consumes no random number), 4,
63 / 64 / 65 (either side of a ballot word), 300 (the reference's window: 40 % of the points on a plane, 1 cm noise; seed 0 and 12345;
max_iterations 1000 and 1), 2049, 4161 (past the 4096 points one wave scores: a hypothesis' count is the sum of two waves' shares), and two
planes of different sizes (the larger wins).  Required: mask, n_inliers, iterations, best_iteration
identical; the RANSAC model the restatement's bits; the refit within the tolerances plane_compare computes from the restatement alone.
Then the quirks and edges: all points on one plane, a degenerate first sample, a NaN point, threshold 0, n = 0 / 1 / 2, the argument errors,
repeatability, no residue in a resident window, the device form against the host-only form (pvio_amd/host/plane_ransac.cpp), the golden
fixture recorded from the reference's own template.
CPU only: the pin against the reference itself (tests/host/plane_ref_harness.cpp above the reference's headers; skipped where they or a compiler
are absent) and the stand-alone sampler check (tests/host/plane_sampler_check.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import ba_compare
import plane_compare as PC
from pvio_amd import BASummary, capi, solver
from pvio_amd.solver import HipContext

assert "pvio_hip_plane_ransac" in capi.EXPORTS, "this module tests an entry point the package does not have"

HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "hipemu")

# name -> (make_points arguments, call arguments)
STRICT = {
    "n3": (dict(n=3, seed=103), {}),
    "n4": (dict(n=4, seed=104), {}),
    "n63": (dict(n=63, seed=163), {}),
    "n64": (dict(n=64, seed=164), {}),
    "n65": (dict(n=65, seed=165), {}),
    "n300": (PC.GOLDEN_CASE, {}),
    "n300_seed12345": (PC.GOLDEN_CASE, dict(seed=12345)),
    "n300_one_iteration": (PC.GOLDEN_CASE, dict(max_iterations=1)),
    "n2049": (dict(n=2049, seed=2149), {}),
    "n4161": (dict(n=4161, seed=4261), {}),  # past the 4096 points of one wave: two waves per hypothesis, the second with 65 points
    "two_planes": (dict(n=600, planes=((0.2, 0.01), (0.35, 0.01)), seed=600), {}),
}

_cache = {}


def strict_case(name):
    """(points, call arguments, restatement's result with its margin) of a strict case, computed once per session and shared, never written"""
    if name not in _cache:
        gen, kw = STRICT[name]
        points = PC.make_points(**gen)
        _cache[name] = (points, kw, PC.reference(points, want_margin=True, **kw))
    return _cache[name]


def run_strict(ctx, name):
    points, kw, ref = strict_case(name)
    res = ctx.plane_ransac(points, **kw)
    assert ctx.plane_ransac_stats()[0] == kw.get("max_iterations", 1000)  # every hypothesis is scored up front, in one launch
    return PC.compare(res, ref, strict=True, what=name)


def run_two_planes(ctx):
    fig = run_strict(ctx, "two_planes")
    gen, kw = STRICT["two_planes"]
    points, which = PC.make_points(labels=True, **gen)
    res = ctx.plane_ransac(points, **kw)
    on = res["inlier_mask"] == 1
    assert (which[on] == 1).sum() >= 0.9 * (which == 1).sum() and (which[on] == 0).sum() <= 0.2 * (which == 0).sum(), "the larger plane (35 %) wins over the smaller (20 %)"
    return fig


def run_one_plane(ctx):
    """all points on one plane: the first hypothesis holds them all, ratio 1 -> N = 0, the run ends after that iteration"""
    points = PC.make_points(200, planes=((1.0, 0.0),), seed=9)
    ref = PC.reference(points)
    res = ctx.plane_ransac(points)
    assert res["n_inliers"] == 200 and res["best_iteration"] == 0 and res["iterations"] == res["best_iteration"] + 1
    PC.compare(res, ref, strict=True, what="one plane")


def run_degenerate_sample(ctx):
    """n = 300, seed 0: the first sample is (0, 40, 227).  With point 40 a copy of point 0 the cross product is zero: a zero normal, distance 0,
    every point an inlier -- the reference's quirk -- and the run ends there.  The refit is still defined: the cloud's flattest direction, signed by
    its first non-zero component."""
    points = PC.make_points(**PC.GOLDEN_CASE)
    points[40] = points[0]
    ref = PC.reference(points)
    assert ref["first_sample"] == (0, 40, 227)
    res = ctx.plane_ransac(points)
    assert (res["normal"] == 0).all() and res["distance"] == 0 and res["n_inliers"] == 300 and (res["inlier_mask"] == 1).all()
    assert res["iterations"] == 1 and res["best_iteration"] == 0 and res["refit_valid"] == 1
    PC.compare(res, ref, strict=True, what="degenerate first sample")
    first = res["refit_normal"][res["refit_normal"] != 0][0]
    assert first > 0


def run_nan_point(ctx):
    """point 40 (in the first sample of seed 0) has a NaN coordinate: never an inlier; hypothesis 0 has no inlier at all; every other hypothesis is untouched"""
    points = PC.make_points(**PC.GOLDEN_CASE)
    clean = PC.reference(points)
    points[40, 1] = np.nan
    ref = PC.reference(points)
    res = ctx.plane_ransac(points)
    PC.compare(res, ref, strict=True, what="NaN point")
    assert res["inlier_mask"][40] == 0 and res["n_inliers"] >= clean["n_inliers"] - 1 > 30
    one = ctx.plane_ransac(points, max_iterations=1)  # only the poisoned hypothesis
    assert one["n_inliers"] == 0 and one["best_iteration"] == -1 and one["iterations"] == 1 and one["refit_valid"] == 0
    assert (one["inlier_mask"] == 0).all() and (one["normal"] == 0).all() and one["distance"] == 0


def run_threshold_zero(ctx):
    """only points whose error is exactly 0 count; the three implementations are one sequence of IEEE operations, so they agree on those too"""
    points = PC.make_points(**PC.GOLDEN_CASE)
    ref = PC.reference(points, threshold=0.0)
    res = ctx.plane_ransac(points, threshold=0.0)
    PC.compare(res, ref, strict=True, what="threshold 0")
    assert res["n_inliers"] <= 3
    if res["n_inliers"]:
        assert (PC.errors(points, res["normal"], res["distance"])[res["inlier_mask"] == 1] == 0).all()
    assert res["refit_valid"] == (1 if res["n_inliers"] >= 3 else 0)


def run_tiny(ctx):
    for n in (0, 1, 2):
        res = ctx.plane_ransac(np.arange(3.0 * n).reshape(n, 3))  # PVIO_OK: HipContext raises on anything else
        assert res["n_inliers"] == 0 and res["iterations"] == 0 and res["best_iteration"] == -1 and res["refit_valid"] == 0
        assert res["inlier_mask"].shape == (n,) and (res["inlier_mask"] == 0).all()
        assert (res["normal"] == 0).all() and res["distance"] == 0 and (res["refit_normal"] == 0).all() and res["refit_distance"] == 0 and (res["reference_point"] == 0).all()
        assert ctx.plane_ransac_stats()[0] == 0
    pb, out = capi.PlaneProblemC(), capi.PlaneResultC()  # NULL arrays are fine when there is no point
    pb.n_points, pb.max_iterations, pb.threshold, pb.confidence = 0, 1000, 0.03, 0.999
    assert ctx.lib.pvio_hip_plane_ransac(ctx.ctx, C.byref(pb), C.byref(out)) == 0 and out.best_iteration == -1
    assert ctx.lib.pvio_hip_plane_ransac_stats(ctx.ctx, None, None) == 0  # the optional arguments


def run_argument_errors(ctx):
    points = PC.make_points(**PC.GOLDEN_CASE)
    n = len(points)
    mask = np.full(n, 77, np.uint8)
    sentinel = -12345.0

    def rc(edit_pb=None, edit_out=None, expect_untouched=True):
        pb, out = capi.PlaneProblemC(), capi.PlaneResultC()
        pb.n_points, pb.max_iterations, pb.points = n, 1000, points.ctypes.data_as(capi.c_double_p)
        pb.threshold, pb.confidence, pb.seed = 0.03, 0.999, 0
        out.n_inliers = out.iterations = out.best_iteration = out.refit_valid = 77
        out.inlier_mask = mask.ctypes.data_as(capi.c_uint8_p)
        out.distance = out.refit_distance = sentinel
        for k in range(3):
            out.normal[k] = out.refit_normal[k] = out.reference_point[k] = sentinel
        if edit_pb:
            edit_pb(pb)
        if edit_out:
            edit_out(out)
        code = ctx.lib.pvio_hip_plane_ransac(ctx.ctx, C.byref(pb), C.byref(out))
        if expect_untouched:
            assert (mask == 77).all() and out.n_inliers == out.iterations == out.best_iteration == out.refit_valid == 77
            assert out.distance == out.refit_distance == sentinel and all(v == sentinel for v in list(out.normal) + list(out.refit_normal) + list(out.reference_point))
        return code, out

    INVALID = -1  # PVIO_ERR_INVALID_ARGUMENT
    assert ctx.lib.pvio_hip_plane_ransac(ctx.ctx, None, None) == INVALID
    pb = capi.PlaneProblemC()
    assert ctx.lib.pvio_hip_plane_ransac(ctx.ctx, C.byref(pb), None) == INVALID
    assert rc(edit_pb=lambda p: setattr(p, "points", None))[0] == INVALID
    assert rc(edit_out=lambda o: setattr(o, "inlier_mask", None))[0] == INVALID
    for bad_n in (-1, (1 << 24) + 1):
        assert rc(edit_pb=lambda p, v=bad_n: setattr(p, "n_points", v))[0] == INVALID
    for bad_it in (0, -5, 4097):
        assert rc(edit_pb=lambda p, v=bad_it: setattr(p, "max_iterations", v))[0] == INVALID
    for bad_thr in (-1e-3, np.inf, -np.inf, np.nan):
        assert rc(edit_pb=lambda p, v=bad_thr: setattr(p, "threshold", v))[0] == INVALID
    assert rc(edit_pb=lambda p: setattr(p, "confidence", np.nan))[0] == INVALID
    assert b"plane_ransac" in ctx.lib.pvio_hip_last_error(ctx.ctx)
    # ... and the same arguments unedited are accepted and written; so is the largest iteration count
    code, out = rc(expect_untouched=False)
    assert code == 0 and out.n_inliers > 30 and set(np.unique(mask)) == {0, 1}
    assert rc(edit_pb=lambda p: setattr(p, "max_iterations", 4096), expect_untouched=False)[0] == 0


def run_repeat_and_residue(ctx, oracle):
    points, kw, _ = strict_case("n2049")
    a, b = ctx.plane_ransac(points, **kw), ctx.plane_ransac(points, **kw)
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), "%s differs between two calls on the same input" % k
    pb = ba_compare.make(oracle, **ba_compare.CASES["vio_rot_prior"])
    ctx.upload(pb)
    sm0 = ctx.solve_resident(BASummary(pb))
    st0 = ctx.download(solver.BAState(pb))
    ctx.plane_ransac(points, **kw)
    sm1 = ctx.solve_resident(BASummary(pb))
    st1 = ctx.download(solver.BAState(pb))
    assert (st0.frame_state == st1.frame_state).all() and (st0.lm_inv_depth == st1.lm_inv_depth).all()
    t0, t1 = sm0.trace(), sm1.trace()
    assert len(t0) == len(t1) and all(x == y for x, y in zip(t0, t1)), "a plane RANSAC call leaves a residue in the next resident solve"
    assert sm0.final_cost == sm1.final_cost and sm0.initial_cost == sm1.initial_cost and sm0.num_iterations == sm1.num_iterations


def run_against_host_form(ctx, host_lib):
    for name in ("n3", "n65", "n300", "n300_seed12345", "n2049", "n4161", "two_planes"):
        points, kw, ref = strict_case(name)
        dev, host = ctx.plane_ransac(points, **kw), PC.host_form(host_lib, points, **kw)
        assert (dev["inlier_mask"] == host["inlier_mask"]).all(), name
        for k in ("n_inliers", "iterations", "best_iteration", "refit_valid"):
            assert dev[k] == host[k], (name, k)
        assert PC.ulp_diff(np.append(dev["normal"], dev["distance"]), np.append(host["normal"], host["distance"])) == 0, name
        PC.compare(host, ref, strict=True, what="host form " + name)  # the refits differ only in the order of their sums


def run_golden(ctx):
    """what the reference's own template returned for the n = 300 case (recorded: tests/golden/plane_ransac_300.npz)"""
    g = np.load(PC.GOLDEN)
    res = ctx.plane_ransac(g["points"], threshold=float(g["threshold"]), confidence=float(g["confidence"]), max_iterations=int(g["max_iterations"]), seed=int(g["seed"]))
    assert res["n_inliers"] == int(g["inlier_count"]) and (res["inlier_mask"] == g["inlier_mask"]).all()
    assert np.abs(res["normal"] - g["normal"]).max() <= 1e-12 and abs(res["distance"] - float(g["distance"])) <= 1e-12


# ---- the restatement alone (no kernels) ----

@pytest.mark.parametrize("name", sorted(STRICT))
def test_strict_cases_have_a_margin(name):
    _, _, ref = strict_case(name)
    print(name, "margin %.3g, n_inliers %d, iterations %d, first sample %s" % (ref["margin"], ref["n_inliers"], ref["iterations"], ref["first_sample"]))
    assert ref["margin"] >= PC.STRICT_MARGIN


def test_restated_sampler_first_samples():
    assert tuple(PC.Sampler(300, 0).sample()) == (0, 40, 227)
    s = PC.Sampler(3, 0)
    assert sorted(s.sample()) == [0, 1, 2] and s.x == 16807 * 16807 % PC.M31  # two numbers drawn, none for the last lot
    assert strict_case("n300")[2]["n_inliers"] > 30 and strict_case("n300")[2]["iterations"] < 1000  # 40 %: the ^5 rule shortens the run
    assert strict_case("two_planes")[2]["iterations"] == 1000                                        # 35 %: it does not


def test_sampler_equals_the_standard_library(tmp_path):
    """pv_plane.h's PlMinstd / pl_uniform / PlSampler against std::default_random_engine + std::uniform_int_distribution<size_t>, stand-alone program"""
    if shutil.which("g++") is None:
        pytest.skip("no compiler")
    exe = str(tmp_path / "plane_sampler_check")
    subprocess.check_call(["g++"] + PC.CXXFLAGS + ["-w", "-o", exe, os.path.join(HERE, "host", "plane_sampler_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "OK: 0 differing indices" in r.stdout and "n 300 seed 0 first sample 0 40 227" in r.stdout


@pytest.fixture(scope="module")
def ref_harness(tmp_path_factory):
    if not PC.reference_available():
        pytest.skip("the reference's headers or a compiler are absent")
    return PC.build_ref_harness(tmp_path_factory.mktemp("plane_ref"))


@pytest.mark.parametrize("name", sorted(STRICT))
def test_restatement_equals_the_reference_template(ref_harness, name):
    """pvio::Ransac<3, PlaneState, PlaneSolver, PlaneEvaluator> itself, header-only, on the strict cases' points"""
    points, kw, ref = strict_case(name)
    out = PC.run_ref_harness(ref_harness, points, **kw)
    assert out["inlier_count"] == ref["n_inliers"] and (out["inlier_mask"] == ref["inlier_mask"]).all()
    assert np.abs(out["normal"] - ref["normal"]).max() <= 1e-12 and abs(out["distance"] - ref["distance"]) <= 1e-12


def test_golden_fixture_equals_a_fresh_run_of_the_reference(ref_harness):
    g, fresh = np.load(PC.GOLDEN), PC.golden_run(ref_harness)
    assert sorted(g.files) == sorted(fresh)
    for k in g.files:
        assert np.array_equal(g[k], fresh[k]), k


def test_extract_plane_applies_the_reference_rule(host_lib):
    """extract_plane = plane_ransac + the `> 30` rule of plane_extractor.cpp:58 + the inlier indices"""
    points, _, ref = strict_case("n300")
    idx, d, cnt = np.zeros(len(points), np.int64), np.zeros(7), C.c_int32(0)
    f64p, i64p = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    found = host_lib.host_extract_plane(C.c_int(len(points)), points.ctypes.data_as(f64p), C.c_int(30), C.byref(cnt), idx.ctypes.data_as(i64p), d.ctypes.data_as(f64p))
    assert found == 1 and cnt.value == ref["n_inliers"] and (idx[:cnt.value] == np.flatnonzero(ref["inlier_mask"])).all()
    assert np.linalg.norm(d[0:3] - ref["refit_normal"]) <= ref["tol_normal"] and abs(d[3] - ref["refit_distance"]) <= ref["tol_distance"]
    assert np.abs(d[4:7] - ref["reference_point"]).max() <= ref["tol_cog"]
    found = host_lib.host_extract_plane(C.c_int(len(points)), points.ctypes.data_as(f64p), C.c_int(ref["n_inliers"]), C.byref(cnt), idx.ctypes.data_as(i64p), d.ctypes.data_as(f64p))
    assert found == 0 and cnt.value == 0  # not MORE than the bar


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    return PC.build_host_form(tmp_path_factory.mktemp("plane_host"))


# ---- emulator ----

@pytest.fixture(scope="module")
def emu_ctx():
    subprocess.check_call(["make", "-s", "-C", EMU_DIR, "libpvio_hipemu.so"])
    ctx = HipContext(lib=capi.load(os.path.join(EMU_DIR, "libpvio_hipemu.so")), use_graph=True)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("name", sorted(set(STRICT) - {"two_planes"}))
def test_emulated_plane_ransac(emu_ctx, name):
    run_strict(emu_ctx, name)


def test_emulated_plane_ransac_two_planes(emu_ctx):
    run_two_planes(emu_ctx)


def test_emulated_plane_ransac_one_plane(emu_ctx):
    run_one_plane(emu_ctx)


def test_emulated_plane_ransac_degenerate_sample(emu_ctx):
    run_degenerate_sample(emu_ctx)


def test_emulated_plane_ransac_nan_point(emu_ctx):
    run_nan_point(emu_ctx)


def test_emulated_plane_ransac_threshold_zero(emu_ctx):
    run_threshold_zero(emu_ctx)


def test_emulated_plane_ransac_fewer_than_three_points(emu_ctx):
    run_tiny(emu_ctx)


def test_emulated_plane_ransac_argument_errors(emu_ctx):
    run_argument_errors(emu_ctx)


def test_emulated_plane_ransac_repeats_and_leaves_no_residue(emu_ctx, oracle):
    run_repeat_and_residue(emu_ctx, oracle)


def test_emulated_plane_ransac_equals_the_host_form(emu_ctx, host_lib):
    run_against_host_form(emu_ctx, host_lib)


def test_emulated_plane_ransac_golden(emu_ctx):
    run_golden(emu_ctx)


# ---- GPU ----

@pytest.fixture(scope="module")
def gpu_ctx():
    ctx = HipContext(device=0, use_graph=True)  # raises without a GPU: no fallback
    yield ctx
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(set(STRICT) - {"two_planes"}))
def test_gpu_plane_ransac(gpu_ctx, name):
    run_strict(gpu_ctx, name)


@pytest.mark.gpu
def test_gpu_plane_ransac_two_planes(gpu_ctx):
    run_two_planes(gpu_ctx)


@pytest.mark.gpu
def test_gpu_plane_ransac_one_plane(gpu_ctx):
    run_one_plane(gpu_ctx)


@pytest.mark.gpu
def test_gpu_plane_ransac_degenerate_sample(gpu_ctx):
    run_degenerate_sample(gpu_ctx)


@pytest.mark.gpu
def test_gpu_plane_ransac_nan_point(gpu_ctx):
    run_nan_point(gpu_ctx)


@pytest.mark.gpu
def test_gpu_plane_ransac_threshold_zero(gpu_ctx):
    run_threshold_zero(gpu_ctx)


@pytest.mark.gpu
def test_gpu_plane_ransac_fewer_than_three_points(gpu_ctx):
    run_tiny(gpu_ctx)


@pytest.mark.gpu
def test_gpu_plane_ransac_argument_errors(gpu_ctx):
    run_argument_errors(gpu_ctx)


@pytest.mark.gpu
def test_gpu_plane_ransac_repeats_and_leaves_no_residue(gpu_ctx, oracle):
    run_repeat_and_residue(gpu_ctx, oracle)


@pytest.mark.gpu
def test_gpu_plane_ransac_equals_the_host_form(gpu_ctx, host_lib):
    run_against_host_form(gpu_ctx, host_lib)


@pytest.mark.gpu
def test_gpu_plane_ransac_golden(gpu_ctx):
    run_golden(gpu_ctx)
