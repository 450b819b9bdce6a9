"""bench.py's host-side helpers (no GPU): workload names, the algorithmic-bytes figure of SURVEY section 8(d), and the rule that
`roofline.traffic` is only printed from a PMC summary that was collected on exactly the kernel sources in the tree; what a plain run
does next to --full, and --dump-outputs (one GPU test runs the plain line)."""
import json
import os
import shutil
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from pvio_amd import synth  # noqa: E402


def test_workload_names():
    assert bench.parse_workload("vio") == (10, 1000, True) and bench.parse_workload("vision") == (10, 1000, False)
    assert bench.parse_workload("30x50000_vio") == (30, 50000, True)
    assert bench.parse_workload("10X50000_vision") == (10, 50000, False)
    assert bench.parse_workload("8x200") == (8, 200, True)


def test_algorithmic_bytes_are_the_survey_formula():
    # 2 (20 F + 32 M) + 8 M + 8 (d N)^2 bytes per iteration; 612 000 at 10 x 1000 VIO (F = 9000 factors)
    pb = synth.make_window(n_frames=10, n_landmarks=1000, use_inertial=False)
    F, M, N = pb.n_obs, pb.n_landmarks, pb.n_frames
    assert synth.algorithmic_bytes_per_iteration(pb) == 2 * (20 * F + 32 * M) + 8 * M + 8 * (6 * N) ** 2
    assert 2 * (20 * 9000 + 32 * 1000) + 8 * 1000 + 8 * 150 ** 2 == 612000


def test_traffic_comes_from_counter_passes_of_the_run_or_is_null(monkeypatch):
    """`roofline.traffic` is measured inside the run (rocprofv3 child passes of bench.py itself) or null: nothing is read from a file
    committed earlier."""
    import argparse
    import inspect
    src = inspect.getsource(bench.live_pmc) + inspect.getsource(bench.pmc_traffic)
    assert "profiles/r" not in src and "_pmc_hbm" not in src and "glob" not in src
    args = argparse.Namespace(workload="vio", no_pmc=True)
    bench._PMC.update(done=False, kernels=None, note=None)
    assert bench.pmc_traffic("k_linearize", args) is None and bench._PMC["note"] == "rocprofv3 not run"
    bench._PMC.update(done=False, kernels=None, note=None)
    monkeypatch.setenv("PVIO_BENCH_NO_PMC", "1")
    assert bench.pmc_traffic("k_linearize", argparse.Namespace(workload="vio", no_pmc=False)) is None
    # a multi-GPU line never carries counters of one rank
    bench._PMC.update(done=True, kernels={"k_linearize": {"hbm_bytes_per_launch": 1.0}}, note="x")
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert bench.pmc_traffic("k_linearize", args) is None
    monkeypatch.setenv("WORLD_SIZE", "1")
    assert bench.pmc_traffic("k_linearize", args) == 1.0 and bench.pmc_traffic("k_nope", args) is None
    bench._PMC.update(done=False, kernels=None, note=None)


def test_dense_roofline_flops():
    # P^3 / 3 + 2 P^2 at P = 150: 1.17 Mflop per factoring launch; the FP64 peak quoted is the MI355X figure
    assert abs((150 ** 3 / 3.0 + 2.0 * 150 ** 2) - 1.17e6) < 1e4 and bench.FP64_PEAK_TFLOPS == 78.6


def test_bare_multi_gpu_invocation_becomes_a_one_rank_per_gpu_launch(monkeypatch):
    """`python bench.py --gpus 8` without a launcher ran on one GPU and printed "n_gpus": 8.  A bare --gpus N > 1 now re-executes
    itself under torch.distributed.run with N ranks (rendezvous on 127.0.0.1); a launcher's WORLD_SIZE that disagrees with the flag is an error;
    the printed n_gpus is the world size, not the flag."""
    import inspect
    import pytest
    calls = []

    class Stop(Exception):
        pass

    def fake_execv(exe, argv):
        calls.append((exe, argv))
        raise Stop()
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(os, "execv", fake_execv)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "7", "--warmup", "2"])
    with pytest.raises(Stop):
        bench.main()
    exe, argv = calls[0]
    assert exe == sys.executable and argv[1:3] == ["-m", "torch.distributed.run"]
    assert argv[argv.index("--nproc-per-node") + 1] == "4" and argv[argv.index("--master-addr") + 1] == "127.0.0.1"
    assert argv[-6:] == ["--gpus", "4", "--steps", "7", "--warmup", "2"] and argv[-7] == os.path.join(ROOT, "bench.py")
    # a launcher's world that disagrees with the flag: refused before anything touches a GPU
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert "does not match WORLD_SIZE" in str(e.value)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1"])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert "does not match WORLD_SIZE" in str(e.value)
    src = inspect.getsource(bench.main)
    assert '"n_gpus": world' in src and '"n_gpus": args.gpus' not in src


def _fake_solved(pb):
    """what bench.dump_outputs needs of a context and a summary, without a GPU: download() fills the state the way the library does"""
    class Ctx:
        def download(self, st):
            st.frame_state += 0.5
            st.lm_inv_depth *= 2.0
            st.lm_quality[:] = np.arange(len(st.lm_quality), dtype=np.float64)
            st.lm_valid[::3] = 0
            return st

    class Summary:
        num_iterations, num_successful_steps, initial_cost, final_cost, termination, is_usable = 7, 5, 12.5, 0.25, 1, 1
    return Ctx(), Summary()


def test_dump_outputs_writes_the_states_and_summary_as_float64(tmp_path):
    """--dump-outputs: the arrays a caller of the resident path receives (download + summary), float64 .npy, the landmarks complete"""
    pb = synth.make_window(n_frames=4, n_landmarks=30, use_inertial=False)
    ctx, sm = _fake_solved(pb)
    out = str(tmp_path / "out")
    bench.dump_outputs(out, ctx, pb, sm, 0, None)
    assert sorted(os.listdir(out)) == ["frame_state.npy", "lm_inv_depth.npy", "lm_quality.npy", "lm_valid.npy", "summary.npy"]
    a = {n[:-4]: np.load(os.path.join(out, n)) for n in os.listdir(out)}
    assert all(v.dtype == np.float64 for v in a.values())
    np.testing.assert_array_equal(a["frame_state"], np.asarray(pb.frame_state, np.float64) + 0.5)
    np.testing.assert_array_equal(a["lm_inv_depth"], 2.0 * np.asarray(pb.lm_inv_depth, np.float64))
    assert a["lm_quality"].shape == a["lm_valid"].shape == (pb.n_landmarks,) and a["lm_valid"].sum() == pb.n_landmarks - len(range(0, 30, 3))
    np.testing.assert_array_equal(a["summary"], [7, 5, 12.5, 0.25, 1, 1])
    # rank != 0 of a run without a process group writes nothing
    bench.dump_outputs(str(tmp_path / "r1"), ctx, pb, sm, 1, None)
    assert not os.path.exists(str(tmp_path / "r1"))


def test_dump_outputs_of_a_large_window_is_a_fixed_sample_within_the_limit(tmp_path, monkeypatch):
    pb = synth.make_window(n_frames=4, n_landmarks=400, use_inertial=False)
    limit = 8 * 4 * 16 + 8 * 4 * 100 + 1024  # frame_state + 100 landmarks x 4 arrays
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", limit)
    dirs = []
    for k in range(2):
        ctx, sm = _fake_solved(pb)
        dirs.append(str(tmp_path / ("d%d" % k)))
        bench.dump_outputs(dirs[-1], ctx, pb, sm, 0, None)
    total = sum(os.path.getsize(os.path.join(dirs[0], n)) - 128 for n in os.listdir(dirs[0]))  # .npy header: 128 bytes
    assert total <= limit
    idx = np.load(os.path.join(dirs[0], "lm_index.npy"))
    assert len(idx) == 100 and (np.diff(idx) > 0).all()
    np.testing.assert_array_equal(np.load(os.path.join(dirs[0], "lm_inv_depth.npy")), 2.0 * np.asarray(pb.lm_inv_depth)[idx.astype(int)])
    for n in os.listdir(dirs[0]):
        np.testing.assert_array_equal(np.load(os.path.join(dirs[0], n)), np.load(os.path.join(dirs[1], n)))


def test_plain_run_is_the_headline_only():
    """A plain run times the headline and prints it; every other leg runs behind --full (off by default)."""
    import inspect
    src = inspect.getsource(bench.main)
    for call in ("bench_roofline(", "bench_scaling_window(", "bench_klt(", "bench_concurrent_windows(", "bench_reference_window(",
                 "O.build()", "lib.pvio_hip_ba_solve(", "reuse_identical_candidates=True"):
        head = src[:src.index(call)]
        guard = head[head.rindex("\n    if "):]
        assert "args.full" in guard, call
    ap_src = src[src.index('"--full"'):]
    assert 'action="store_true"' in ap_src.split("\n")[0]


@pytest.mark.gpu
def test_plain_run_prints_one_line_and_dumps_the_same_outputs_twice(tmp_path):
    """bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR on the GPU: one JSON line with the headline fields and K steps,
    the --full objects null, float64 outputs; two runs with the same arguments write the same arrays."""
    import subprocess
    lines, dirs = [], []
    for k in range(2):
        dirs.append(str(tmp_path / ("run%d" % k)))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
                            "--dump-outputs", dirs[-1]], cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        out = r.stdout.decode().strip().splitlines()
        assert len(out) == 1
        lines.append(json.loads(out[0]))
    d = lines[0]
    assert d["metric"] == "BA iterations/sec" and d["unit"] == "iterations/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["value"] > 0
    assert abs(d["value"] - d["iterations_per_solve"] / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    for k in ("api", "identical_candidate_reuse", "roofline", "roofline_dense", "cpu_baseline", "klt", "concurrent_windows", "scaling_window", "reference_window"):
        assert d[k] is None, k
    names = sorted(os.listdir(dirs[0]))
    assert names == ["frame_state.npy", "lm_inv_depth.npy", "lm_quality.npy", "lm_valid.npy", "summary.npy"]
    assert sum(os.path.getsize(os.path.join(dirs[0], n)) for n in names) <= 64 << 20
    for n in names:
        a, b = np.load(os.path.join(dirs[0], n)), np.load(os.path.join(dirs[1], n))
        assert a.dtype == np.float64
        np.testing.assert_array_equal(a, b)
    summary = np.load(os.path.join(dirs[0], "summary.npy"))
    assert summary[0] == d["iterations_per_solve"] and summary[3] == d["final_cost"]
    assert np.load(os.path.join(dirs[0], "frame_state.npy")).shape == (10, 16)
    assert np.load(os.path.join(dirs[0], "lm_inv_depth.npy")).shape == (1000,)
