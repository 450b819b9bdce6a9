"""pvio_hip_triangulate on the GPU: writes triangulate_timing.txt (kernel time from pvio_hip_triangulate_stats and wall time of the call, mean of 50
calls after 5 warm-ups; the adapter's plane re-validation on tests/test_host_adapter.py's POST window with PVIO_HIP_DEVICE_TRIANGULATION off and on,
alternating fresh processes, four solves each) and triangulate_parity.txt (worst |q - q_ref| / tol_q and max_sweeps per case of
tests/test_triangulate.py).
usage: python tests/prof_triangulate.py [output directory, default profiles/] [calls]"""
import os, re, subprocess, sys, time
os.environ["PVIO_HIP_TIMING"] = "1"  # the library records the kernel's events only then (read once, at the first call)
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT); sys.path.insert(0, HERE)
import numpy as np
from pvio_amd.solver import HipContext
import tri_compare, test_triangulate as TT

out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles")
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 50
os.makedirs(out_dir, exist_ok=True)
ctx = HipContext(device=0)

today = time.strftime("%Y-%m-%d")
lines = ["pvio_hip_triangulate on an MI355X, %s, written by tests/prof_triangulate.py (one process, PVIO_HIP_TIMING=1)." % today,
         "call: wall time of HipContext.triangulate (staging, one H2D copy, one launch, one D2H copy, synchronize, unpacking); k_triangulate: hipEvent time",
         "of the kernel from pvio_hip_triangulate_stats.  Mean of %d calls after 5 warm-ups." % calls, ""]
for T, K in ((150, 10), (1000, 10), (3000, 11), (1000, 32), (1000, 16)):
    inp = tri_compare.make_tracks([K] * T, seed=7000 + T + K)
    for _ in range(5):
        tri_compare.call(ctx, inp)
    ms, t0 = 0.0, time.perf_counter()
    for _ in range(calls):
        tri_compare.call(ctx, inp)
        ms += ctx.triangulate_stats()[1]
    wall = (time.perf_counter() - t0) / calls
    lines.append("%d tracks x %d views (%d-lane groups), mean of %d calls: call %.1f us   k_triangulate %.1f us   max_sweeps %d"
                 % (T, K, 32 if K <= 16 else 64, calls, 1e6 * wall, 1e3 * ms / calls, ctx.triangulate_stats()[0]))
    print(lines[-1], flush=True)

# the adapter: re-validation time of the POST window, switch off (the host SVDs: the parent's path) and on, alternating processes
lines += ["", "The adapter's plane-track re-validation (pvio_amd/host/bundle_adjustor.cpp, its own PVIO_HIP_TIMING line) on the post-pass window of",
          "tests/test_host_adapter.py, same box, fresh processes alternating, four solves per process.  Switch 0 is the parent's path: one",
          "Track::try_triangulate (host SVD) per track.", ""]
child = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
         "import host_compare\nfrom oracle import oracle_py as O\nfrom test_host_adapter import POST\nO.build(); O.lib()\n"
         "lib = host_compare.load('libpvio_host.so')\n"
         "for _ in range(4): host_compare.check_adapter_post_passes(lib, O, **POST)\n") % (ROOT, HERE)
for rep in range(2):
    for switch in ("0", "1"):
        r = subprocess.run([sys.executable, "-c", child], capture_output=True, text=True, timeout=600, env=dict(os.environ, PVIO_HIP_DEVICE_TRIANGULATION=switch))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        m = re.findall(r"plane re-validation: ([0-9.]+) us, (\d+) tracks triangulated on the device", r.stderr)
        lines.append("adapter, POST window (12 x 200, 80 plane tracks), PVIO_HIP_DEVICE_TRIANGULATION=%s, process %d: re-validation of 4 solves %s us, tracks on the device %s"
                     % (switch, rep, " / ".join(x[0] for x in m), m[0][1]))
        print(lines[-1], flush=True)
open(os.path.join(out_dir, "triangulate_timing.txt"), "w").write("\n".join(lines) + "\n")

rows = ["pvio_hip_triangulate on an MI355X, %s, against numpy.linalg.svd (tests/tri_compare.py), written by tests/prof_triangulate.py." % today,
        "tol_q = max(8 K eps sigma_1 / (sigma_3 - sigma_4), 4 x the reference's spread over 8 one-ulp perturbations of view_P and obs_z), per track;",
        "|dq| / tol_q and |dp| / tol_p: the worst track's |q - q_ref| and |point - point_ref| over its own tolerance; max_sweeps: pvio_hip_triangulate_stats",
        "(the kernel's bound is %d)." % tri_compare.MAX_SWEEPS, "",
        "%-28s %7s %10s %10s %12s %14s %11s" % ("case", "tracks", "tol_q min", "tol_q max", "|dq| / tol_q", "|dp| / tol_p", "max_sweeps")]
def row(name, fig):
    rows.append("%-28s %7d %10.3g %10.3g %12.3g %14.3g %11d" % (name, fig["tracks"], fig.get("tol_q_min", 0), fig["tol_q_max"], fig["worst_q"], fig["worst_point"], fig["max_sweeps"]))
for K in TT.STRICT_K:
    for T in TT.STRICT_T + ((3000,) if K == 11 else ()):
        row("K=%d T=%d" % (K, T), TT.run_strict(ctx, K, T))
row("mixed K in {1,2,11,16,17,32}", TT.run_mixed(ctx))
row("low parallax (40 m, 2 views)", TT.run_low_parallax(ctx))
open(os.path.join(out_dir, "triangulate_parity.txt"), "w").write("\n".join(rows) + "\n")
print("\n".join(rows))
