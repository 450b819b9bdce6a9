"""pvio_hip_plane_ransac on the GPU: writes plane_ransac_timing.txt (wall time of the call, hipEvent times of k_plane_hypotheses and k_plane_refit
from pvio_hip_plane_ransac_stats, and the host-only form of pvio_amd/host/plane_ransac.cpp on the same box, for n = 300, 3000 and 50 000 at 1000
iterations with a plane of 20 % of the points -- no early stop --; mean of 50 calls after 5 warm-ups) and plane_parity.txt (per case of
tests/test_plane_ransac.py the observed fraction of each refit tolerance and the ulp distance of the RANSAC model from the restatement's).
usage: python tests/prof_plane_ransac.py [output directory, default profiles/] [calls]"""
import os, sys, tempfile, time
os.environ["PVIO_HIP_TIMING"] = "1"  # the library records the kernels' events only then (read once, at the first call)
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT); sys.path.insert(0, HERE)
import numpy as np
from pvio_amd.solver import HipContext
import plane_compare as PC, test_plane_ransac as TP

out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles")
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 50
os.makedirs(out_dir, exist_ok=True)
ctx = HipContext(device=0)
tmp = tempfile.TemporaryDirectory()
host = PC.build_host_form(tmp.name)

today = time.strftime("%Y-%m-%d")
lines = ["pvio_hip_plane_ransac on an MI355X, %s, written by tests/prof_plane_ransac.py (one process, PVIO_HIP_TIMING=1)." % today,
         "call: wall time of HipContext.plane_ransac (1000 samples drawn on the host, one H2D copy, k_plane_hypotheses, D2H of counts and models, synchronize,",
         "the replay, k_plane_refit, D2H of record and mask, synchronize, unpacking); kernels: hipEvent times from pvio_hip_plane_ransac_stats; host: the",
         "sequential host-only form (pvio_amd/host/plane_ransac.cpp, g++ -O2, one thread) through ctypes on the same box.  20 % of the points on a plane, 1 cm",
         "noise, threshold 0.03, confidence 0.999, 1000 iterations, seed 0: the ^5 rule never shortens the run.  Mean of %d calls after 5 warm-ups." % calls, ""]
def timed(points):
    for _ in range(5):
        res = ctx.plane_ransac(points)
    ms, t0 = np.zeros(2), time.perf_counter()
    for _ in range(calls):
        res = ctx.plane_ransac(points)
        ms += ctx.plane_ransac_stats()[1]
    return res, (time.perf_counter() - t0) / calls, ms

for n in (300, 3000, 50000):
    points = PC.make_points(n, planes=((0.2, 0.01),), seed=5000 + n)
    res, wall, ms = timed(points)
    host_calls = max(1, min(calls, 5 if n > 10000 else calls))
    h = PC.host_form(host, points)
    t0 = time.perf_counter()
    for _ in range(host_calls):
        h = PC.host_form(host, points)
    host_wall = (time.perf_counter() - t0) / host_calls
    assert (h["inlier_mask"] == res["inlier_mask"]).all() and h["iterations"] == res["iterations"] == 1000
    lines.append("n = %5d: %d inliers, %d iterations; call %.1f us   k_plane_hypotheses %.1f us   k_plane_refit %.1f us   host-only form %.1f us (mean of %d)   host / call %.1f"
                 % (n, res["n_inliers"], res["iterations"], 1e6 * wall, 1e3 * ms[0] / calls, 1e3 * ms[1] / calls, 1e6 * host_wall, host_calls, host_wall / wall))
    print(lines[-1], flush=True)

# A/B of the points one wave of k_plane_hypotheses scores (PVIO_HIP_PLANE_CHUNK, read at every call): 2^24 is the first form built, a hypothesis
# walked by ONE wave; 4096 is the default.  Same process, the settings alternating, two rounds.
lines += ["", "A/B, n = 50000, same process, settings alternating: PVIO_HIP_PLANE_CHUNK = points per wave of k_plane_hypotheses (16777216: one wave walks all",
          "points of a hypothesis, the first form built; 4096: the default).  Results are identical bit for bit (asserted).", ""]
points = PC.make_points(50000, planes=((0.2, 0.01),), seed=55000)
base = None
for rep in range(2):
    for chunk in (1 << 24, 16384, 4096, 1024):
        os.environ["PVIO_HIP_PLANE_CHUNK"] = str(chunk)
        res, wall, ms = timed(points)
        if base is None:
            base = res
        assert all(np.asarray(res[k]).tobytes() == np.asarray(base[k]).tobytes() for k in base)
        lines.append("round %d  chunk %8d: call %.1f us   k_plane_hypotheses %.1f us   k_plane_refit %.1f us" % (rep, chunk, 1e6 * wall, 1e3 * ms[0] / calls, 1e3 * ms[1] / calls))
        print(lines[-1], flush=True)
del os.environ["PVIO_HIP_PLANE_CHUNK"]
open(os.path.join(out_dir, "plane_ransac_timing.txt"), "w").write("\n".join(lines) + "\n")

rows = ["pvio_hip_plane_ransac on an MI355X, %s, against the numpy restatement (tests/plane_compare.py), written by tests/prof_plane_ransac.py." % today,
        "mask, n_inliers, iterations and best_iteration are identical in every case (asserted).  model ulp: largest distance of normal and distance from the",
        "restatement's bits.  cog, normal, distance: the refit's error over its tolerance (4 count eps max|p|; 4 count eps trace(cov) / (l1 - l0) + 16 eps;",
        "|cog| tol_normal + tol_cog + 4 eps |cog|), each computed from the restatement alone.", "",
        "%-22s %9s %10s %10s %12s" % ("case", "model ulp", "cog / tol", "normal / tol", "distance / tol")]
worst = dict(model_ulp=0, cog=0.0, normal=0.0, distance=0.0)
for name in sorted(TP.STRICT):
    fig = TP.run_two_planes(ctx) if name == "two_planes" else TP.run_strict(ctx, name)
    rows.append("%-22s %9d %10.3g %10.3g %12.3g" % (name, fig["model_ulp"], fig["cog"], fig["normal"], fig["distance"]))
    worst = {k: max(worst[k], fig[k]) for k in worst}
rows.append("%-22s %9d %10.3g %10.3g %12.3g" % ("largest", worst["model_ulp"], worst["cog"], worst["normal"], worst["distance"]))
open(os.path.join(out_dir, "plane_parity.txt"), "w").write("\n".join(rows) + "\n")
print("\n".join(rows))
