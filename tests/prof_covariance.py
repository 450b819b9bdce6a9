"""Time of pvio_hip_ba_covariance (upload + undamped linearization + reduction + k_cov_assemble / k_cov_invert / k_cov_landmarks + read-back):
wall time of the call and hipEvent time of the three new kernels, means over the calls of one process after warm-up.
usage: python tests/prof_covariance.py [calls]"""
import os, sys, time
os.environ["PVIO_HIP_TIMING"] = "1"  # the library records the kernels' events only then (read once, at the first call)
sys.path.insert(0, '.'); sys.path.insert(0, 'tests')
import numpy as np
from pvio_amd import BAState
from pvio_amd.solver import HipContext
import ba_compare, marg_compare
from oracle import oracle_py as O
O.build()
calls = int(sys.argv[1]) if len(sys.argv) > 1 else 50
ctx = HipContext(device=0)
for nf, nl in ((8, 300), (10, 1000), (10, 50000)):
    pb = ba_compare.make(O, n_frames=nf, n_landmarks=nl, use_inertial=True)
    marg_compare.set_regular_prior(pb, pb.prior_frames)
    st = BAState(pb)
    for _ in range(5):
        res = ctx.covariance(pb, st, landmarks=True)
    assert res["positive_definite"] == 1
    ms = np.zeros(3)
    t0 = time.perf_counter()
    for _ in range(calls):
        ctx.covariance(pb, st, landmarks=True)
        ms += ctx.covariance_kernel_ms()
    t_c = (time.perf_counter() - t0) / calls
    ms /= calls
    print("%dx%d (P = %d, with lm_var), mean of %d calls: call %.3f ms   k_cov_assemble %.1f us  k_cov_invert %.1f us  k_cov_landmarks %.1f us"
          % (nf, nl, 15 * nf, calls, 1e3 * t_c, 1e3 * ms[0], 1e3 * ms[1], 1e3 * ms[2]), flush=True)
