"""The front end's scratch buffers across sizes in ONE context: small -> large -> small.  Every buffer of pvklt::Klt is grow-only (csrc/hip_buffer.h) and
its layout depends on the size of the call (csrc/klt.hip: DetectScratch, FundBlock, TrackBlock, the distorted-source buffer), so a call has to be right
in a buffer that an earlier, larger call left behind, and after a growth.  The other tests open a context per case or only shrink their sizes.  The
checks are the existing ones: bit-exact against the oracle (and, for the RANSAC, against the sequential host form)."""
import os
import subprocess

import numpy as np
import pytest

import gftt_compare
import host_compare
import klt_compare
import test_host_ingest as ingest
import test_host_ransac as ransac

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu")

DETECT_SIZES = [(64, 48), (176, 132), (64, 48)]
RANSAC_CASES = [(9, 0.0, 0.05, 6), (300, 0.2, 0.3, 2), (9, 0.0, 0.05, 6)]  # mask words per model: 1, 5, 1
SOURCE_SIZES = [(80, 60), (200, 150), (80, 60)]  # distorted images behind one 64 x 48 undistortion map
TRACK_COUNTS = [6, 60, 6]


def _small_large_small(ctx, host, oracle):
    rng = np.random.default_rng(21)
    xy, fr = ingest._random_maps(rng, 64, 48, *SOURCE_SIZES[0])
    for (w, h), case, (sw, sh), n in zip(DETECT_SIZES, RANSAC_CASES, SOURCE_SIZES, TRACK_COUNTS):
        print((w, h), gftt_compare.check_detect(ctx, oracle, w, h))
        print(case, ransac._check_device(ctx, host, *case))
        ingest._check_remap(ctx, oracle, rng, 64, 48, sw, sh, xy, fr)
        print(n, klt_compare.check_klt(ctx, oracle, 176, 132, n))


def _host_harness(name):
    lib = host_compare.load(name)
    lib.host_ransac.restype = ransac.C.c_int
    return lib


def test_emulated_scratch_reuse_small_large_small(oracle):
    from pvio_amd import capi
    from pvio_amd.solver import HipContext
    subprocess.check_call(["make", "-s", "-C", EMU_DIR, "libpvio_hipemu.so"])
    ctx = HipContext(lib=capi.load(os.path.join(EMU_DIR, "libpvio_hipemu.so")))
    try:
        _small_large_small(ctx, _host_harness("libpvio_host_emu.so"), oracle)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_gpu_scratch_reuse_small_large_small(oracle):
    """the same on the product library (its harness is the one linked against it: the emulated build and the product both define the kernels' symbols)"""
    from pvio_amd.solver import HipContext
    ctx = HipContext(device=0)
    try:
        _small_large_small(ctx, _host_harness("libpvio_host.so"), oracle)
    finally:
        ctx.close()
