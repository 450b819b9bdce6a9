"""Seconds per flattening of a Map by the host adapter (pvio_amd/host/bundle_adjustor.cpp, host_flatten_seconds of tests/host/roundtrip.cpp) on
the two windows of tests/prof_keyframe.py: every track walked from scratch (reps > 0) and replayed from the observation cache (reps < 0).
No GPU: python tests/prof_flatten.py [path of a libpvio_host_emu.so; default: tests/host/libpvio_host_emu.so, built if need be]"""
import ctypes as C
import sys
sys.path.insert(0, '.'); sys.path.insert(0, 'tests')
import host_compare, marg_compare
from oracle import oracle_py as O
O.build()
lib = C.CDLL(sys.argv[1]) if len(sys.argv) > 1 else host_compare.load("libpvio_host_emu.so")
lib.host_flatten_seconds.restype = C.c_double
for nf, nl in ((10, 1000), (8, 300)):
    pb, st = marg_compare.solved_window(O, regular_prior=False, n_frames=nf, n_landmarks=nl, use_inertial=True)
    pbc, stc = pb.as_c(), st.as_c()
    us = [1e6 * lib.host_flatten_seconds(C.byref(pbc), C.byref(stc), C.c_int32(1), C.c_int32(reps)) for reps in (200, -200, 200, -200)]
    print("%d x %d: flatten from scratch %.1f us, from the cache %.1f us; again %.1f us, %.1f us" % (nf, nl, us[0], us[1], us[2], us[3]))
