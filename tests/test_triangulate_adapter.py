"""The adapter's plane-track re-validation with PVIO_HIP_DEVICE_TRIANGULATION=1 (pvio_amd/host/bundle_adjustor.cpp): the tracks are triangulated
by one pvio_hip_triangulate call in place of one host SVD each.  The switch is read once per process, so every case runs in a fresh child: the
post-pass window of tests/test_host_adapter.py against oracle.post_passes, the same `moved` pattern, and the child's own report (PVIO_HIP_TIMING)
that a non-zero number of tracks went to the device.  Emulator (libpvio_host_emu.so) and, under -m gpu, the product library."""
import os
import re
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

CHILD = (
    "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
    "import host_compare\n"
    "from oracle import oracle_py as O\n"
    "from test_host_adapter import POST\n"
    "O.build(); O.lib()\n"
    "lib = host_compare.load(%%r)\n"
    "moved, orphaned = host_compare.check_adapter_post_passes(lib, O, **POST)\n"
    "assert moved[:5].all() and moved[40:45].all() and not moved[5:40].any()\n"
    "print('post passes agree; moved', int(moved.sum()))\n") % (ROOT, HERE)


def run_child(target, device_triangulation):
    env = dict(os.environ, PVIO_HIP_TIMING="1")
    env.pop("PVIO_HIP_DEVICE_TRIANGULATION", None)
    if device_triangulation:
        env["PVIO_HIP_DEVICE_TRIANGULATION"] = "1"
    r = subprocess.run([sys.executable, "-c", CHILD % target], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "post passes agree" in r.stdout
    m = re.findall(r"plane re-validation: ([0-9.]+) us, (\d+) tracks triangulated on the device, (\d+) tracks moved \(PVIO_HIP_DEVICE_TRIANGULATION (on|off)\)", r.stderr)
    assert len(m) == 1, r.stderr[-2000:]
    us, on_device, moved, switch = float(m[0][0]), int(m[0][1]), int(m[0][2]), m[0][3]
    print("%s: re-validation %.1f us, %d tracks on the device, %d moved, switch %s" % (target, us, on_device, moved, switch))
    return on_device, moved, switch


def check_switch(target):
    on_device, moved_on, switch = run_child(target, True)
    assert switch == "on" and on_device > 0
    off_device, moved_off, switch = run_child(target, False)  # default: nothing goes to the device, the same tracks move
    assert switch == "off" and off_device == 0 and moved_off == moved_on


def test_adapter_post_passes_with_device_triangulation_emulated():
    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "hipemu"), "libpvio_hipemu.so"])
    check_switch("libpvio_host_emu.so")


@pytest.mark.gpu
def test_adapter_post_passes_with_device_triangulation_gpu():
    check_switch("libpvio_host.so")
