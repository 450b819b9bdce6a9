"""pvio_amd/csrc/hip_buffer.h -- the owner of the grow-only scratch buffers of Klt and BASolver -- alone: a stand-alone program above the
emulator's allocator, built with the address and undefined-behaviour sanitizers (tests/hipemu/hip_buffer_check.cpp), run as a child process."""
import os
import subprocess

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu")


def test_scratch_buffer_keeps_grows_frees_once_and_survives_a_failed_allocation():
    subprocess.check_call(["make", "-s", "-C", EMU_DIR, "hip_buffer_check"])
    r = subprocess.run([os.path.join(EMU_DIR, "hip_buffer_check")], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "FAILED" not in r.stdout and r.stderr.count("ERROR") == 0
    assert r.stdout.splitlines()[:2] == ["device: ok", "pinned: ok"]
