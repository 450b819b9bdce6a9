"""pvio_amd/csrc/marg_prior.h -- the dense host algebra of a marginalization (assemble_information, eliminate_victim, sqrt_information) -- alone:
a stand-alone program built with the address and undefined-behaviour sanitizers (tests/hipemu/marg_prior_check.cpp), run as a child process."""
import os
import subprocess

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu")


def test_prior_algebra_is_exact_on_exact_inputs_and_keeps_its_square_root_invariants():
    subprocess.check_call(["make", "-s", "-C", EMU_DIR, "marg_prior_check"])
    r = subprocess.run([os.path.join(EMU_DIR, "marg_prior_check")], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "FAILED" not in r.stdout and r.stderr.count("ERROR") == 0
    lines = r.stdout.splitlines()
    assert len(lines) == 11 and all(l.endswith(": ok") for l in lines)
