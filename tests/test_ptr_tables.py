"""pvio_amd/host/ptr_tables.h -- the pointer-keyed tables of the host adapter and the protocol of its observation cache (unchanged / grown by
the newest observation / rebuilt, replay against the window's frame ids, the wholesale drop) -- alone: a stand-alone program built with the
address and undefined-behaviour sanitizers (tests/host/ptr_tables_check.cpp), run as a child process."""
import os
import subprocess

HOST_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host")


def test_fixed_table_refuses_ptr_set_grows_and_the_observation_cache_replays_what_a_walk_gives():
    subprocess.check_call(["make", "-s", "-C", HOST_DIR, "ptr_tables_check"])
    r = subprocess.run([os.path.join(HOST_DIR, "ptr_tables_check")], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "FAILED" not in r.stdout and r.stderr.count("ERROR") == 0
    assert r.stdout.splitlines() == ["fixed table: ok", "PtrSet: ok", "ObsCache outcomes: ok", "ObsCache replay: ok", "ObsCache rehash: ok",
                                     "ObsCache begin_window: ok"]
