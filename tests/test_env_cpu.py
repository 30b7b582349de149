"""The RSX_* switches on the CPU: tests/cpp/env_check drives Env::load() (radix_sorting_amd/csrc/rsx_env.hpp) with setenv / unsetenv.

What it pins: one switch of every parse kind gives the documented value, and a variable that has been taken away again gives
the member's default ON THE SAME OBJECT -- rsx_reload_env() between two tests (the _fresh_routes fixtures) relies on that; before
the loader started from the defaults, RSX_PASS32_MIN_MI, RSX_PASS32_PREFETCH and RSX_FORCE_LEAFC kept a test's value for the rest
of the process.  No GPU and no library: the program includes the header alone.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_env_check_program():
    exe = os.path.join(ROOT, "tests", "cpp", "env_check")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", ROOT, "tests/cpp/env_check"], check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("RSX_")}
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    assert out.returncode == 0 and "env_check OK" in out.stdout, out.stdout + out.stderr
