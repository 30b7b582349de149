"""The arithmetic of rsx_sort_locate*'s search route on the CPU: tests/cpp/locate_shape_check drives
radix_sorting_amd/csrc/rsx_locate_shape.hpp.

What it pins: the start table and the per-key search agree with std::upper_bound for every key within one of any edge, 0 and
all-ones -- for 1, 2, 255, 256, 257 and 4096 edges, edges inside one digit of the start table (the longest search: 12 halvings),
in exactly two digits, sharing prefixes of 0 to 63 bits, at 0 and at all-ones; the edges and cum of duplicate-heavy values agree
with a brute-force count; the finish gives brute-force less / equal; the LDS layout fits and the grid covers every tile once.
No GPU and no library: the program includes the header alone.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_locate_shape_check_program():
    exe = os.path.join(ROOT, "tests", "cpp", "locate_shape_check")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", ROOT, "tests/cpp/locate_shape_check"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "locate_shape_check OK" in out.stdout, out.stdout + out.stderr
