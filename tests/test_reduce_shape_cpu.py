"""The arithmetic of rsx_sort_reduce* on the CPU: tests/cpp/reduce_shape_check drives radix_sorting_amd/csrc/rsx_reduce_shape.hpp.

What it pins: the bytes of a cell for every ops mask and value width; the copies of the cells a workgroup keeps against a
brute-force search (powers of two, at most 32, RSX_REDUCE_REPLICAS brought down to one that fits) and their layout against a byte
map (no part overlaps, every part aligned, all inside the budget); 2^12 cells fit whatever is wanted; the grid; and the seam rule
of the sort route: over random sorted arrays cut into tiles of 1, 2, 7 and 64, the runs written inside a tile and the runs
combined from tails and leads cover every run exactly once and add up to a plain loop's sums.
No GPU and no library: the program includes the header alone.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reduce_shape_check_program():
    exe = os.path.join(ROOT, "tests", "cpp", "reduce_shape_check")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", ROOT, "tests/cpp/reduce_shape_check"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "reduce_shape_check OK" in out.stdout, out.stdout + out.stderr
