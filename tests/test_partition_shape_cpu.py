"""The arithmetic of rsx_sort_partition*'s scatter route on the CPU: tests/cpp/partition_shape_check drives
radix_sorting_amd/csrc/rsx_partition_shape.hpp.

What it pins: the shares cover [0, n) exactly once and in order for n around every seam (a tile, the smallest share, the largest
grid, 2^32) and every head of 0 .. 15 keys, with the head in the first share and the tail in the last and every other boundary
a whole number of tiles behind the head; the bin-major scan gives the starts and totals of one serial loop in output order; the
read-out of the caller's offsets agrees with a brute-force count where edges repeat (empty parts); the seam between the ranking
forms and the bits of a bin number.  No GPU and no library: the program includes the header alone.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_partition_shape_check_program():
    exe = os.path.join(ROOT, "tests", "cpp", "partition_shape_check")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", ROOT, "tests/cpp/partition_shape_check"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "partition_shape_check OK" in out.stdout, out.stdout + out.stderr
