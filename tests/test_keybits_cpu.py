"""The arithmetic over the varying bits on the CPU: tests/cpp/keybits_check drives radix_sorting_amd/csrc/rsx_keybits.hpp.

What it pins: the bitmap of rsx_sort_unique* and rsx_sort_group* keeps the words, chunks and bytes (table_bytes), the variant of
the mark kernel and the grids that each driver worked out for itself before the header; the sweeps over the keys keep their grid at
both ends of the clamp; bit_runs gives the runs of a mask lowest first, takes eight of them and refuses nine; one kept column is
one run of eight bits.  No GPU and no library: the program includes the header alone.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_keybits_check_program():
    exe = os.path.join(ROOT, "tests", "cpp", "keybits_check")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", ROOT, "tests/cpp/keybits_check"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "keybits_check OK" in out.stdout, out.stdout + out.stderr
