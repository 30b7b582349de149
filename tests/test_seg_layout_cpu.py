"""SegLayout and SlotParts on the CPU: tests/cpp/seg_layout_check drives radix_sorting_amd/csrc/rsx_seg_layout.hpp.

What it pins: the control block of the segmented routes (c.seg) keeps the regions, sizes and total that seg_bytes / seg_layout
gave when each route wrote the arithmetic out itself -- rsx_workspace_bytes_fast hands those totals to callers -- and the
placement of level-1 slots in two arrays (the caller's spare buffer and scratch) puts every slot inside its array within 32-bit
reach of one base, both ways round, at lo = 0 and 255, and exactly up to a span of 2^32 - 1 elements.  No GPU and no library:
the program includes the header alone.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_seg_layout_check_program():
    exe = os.path.join(ROOT, "tests", "cpp", "seg_layout_check")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", ROOT, "tests/cpp/seg_layout_check"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "seg_layout_check OK" in out.stdout, out.stdout + out.stderr
