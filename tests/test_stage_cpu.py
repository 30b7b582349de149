"""stage_layout on the CPU: tests/cpp/stage_check drives radix_sorting_amd/csrc/rsx_stage.hpp.

What it pins: where the arrays of a blocking call on host buffers lie in the context's one staging buffer -- for every combination
of up to five arrays, each absent or of 0, 1, 255, 256 or 257 bytes (either side of a multiple of 256): every slot starts on a
256-byte boundary, no two slots overlap, an absent array takes no room and has no offset, and the total is the end of the last
slot.  No GPU and no library: the program includes the header alone.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stage_check_program():
    exe = os.path.join(ROOT, "tests", "cpp", "stage_check")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", ROOT, "tests/cpp/stage_check"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "stage_check OK" in out.stdout, out.stdout + out.stderr
