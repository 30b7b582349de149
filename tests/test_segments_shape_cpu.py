"""The arithmetic of rsx_sort_segments*'s LDS route on the CPU: tests/cpp/segments_shape_check drives
radix_sorting_amd/csrc/rsx_segments_shape.hpp.

What it pins: every class's LDS bytes are at most 163,840 (a CU's) for every key width, with and without indices, whatever the
longest segment of the launch; cap is monotone in the key width and no step more would fit; every length 0 .. cap + 1 lands in
exactly one class and fits its team's buffers; a class's grid covers its list with no workgroup to spare; the plan kernels'
shares cover the segments.  No GPU and no library: the program includes the header alone.  The same program is built a second
time with the address and undefined-behaviour sanitizers (host code with its own main) and must come out the same.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_segments_shape_check_program():
    exe = os.path.join(ROOT, "tests", "cpp", "segments_shape_check")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", ROOT, "tests/cpp/segments_shape_check"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "segments_shape_check OK" in out.stdout, out.stdout + out.stderr


def test_segments_shape_check_under_sanitizers(tmp_path):
    exe = str(tmp_path / "segments_shape_check_san")
    src = os.path.join(ROOT, "tests", "cpp", "segments_shape_check.cpp")
    subprocess.run(["g++", "-std=gnu++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe],
                   check=True, timeout=300)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "segments_shape_check OK" in out.stdout, out.stdout + out.stderr
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
