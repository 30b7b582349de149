"""WsLayout on the CPU: tests/cpp/ws_layout_check drives radix_sorting_amd/csrc/rsx_ws_layout.hpp.

What it pins: a caller-owned workspace keeps the parts, offsets and totals that rsx_workspace_bytes, borrow_ctx, borrow_blind,
rsx_workspace_bytes_fast and rsx_async_route_ws gave when each wrote the arithmetic out itself -- all four key widths, n at 2,
either side of 2^22 and of 2^30 (the window of the attempt without a histogram; 64-bit status words), the plan at + 64, the
attempt's control block behind gscan, and a workspace one byte short of the fast total, which does not borrow the attempt's part.
No GPU and no library: the program includes the header alone.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ws_layout_check_program():
    exe = os.path.join(ROOT, "tests", "cpp", "ws_layout_check")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", ROOT, "tests/cpp/ws_layout_check"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "ws_layout_check OK" in out.stdout, out.stdout + out.stderr
