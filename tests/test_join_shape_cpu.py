"""The arithmetic of rsx_sort_join* / rsx_join_pairs* on the CPU: tests/cpp/join_shape_check drives radix_sorting_amd/csrc/rsx_join_shape.hpp.

What it pins: the route rule at its edges (16 / 17 varying bits, 8 / 9 runs of them, m = 2^32 - 1 / 2^32; a forced route before
the table, the table before the search-or-merge rule), the table's size and the grids; and the expansion: a plain C++ model built
from the header's own functions (the row-tile sums and their scan, the segment of an output tile inside a row tile, the row of a
pair position) over random count arrays -- runs of zeros spanning whole row tiles, rows larger than several output tiles, totals
of k tiles and one more or less, inner and left -- with tiles of 1, 2, 7 and 64 rows and pairs: every pair position is produced
exactly once and is what a naive loop over the rows gives.  Totals above 2^32 are checked by arithmetic, with the library's tiles.
No GPU and no library: the program includes the header alone.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_join_shape_check_program():
    exe = os.path.join(ROOT, "tests", "cpp", "join_shape_check")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", ROOT, "tests/cpp/join_shape_check"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "join_shape_check OK" in out.stdout, out.stdout + out.stderr
