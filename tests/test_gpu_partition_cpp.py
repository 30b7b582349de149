"""radix_sort_partition (include/radix_sort.hpp) on the GPU: tests/cpp/partition_check runs the template with u32, float, int64_t
and uint8_t keys, ascending and descending, uint32_t and uint64_t indices, 1 / 3 / 200 / 700 edges (both routes), on host arrays
(rsx_sort_partition's host-pointer form), against std::upper_bound / std::lower_bound over the sorted edges and a
std::stable_sort of the positions by bin."""
import os
import subprocess

import pytest

import radix_sorting_amd as rsa

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    rsa.require_gpu()


def test_partition_check_program():
    exe = os.path.join(ROOT, "tests", "cpp", "partition_check")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", ROOT, "cpp"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "partition_check: ok" in out.stdout, out.stdout + out.stderr
