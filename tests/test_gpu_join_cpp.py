"""radix_sort_join and radix_sort_join_pairs (include/radix_sort.hpp) on the GPU: tests/cpp/join_check runs the templates with u32
(many to many, and dense ids), float, int64_t and uint8_t keys, ascending and descending, inner and left, uint32_t and uint64_t
indices, on host arrays (the host-pointer forms of rsx_sort_join and rsx_join_pairs), against std::stable_sort of the right row
numbers and std::equal_range by the key derivation."""
import os
import subprocess

import pytest

import radix_sorting_amd as rsa

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    rsa.require_gpu()


def test_join_check_program():
    exe = os.path.join(ROOT, "tests", "cpp", "join_check")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", ROOT, "cpp"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "join_check: ok" in out.stdout, out.stdout + out.stderr
