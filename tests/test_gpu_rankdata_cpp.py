"""radix_sort_rankdata (include/radix_sort.hpp) on the GPU: tests/cpp/rankdata_check runs the template with u32, float and int64_t
keys, 4- and 8-byte indices and rsx_kdf::descending against answers derived from std::stable_sort, and with a KeyFunc that must
be refused."""
import os
import subprocess

import pytest

import radix_sorting_amd as rsa

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    rsa.require_gpu()


def test_rankdata_check_program():
    exe = os.path.join(ROOT, "tests", "cpp", "rankdata_check")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", ROOT, "cpp"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "rankdata_check: ok" in out.stdout, out.stdout + out.stderr
