"""radix_sort_segments (include/radix_sort.hpp) on the GPU: tests/cpp/segments_check runs the template with u32, float, int64_t and
uint8_t keys, ascending and descending, uint32_t and uint64_t offsets and indices, global and local, on host arrays
(rsx_sort_segments's host-pointer form) whose segments fall in every size class, against a std::stable_sort of every segment's
positions -- on the route the library takes by itself, on the LDS / MIXED route and on the composed route."""
import os
import subprocess

import pytest

import radix_sorting_amd as rsa

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    rsa.require_gpu()


@pytest.mark.parametrize("force", [None, "1", "2"])
def test_segments_check_program(force):
    exe = os.path.join(ROOT, "tests", "cpp", "segments_check")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", ROOT, "cpp"], check=True)
    env = {k: v for k, v in os.environ.items() if k not in ("RSX_SEGMENTS_FORCE", "RSX_SEGMENTS_MAX_LONG")}
    if force:
        env.update(RSX_SEGMENTS_FORCE=force, RSX_SEGMENTS_MAX_LONG="8")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0 and "segments_check: ok" in out.stdout, out.stdout + out.stderr
