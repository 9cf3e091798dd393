"""ASan + UBSan runs of the CPU-side code (the reference has no race/sanitizer tooling; GPU
sanitizers are not available on the pool, so these cover the oracle and the host half of the library)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_oracle_under_asan_ubsan():
    out = subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "-s", "asan-test"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 mismatches" in out.stdout and "ERROR" not in out.stderr


def test_host_library_under_asan_ubsan():
    # where a GPU is visible the selftest's shoots run on it, and ROCm's runtime keeps a few allocations until exit.  tests/lsan_rocm.supp
    # makes LeakSanitizer skip every leaked block with a frame of ROCm's runtime libraries in its allocation stack: those blocks, but also
    # a runtime object the library would create and never release (a stream, an event, ...).  Leaks of memory the project allocates
    # itself (new, malloc, containers) are still errors; a leaked runtime object is not caught here on a machine with a GPU
    env = dict(os.environ, LSAN_OPTIONS="suppressions=" + os.path.join(ROOT, "tests", "lsan_rocm.supp"))
    out = subprocess.run(["make", "-C", os.path.join(ROOT, "hare_amd", "csrc"), "-s", "asan-test"], capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 failures" in out.stdout and "ERROR" not in out.stderr


def test_host_threading_under_tsan():
    # the fan-out, the ray split and the context lease of the host-buffer calls (tests/stubs/fan_out_tsan.cpp), against the recording HIP
    # stand-in: a program of its own, no GPU
    out = subprocess.run(["make", "-C", os.path.join(ROOT, "hare_amd", "csrc"), "-s", "tsan-test"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "fan_out_tsan: 0 failures" in out.stdout and "ThreadSanitizer" not in out.stderr
