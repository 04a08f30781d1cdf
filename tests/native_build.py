"""Build helpers the native tests share: the compilers, and the library's translation unit compiled once per
process under AddressSanitizer and UndefinedBehaviorSanitizer, for the stand-alone drivers of tests/native/ to
link against. Nothing here runs on a GPU and nothing is loaded into Python."""

import functools
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
SANITIZE_FLAGS = ["--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-omit-frame-pointer",
                  "-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fsanitize=undefined",
                  "-I", os.path.join(ROOT, "include")]
SANITIZE_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1",
                    UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


def hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    return None


def cc():
    return os.environ.get("CC") or shutil.which("gcc") or shutil.which("cc") or shutil.which("clang")


@functools.lru_cache(maxsize=1)
def sanitized_library_object():
    """csrc/merging_hip.hip compiled with SANITIZE_FLAGS into an object file in a fresh temporary directory
    (kept for the process): the half minute every sanitizer test would otherwise spend on the same source."""
    obj = os.path.join(tempfile.mkdtemp(prefix="merging_hip_sanitize."), "merging_hip.o")
    b = subprocess.run([hipcc(), *SANITIZE_FLAGS, "-c", "-o", obj,
                        os.path.join(ROOT, "merging-gym_amd", "csrc", "merging_hip.hip")],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    return obj


def run_sanitized_driver(driver, tmp_path):
    """Link tests/native/<driver>.cpp (its own main) against the sanitized library object with the same flags
    and run the program: the finished process, for the test to assert on."""
    exe = str(tmp_path / driver)
    b = subprocess.run([hipcc(), *SANITIZE_FLAGS, "-o", exe, sanitized_library_object(),
                        os.path.join(NATIVE, driver + ".cpp")], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    return subprocess.run([exe], env=SANITIZE_ENV, capture_output=True, text=True, timeout=300)
