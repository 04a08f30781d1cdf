"""The kernel source's parts (CPU): csrc/merging_hip.hip holds the C entry points and includes one
part per subsystem (DESIGN.md's source map). Every file under csrc/ is part of the build, no kernel
is left in the translation unit itself, and every part names what it uses: it compiles on its own."""
import glob
import os
import subprocess

import pytest

from conftest import ROOT
from merging_gym import build
from native_build import hipcc

CSRC = os.path.join(ROOT, "merging-gym_amd", "csrc")
PARTS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*.h")))


def test_no_orphan_parts():
    files = build.source_files()
    assert files[0] == build.SRC == os.path.join(CSRC, "merging_hip.hip")
    assert sorted(files) == sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC))
    assert len(PARTS) == len(files) - 1 >= 14


def test_translation_unit_holds_no_kernel():
    with open(build.SRC) as f:
        assert "__global__" not in f.read()


@pytest.mark.skipif(hipcc() is None, reason="hipcc not found")
@pytest.mark.parametrize("part", PARTS)
def test_part_compiles_alone(part):
    r = subprocess.run([hipcc(), "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off",
                        "-I", os.path.join(ROOT, "include"), "-x", "hip", "-fsyntax-only", os.path.join(CSRC, part)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
