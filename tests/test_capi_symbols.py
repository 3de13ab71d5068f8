"""The C-ABI library builds for gfx950 and exports every symbol include/grid_capi.h declares (no compute calls here)."""
import json
import os
import re
import subprocess
import sys

import pytest

from gridcodegenerator_amd.runtime import INCLUDE_DIR, build_library


def declared_symbols():
    text = open(os.path.join(INCLUDE_DIR, "grid_capi.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(grid_[a-z_0-9]+)\s*\(", text)))


def test_header_declares_the_hot_path_entry_points():
    syms = declared_symbols()
    for s in ("grid_init", "grid_close", "grid_forward_dynamics_gradient_host", "grid_forward_dynamics_gradient_device",
              "grid_forward_dynamics_gradient_qdd_minv_device", "grid_last_error"):
        assert s in syms


@pytest.mark.parametrize("robot", ["iiwa14"])
def test_library_builds_and_exports_all_symbols(robot):
    so = build_library(robot)  # hipcc cross-compiles gfx950 without a GPU
    # (loaded in a child process: the HIP runtime it links would otherwise be loaded into the test process ahead of torch's own copy, torch
    # would then load a second one, and the GPU tests later in the same session would find no device)
    probe = ("import ctypes, json, sys\n"
             "lib = ctypes.CDLL(sys.argv[1])\n"
             "lib.grid_robot_name.restype = ctypes.c_char_p\n"
             "print(json.dumps({'missing': [s for s in sys.argv[2:] if not hasattr(lib, s)], 'robot': lib.grid_robot_name().decode(),\n"
             "                  'joints': lib.grid_num_joints(), 'lanes': lib.grid_lanes_per_solve(), 'lds': lib.grid_lds_bytes_per_block()}))\n")
    out = subprocess.run([sys.executable, "-c", probe, so] + declared_symbols(), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads(out.stdout.strip().splitlines()[-1])
    assert d["missing"] == [], d["missing"]
    assert d["robot"] == robot
    assert d["joints"] == 7
    assert d["lanes"] == 8
    assert d["lds"] <= 80 * 1024  # two SUGGESTED_THREADS blocks fit the 160 KB LDS of a CU


def test_missing_library_fails_loudly(tmp_path):
    from gridcodegenerator_amd.runtime import GridError, GridLibrary

    with pytest.raises(GridError):
        GridLibrary(str(tmp_path / "libgrid_nope.so"))
