"""The C-ABI and header side of the POA alignment modes, without a GPU: the ctypes mirror of hx_poa_mode_params has the C size, a caller
compiled against include/spoa_hx.hpp constructs kSW and kOV engines (they used to throw), and without a device its consensus fails loudly."""
import ctypes as C
import os
import subprocess

import pytest

from haslr_amd import ctypes_defs as T
from haslr_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def modes_caller(built, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("spoa_modes") / "spoa_modes_caller")
    lib = os.path.join(ROOT, "haslr_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "spoa_modes_caller.cpp"), "-o", exe,
                           "-L", lib, "-lhaslr_hip", "-pthread", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_mode_params_size_and_values_match_c(built, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "haslr_types.h"\nint main(){printf("%zu %d %d %d\\n",sizeof(hx_poa_mode_params),HX_POA_SW,HX_POA_NW,HX_POA_OV);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [C.sizeof(T.PoaModeParams), T.POA_TYPES["sw"], T.POA_TYPES["nw"], T.POA_TYPES["ov"]]


def test_entry_point_is_exported(built):
    assert hasattr(hip.lib(), "hx_poa_sequences_mode")
    assert "poa_general" in hip.option_names() and "poa_modes_slot_kb" in hip.option_names()


def test_sw_and_ov_engines_can_be_constructed(modes_caller):
    r = subprocess.run([modes_caller, "--construct"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "ok\n", (r.returncode, r.stderr)


def test_consensus_without_a_device_fails_loudly(modes_caller):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a HIP device is present: covered by tests/test_poa_modes_gpu.py")
    for t in ("sw", "ov"):
        r = subprocess.run([modes_caller], input=f"{t}\nACGTACGT\nACGTTCGT\n", capture_output=True, text=True)
        assert r.returncode == 1 and "no HIP device" in r.stderr and r.stdout == "", (t, r.returncode, r.stderr)
