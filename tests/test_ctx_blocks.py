"""CPU-side checks of the owner of a call's device blocks (diffsol_amd/csrc/dsh_ctx_blocks.hpp), through which the device-resident solve drivers take and return
every block of a solve."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "diffsol_amd", "csrc", "dsh_ctx_blocks.hpp")


def test_blocks_are_returned_once_on_every_way_out(tmp_path):
    """tests/ctx_blocks_check/ctx_blocks_check.cpp: a stand-alone program over dsh_ctx_blocks.hpp alone, with counting fakes of dsh_malloc / dsh_free over malloc and
    an opaque context, built with the address and undefined-behaviour sanitizers (a block never returned is a leak, one returned twice a double free).  Normal
    use, two contexts, failure of the 1st .. 4th allocation, an owner that goes on after a failure, a scope left early, zero blocks, a block beyond the capacity."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the block-owner check"
    exe = tmp_path / "ctx_blocks_check"
    src = os.path.join(ROOT, "tests", "ctx_blocks_check", "ctx_blocks_check.cpp")
    r = subprocess.run([gxx, "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-Wall", "-Wextra", "-Werror",
                        "-I" + os.path.join(ROOT, "diffsol_amd", "csrc"), src, "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "ALL OK" and len(lines) >= 20 and not [ln for ln in lines if "WRONG" in ln]


def test_block_owner_header_is_plain_cxx():
    """the owner must build without HIP: the C ABI header is its only include, no device qualifiers"""
    txt = open(HEADER).read()
    assert "hip/" not in txt and "__device__" not in txt and "__global__" not in txt and "__host__" not in txt
    assert re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", txt) == ["../../include/diffsol_hip.h"]
    # the header it includes is the C ABI: no HIP there either
    abi = open(os.path.join(ROOT, "include", "diffsol_hip.h")).read()
    assert "hip/" not in abi
