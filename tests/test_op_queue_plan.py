"""CPU-side checks of the op queue (dsh_ctx_set_op_queue): the hazard planner decides flush / no flush exactly as specified, and the new entry points are
declared in the headers and exported by both libraries."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DEVICE_SYMBOLS = ("dsh_ctx_set_op_queue", "dsh_ctx_get_op_queue", "dsh_ctx_flush", "dsh_ctx_op_queue_stats")
HOST_SYMBOLS = ("dshs_set_op_queue", "dshs_get_op_queue_stats")


def test_hazard_planner_decisions(tmp_path):
    """tests/opq_plan_check/opq_plan_check.cpp: a stand-alone program over diffsol_amd/csrc/dsh_opq_plan.hpp alone (no HIP include), built with the address and
    undefined-behaviour sanitizers.  Identical in-place ranges, a read of a just-written range and the adjacent-column ladder of an n x 8 matrix stay one
    chain; ranges shifted by one element or by one column minus one element, a write over a range read earlier, a broadcast operand over a written range,
    another total, another nb with the same total and the K+1-th op flush; zero-length ops never overlap."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the planner check"
    exe = tmp_path / "opq_plan_check"
    src = os.path.join(ROOT, "tests", "opq_plan_check", "opq_plan_check.cpp")
    r = subprocess.run([gxx, "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-Wall", "-Wextra", "-Werror",
                        "-I" + os.path.join(ROOT, "diffsol_amd", "csrc"), src, "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "ALL OK" and len(lines) >= 30 and not [ln for ln in lines if "WRONG" in ln]


def test_planner_header_is_plain_cxx():
    """the planner must build without HIP: no HIP include, no device qualifiers"""
    txt = open(os.path.join(ROOT, "diffsol_amd", "csrc", "dsh_opq_plan.hpp")).read()
    assert "hip/" not in txt and "__device__" not in txt and "__global__" not in txt
    assert re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", txt) == ["cstdint"]


def _declared(header, prefix):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(rf"\b({prefix}[a-z0-9_]+)\s*\(", src))


def test_op_queue_symbols_are_declared_and_exported():
    import __graft_entry__
    __graft_entry__.build()
    from diffsol_amd import _ffi
    dev_decl, host_decl = _declared("diffsol_hip.h", "dsh_"), _declared("diffsol_hip_solver.h", "dshs_")
    dev = ctypes.CDLL(_ffi.lib_paths()[0])
    _ffi.load_device_lib()
    host = ctypes.CDLL(_ffi.lib_paths()[1])
    for n in DEVICE_SYMBOLS:
        assert n in dev_decl, f"{n} is not declared in include/diffsol_hip.h"
        assert hasattr(dev, n), f"{n} is not exported by the device library"
        assert n in _ffi.DEVICE_ABI
    for n in HOST_SYMBOLS:
        assert n in host_decl, f"{n} is not declared in include/diffsol_hip_solver.h"
        assert hasattr(host, n), f"{n} is not exported by the host library"
        assert n in _ffi.HOST_ABI
    # no GPU is needed to ask a null context for its mode
    dev.dsh_ctx_get_op_queue.argtypes = [ctypes.c_void_p]
    assert dev.dsh_ctx_get_op_queue(None) == -1
    # the Rust shim binds them too
    ffi_rs = open(os.path.join(ROOT, "rust", "diffsol-hip", "src", "ffi.rs")).read()
    ctx_rs = open(os.path.join(ROOT, "rust", "diffsol-hip", "src", "context.rs")).read()
    for n in DEVICE_SYMBOLS:
        assert f"pub fn {n}(" in ffi_rs
    assert "pub fn set_op_queue(" in ctx_rs and "pub fn flush(" in ctx_rs
