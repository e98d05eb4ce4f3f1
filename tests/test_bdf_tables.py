"""The Bdf::_new tables (alpha, gamma, squared error constants; diffsol_amd/csrc/dsh_bdf_tables.hpp) that the per-order step bodies of the lock-step fast BDF kernel
carry as compile-time constants against the tables the host set-up fills at run time, as 64-bit patterns.  Both come from one function, bdf_new_tables(): the set-up
(dsh_adaptive.hip) runs it as compiled code, the kernel reads kBdfTables, its constant-evaluated result.  A small host program (tests/bdf_tables_check) built
without optimisation and with -ffp-contract=off, the set-up's flag, prints both; a third evaluation of the same operations in numpy's IEEE doubles stands beside
them.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "bdf_tables_check", "bdf_tables_check.cpp")
_CSRC = os.path.join(os.path.dirname(_HERE), "diffsol_amd", "csrc")


def numpy_tables():
    """bdf.rs:286-306 in the order of the set-up's loop, every operation one rounded float64 operation."""
    f = np.float64
    kappa = [f(0.0), f(-0.1850), f(-1.0) / f(9.0), f(-0.0823), f(-0.0415), f(0.0)]
    alpha, gamma, ec2 = [f(0.0)], [f(0.0)], [f(1.0)]
    for i in range(1, 6):
        i_t = f(i)
        one_over_i, one_over_i_plus_one = f(1.0) / i_t, f(1.0) / (i_t + f(1.0))
        gamma.append(gamma[i - 1] + one_over_i)
        alpha.append(f(1.0) / ((f(1.0) - kappa[i]) * gamma[i]))
        e = kappa[i] * gamma[i] + one_over_i_plus_one
        ec2.append(e * e)
    return {"alpha": alpha, "gamma": gamma, "ec2": ec2}


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("bdf_tables") / "bdf_tables_check")
    subprocess.run([cxx, "-std=c++17", "-O0", "-ffp-contract=off", "-I", _CSRC, "-o", exe, _SRC], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    tabs = {"run": {}, "const": {}}
    for line in out.split("\n"):
        if line:
            tag, name, i, bits = line.split()
            tabs[tag].setdefault(name, [None] * 6)[int(i)] = int(bits, 16)
    return tabs


@pytest.mark.parametrize("name", ["alpha", "gamma", "ec2"])
def test_compile_time_tables_have_the_bits_of_the_tables_the_set_up_fills(printed, name):
    run, const = printed["run"][name], printed["const"][name]
    assert None not in run and None not in const
    ref = [int(np.float64(v).view(np.uint64)) for v in numpy_tables()[name]]
    for i in range(6):
        print(f"{name}[{i}]: run {run[i]:016x} const {const[i]:016x} numpy {ref[i]:016x}")
    assert run == const, f"{name}: the constant-evaluated table differs from the table computed at run time"
    assert run == ref, f"{name}: the host program's table differs from the same operations in numpy"


def test_the_tables_are_the_known_values(printed):
    """gamma_k = sum 1/j and alpha_1 = 1 / (1.185 gamma_1): a table of the right shape, not only two equal ones."""
    g = np.array(printed["const"]["gamma"], dtype=np.uint64).view(np.float64)
    a = np.array(printed["const"]["alpha"], dtype=np.uint64).view(np.float64)
    assert g[0] == 0.0 and g[1] == 1.0 and g[2] == 1.5 and abs(g[5] - 137.0 / 60.0) < 1e-15
    assert a[0] == 0.0 and abs(a[1] - 1.0 / 1.185) < 1e-15 and abs(a[5] - 60.0 / 137.0) < 1e-15
