"""The admission bounds of the device-resident Tsit45 kernel (kErkMaxLaneDoubles = 112, built-in models with n <= 4; csrc/dsh_erk_kernel.hpp) are claims about the
compiler: every admitted instantiation keeps its lane state in registers.  This CPU-tier test asks the compiler: csrc/dsh_erk_resident.hip compiled for the device
only with the Makefile's HIPFLAGS and -Rpass-analysis=kernel-resource-usage (hipcc cross-compiles gfx950 without a GPU, about 8 s), and the resource remarks of every
k_erk_resident instantiation read — no scratch memory, no vector register spilled.  It reads the remarks only, not the instruction listing."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "diffsol_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def makefile_hipflags():
    text = open(os.path.join(CSRC, "Makefile")).read()
    arch = re.search(r"^ARCH \?= (\S+)$", text, re.M).group(1)
    return re.search(r"^HIPFLAGS \?= (.*)$", text, re.M).group(1).replace("$(ARCH)", arch).split()


def resource_remarks(stderr):
    """{mangled kernel name: {remark field: integer}} of the compiler's kernel-resource-usage remarks"""
    kernels, cur = {}, None
    for line in stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+) \[-Rpass-analysis", line)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    return kernels


def test_every_tsit45_instantiation_stays_in_registers(tmp_path):
    r = subprocess.run([HIPCC] + makefile_hipflags() + ["-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-S", "dsh_erk_resident.hip", "-o", str(tmp_path / "erk.s")],
                       cwd=CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    erk = {k: v for k, v in resource_remarks(r.stderr).items() if "k_erk_resident" in k}
    kinds = {"plain": 0, "SENS": 0, "INTOUT": 0}
    for name, res in erk.items():
        assert res["ScratchSize"] == 0 and res["VGPRs Spill"] == 0, (name, res)
        ba, wave, sens, intout = re.search(r"((?:Lb[01]E){4})E", name).group(1)[2::4]  # the four trailing template flags <.., BA, WAVE, SENS, INTOUT>
        kinds["SENS" if sens == "1" else "INTOUT" if intout == "1" else "plain"] += 1
    # exponential decay with and without its root function and robertson_ode, BA x WAVE each: plain and INTOUT; exponential decay alone is admitted with SENS
    assert kinds == {"plain": 12, "SENS": 4, "INTOUT": 12}, kinds
