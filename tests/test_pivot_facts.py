"""CPU tier of the reload-free step loop of the lock-step fast BDF kernel with the default options (csrc/dsh_adaptive_kernel.hpp DSH_STEP_NO_RELOAD;
profiles/pivot_facts.md) and of the pivot conditions its GPU cases are built on.

  * The flagship instantiation k_bdf_adaptive<RobertsonOde1, BA, WAVE, false, false, FAST, DEFOPT>, compiled alone for gfx950 with the Makefile's flags of
    dsh_adaptive_fast.hip (tests/pivot_facts_check/flagship.hip; hipcc cross-compiles without a GPU, a few seconds): 256 VGPRs or fewer, no more scratch than the 80 B
    it had, two wavefronts per SIMD, and as many scratch reload instructions in its listing as profiles/pivot_facts.md records.
  * The pivot conditions of the GPU cases (tests/test_gpu_pivot_facts.py), established with the oracle's lock-step group and first-max partial pivoting of M - c J in
    numpy along its accepted steps (tests/pivot_facts_cases.py)."""
import os
import re
import subprocess

import numpy as np

import pivot_facts_cases as PC
from test_erk_kernel_resources import CSRC, HIPCC, ROOT, makefile_hipflags, resource_remarks

FLAGSHIP = "_ZN3dsh14k_bdf_adaptiveINS_13RobertsonOde1ELb1ELb1ELb0ELb0ELb1ELb1EEE"


def makefile_fastflags():
    text = open(os.path.join(CSRC, "Makefile")).read()
    m = re.search(r"^FASTFLAGS := \$\(filter-out (.*?),\$\(HIPFLAGS\)\) (.*)$", text, re.M)
    drop = m.group(1).split()
    return [f for f in makefile_hipflags() if f not in drop] + m.group(2).split()


def recorded_reloads():
    text = open(os.path.join(ROOT, "profiles", "pivot_facts.md")).read()
    return int(re.search(r"scratch reload instructions in the flagship kernel: (\d+)", text).group(1))


def test_the_flagship_kernel_keeps_its_registers_its_occupancy_and_the_recorded_scratch_reloads(tmp_path):
    asm = tmp_path / "flagship.s"
    r = subprocess.run([HIPCC] + makefile_fastflags() + ["-I", CSRC, "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-S",
                                                         os.path.join(ROOT, "tests", "pivot_facts_check", "flagship.hip"), "-o", str(asm)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    res = [v for k, v in resource_remarks(r.stderr).items() if k.startswith(FLAGSHIP)]
    assert len(res) == 1, list(resource_remarks(r.stderr))
    res = res[0]
    reloads = sum(1 for line in open(asm) if re.match(r"\s+scratch_load_", line))
    print(f"flagship kernel: {res}; scratch reload instructions {reloads}")
    assert res["VGPRs"] <= 256
    assert res["ScratchSize"] <= 80
    assert res["Occupancy"] == 2
    assert reloads == recorded_reloads()


def test_the_jacobians_written_out_for_the_conditions_are_the_oracles(O):
    rng = np.random.default_rng(3)
    y, p = rng.uniform(-1, 1, (8, 3)), PC.robertson_params(8)
    for model, size in (("robertson_ode", 1), ("robertson", 0)):
        J = PC.jacobian(model, y, p)
        for b in range(8):
            for j in range(3):
                assert np.array_equal(J[b, :, j], O.model_jac_mul(PC.ORACLE_MODEL[model], y[b], p[b], np.eye(3)[j], model_size=size)), (model, b, j)
    assert np.array_equal(PC.mass("robertson"), np.stack([O.model_mass_gemv(PC.ORACLE_MODEL["robertson"], np.eye(3)[j], p[0], np.zeros(3), 0.0) for j in range(3)], axis=1))


def test_first_max_partial_pivoting_in_numpy():
    A = np.array([[[1.0, 2.0, 3.0], [-1.0, 5.0, 6.0], [0.5, 9.0, 10.0]],      # a tie in column 0: the first maximum stays; row 2 wins column 1
                  [[0.0, 1.0, 0.0], [2.0, 0.0, 0.0], [0.0, 0.0, 0.0]],        # row 1 wins column 0, then a zero pivot in the last place
                  [[np.nan, 1.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]],     # a NaN on the diagonal stays (nothing is greater), and is no zero
                  [[1.0, 1.0, 0.0], [np.nan, 1.0, 0.0], [2.0, 0.0, 1.0]]])    # a NaN below the diagonal never wins
    P, zero = PC.pivot_rows(A)
    assert P[:3].tolist() == [[0, 2, 2], [1, 1, 2], [0, 1, 2]] and P[3, 0] == 2 and zero.tolist() == [False, True, False, False]


def test_robertson_at_the_benchs_tolerances_has_identity_pivots_in_every_lane(O):
    assert PC.identity_condition(192)


def test_the_robertson_dae_leaves_the_identity_uniformly_once_c_exceeds_its_threshold(O):
    assert PC.dae_condition(192)


def test_the_lanes_of_the_mixed_group_disagree_and_its_neighbours_keep_the_identity(O):
    assert PC.mixed_condition()
