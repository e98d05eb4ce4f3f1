"""The lock-step fast BDF kernel with the default options (k_bdf_adaptive<.., FAST, WAVE, DEFOPT>: the instantiation bench.py times) with its step loop free of
spill reloads (DSH_STEP_NO_RELOAD in csrc/dsh_adaptive_kernel.hpp: the next save point a wavefront-uniform value that is NaN behind the last column; profiles/
pivot_facts.md), against the general fast kernel <.., FAST, WAVE, DEFOPT = false>, which keeps the next save point and the column count as they were: the same call,
bit for bit.  The cases are those of the row permutation of the Newton solves: forming the pivot facts once per factorisation was built with this change, held these
bits, measured slower and was left out (profiles/pivot_facts.md, section 4); the cases stay for whoever returns to it, and they run the save-point logic on groups
that end early, fail, or have one live lane.

The call is routed to the general kernel as tests/test_gpu_wave_max_raw.py does it (max_steps = default + 1, nothing else changed) and compared with array_equal on
the bit patterns: the states at every save point, the five per-member counters, status and ncols.

Sizes: 64 members (one full group), 65 (a second group of one member and 63 shadow lanes), 192 (three groups).  Cases, each with its condition established on the
CPU (tests/pivot_facts_cases.py: the oracle's lock-step group, first-max partial pivoting of M - c J in numpy along its accepted steps) and asserted here again:
  * identity everywhere: the Robertson ODE at bench.py's tolerances and save points;
  * a uniform permutation that is not the identity, and a change between factorisations: the Robertson DAE, whose row 2 wins column 0 once c (1 - k1) > 1;
  * lanes of one wavefront disagree: 192 linear members, the second group with k1 of both signs (row 1 wins column 0 for k1 < 0 once c |k1| > 1/2), its neighbours
    with the identity everywhere;
  * NaN lanes: the NaN and 1e308 members of tests/test_gpu_wave_max_raw.py.  A NaN pivot is not a zero pivot: the groups fail as before, in both kernels alike, and
    their unwritten columns are filled behind the loop from a column count that the new save-point test no longer reads per step.
No input that reaches the zero-pivot exit (LuSolveFailed) was found: profiles/pivot_facts.md, section 4."""
import numpy as np
import pytest

import pivot_facts_cases as PC
from bench import robertson_params, T_EVAL, RTOL, ATOL
from test_gpu_wave_max_raw import both

gpu = pytest.mark.gpu


@gpu
@pytest.mark.parametrize("nb", [64, 65, 192])
def test_bits_of_the_general_kernel_with_identity_pivots_everywhere(nb, O):
    assert PC.identity_condition(nb)
    y, s, st, nc = both("robertson_ode", 1, 3, robertson_params(192)[:nb], ATOL, RTOL, T_EVAL)
    assert (st == 0).all() and (nc == len(T_EVAL)).all() and (s[0] > 50).all() and (s[2] > 10).all(), "the general kernel's run is not the solve the case was meant to be"
    print(f"identity, nb = {nb}: steps per group {[int(s[0, g]) for g in range(0, nb, 64)]}, factorisations {[int(s[2, g]) for g in range(0, nb, 64)]}")


@gpu
@pytest.mark.parametrize("nb", [64, 65, 192])
def test_bits_of_the_general_kernel_when_the_permutation_changes_between_factorisations(nb, O):
    assert PC.dae_condition(nb)
    y, s, st, nc = both("robertson", 0, 3, robertson_params(192)[:nb], ATOL, RTOL, T_EVAL)
    assert (st == 0).all() and (nc == len(T_EVAL)).all() and (s[0] > 100).all() and (s[2] > 10).all(), "the general kernel's run is not the solve the case was meant to be"
    assert np.allclose(y.sum(axis=1), 1.0, atol=1e-4), "the algebraic equation of the DAE does not hold: not a solve of the model"
    print(f"DAE, nb = {nb}: steps per group {[int(s[0, g]) for g in range(0, nb, 64)]}, factorisations {[int(s[2, g]) for g in range(0, nb, 64)]}")


@gpu
def test_bits_of_the_general_kernel_when_the_lanes_of_the_second_group_disagree(O):
    assert PC.mixed_condition()
    p = PC.mixed_params()
    y, s, st, nc = both("robertson_ode", 1, 3, p, PC.MIXED_ATOL, PC.MIXED_RTOL, PC.MIXED_T_EVAL)
    assert (st == 0).all() and (nc == len(PC.MIXED_T_EVAL)).all() and (s[2] > 3).all(), "the general kernel's run is not the solve the case was meant to be"
    assert np.isfinite(y).all()  # no accuracy to hold the run to: the tolerance is loose on purpose, so that the step size passes the pivot threshold
    print(f"mixed: steps per group {[int(s[0, g]) for g in (0, 64, 128)]}, factorisations {[int(s[2, g]) for g in (0, 64, 128)]}")


@gpu
def test_bits_of_the_general_kernel_when_a_pivot_is_nan():
    y, s, st, nc = both("robertson_ode", 1, 3, PC.nan_params(), ATOL, RTOL, T_EVAL)
    g0, g1, g2 = slice(0, 64), slice(64, 128), slice(128, 192)
    print(f"NaN lanes: per group (status, columns, steps, Newton failures): {[(sorted(set(st[g].tolist())), sorted(set(nc[g].tolist())), int(s[0, g][0]), int(s[4, g][0])) for g in (g0, g1, g2)]}")
    assert (st[g0] == 0).all() and (nc[g0] == len(T_EVAL)).all(), "the group without a non-finite member was meant to succeed"
    assert (st[g1] != 0).all() and (s[0, g1] > 0).all() and (s[4, g1] > 0).all(), "the group with the overflowing member was meant to take steps and then fail as a whole"
    assert (st[g2] != 0).all(), "a lock-step group with a NaN member was meant to fail as a whole"
