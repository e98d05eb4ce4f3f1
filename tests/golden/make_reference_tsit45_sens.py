"""Extracts the data of the reference's Tsit45 snapshot test WITH FORWARD SENSITIVITIES into tests/golden/reference_tsit45_sens.json (the tests read only the JSON).

    python tests/golden/make_reference_tsit45_sens.py <reference root>

* snapshot: the insta counters of test_tsit45_nalgebra_exponential_decay_sens (crates/diffsol/src/ode_solver/explicit_rk.rs): the solver's statistics and the
  right-hand side's OpStatistics (number_of_calls, number_of_jac_muls).
* problem: the constants of exponential_decay_problem_sens (crates/diffsol/src/ode_equations/test_models/exponential_decay.rs): p = [k, y0], sens_rtol, sens_atol, the
  number of solution points (t = 0, 1, .., npoints - 1).  rtol, atol and h0 are the builder's defaults (ode_solver/builder.rs), which this problem does not set.
* acceptance: the bounds test_ode_solver (ode_solver/mod.rs) asserts on the weighted error norm of the states and of the sensitivities; it weighs both with the
  problem's STATE tolerances (rtol, atol), not with sens_rtol / sens_atol (asserted below on the source).
Only numbers go into the JSON.
"""
import json
import os
import re
import sys

if len(sys.argv) != 2:
    sys.exit(__doc__)
ref = sys.argv[1]


def read(rel):
    with open(os.path.join(ref, rel)) as f:
        return f.read()


ex = read("crates/diffsol/src/ode_solver/explicit_rk.rs")
blk = ex[ex.index("fn test_tsit45_nalgebra_exponential_decay_sens()"):]
blk = blk[: blk.index("#[test]")]
snap = {k: int(v) for k, v in re.findall(r"(number_of_[a-z_]+): (\d+)", blk)}
assert "exponential_decay_problem_sens::<M>(false)" in blk and "tsit45_sens()" in blk

md = read("crates/diffsol/src/ode_equations/test_models/exponential_decay.rs")
pb = md[md.index("pub fn exponential_decay_problem_sens<"):]
pb = pb[: pb.index("#[allow(clippy::type_complexity)]")]
num = r"([0-9][0-9_.eE+-]*)"
k = float(re.search(r"let k = %s;" % num, pb).group(1))
y0 = float(re.search(r"let y0 = %s;" % num, pb).group(1))
sens_rtol = float(re.search(r"\.sens_rtol\(%s\)" % num, pb).group(1))
sens_atol = [float(x) for x in re.search(r"\.sens_atol\(\[([^\]]*)\]\)", pb).group(1).split(",")]
npoints = int(re.search(r"for i in 0\.\.(\d+)", pb).group(1))
assert ".rtol(" not in pb and ".atol(" not in pb and ".h0(" not in pb  # the builder's defaults

bd = read("crates/diffsol/src/ode_solver/builder.rs")
nw = bd[bd.index("pub fn new() -> Self {"):]
nw = nw[: nw.index("\n    }\n")]
rtol = float(re.search(r"let default_rtol = M::T::from_f64\(%s\)" % num, nw).group(1))
atol = [float(x) for x in re.findall(r"M::T::from_f64\(%s\)" % num, re.search(r"let default_atol = vec!\[(.*?)\];", nw, re.S).group(1))]
assert re.search(r"\brtol: default_rtol,", nw) and re.search(r"\batol: default_atol\.clone\(\),", nw) and re.search(r"\bh0: M::T::one\(\),", nw)
h0 = 1.0

mod = read("crates/diffsol/src/ode_solver/mod.rs")
tb = mod[mod.index("pub fn test_ode_solver<"):]
tb = tb[: tb.index("pub fn setup_test_adjoint<")]
bounds = [float(x) for x in re.findall(r"error_norm < M::T::from_f64\(([0-9.]+)\)", tb)]
assert len(bounds) == 2 and tb.count("squared_norm(&sens_point.state, atol, rtol)") == 1  # states first, then the sensitivities with the same (rtol, atol)

out = {"snapshot": snap,
       "problem": {"p": [k, y0], "rtol": rtol, "atol": atol, "h0": h0, "sens_rtol": sens_rtol, "sens_atol": sens_atol, "npoints": npoints},
       "acceptance": {"state_bound": bounds[0], "sens_bound": bounds[1]}}
dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_tsit45_sens.json")
with open(dst, "w") as f:
    json.dump(out, f, indent=1)
print(dst, out)
