"""Extracts the Tsit45 data of the reference into tests/golden/reference_tsit45.json (the tests read only the JSON).

    python tests/golden/make_reference_tsit45.py [reference root, default /root/reference]

* tableau: `a`, `b`, `c`, `d`, `beta`, order of Tableau::tsit45 (crates/diffsol/src/ode_solver/tableau.rs): the literals of the source, and the first column of `a`
  computed as the source computes it (a(i,0) = c(i) - sum_{j=1}^{i-1} a(i,j), summed left to right from zero; last row = b).
* order_condition_residuals: max |sum(b) - 1|, max_i |sum_j a_ij - c_i| and max_i |d_i - (b_i - bhat_i)| cannot be formed (the source holds d, not bhat), so the
  d-consistency recorded here is |sum(d)| (sum(b) = sum(bhat) = 1 for two consistent weight sets).  Measured on the reference's own constants.
* snapshots: the insta counters of the Tsit45 snapshot tests in explicit_rk.rs whose problems the model set has: test_tsit45_nalgebra_exponential_decay.
  test_tsit45_nalgebra_heat1d_diffsl (93 steps, 11 failures) is left out: its problem is a DiffSL text with 10 states (heat1d_diffsl_problem::<M, _, 10>) — the
  built-in `heat1d` of the model set was not shown to be the same discretisation and boundary treatment, and 10 states is outside what the Tsit45 kernel accepts.
"""
import json
import os
import re
import sys

ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
src = open(os.path.join(ref, "crates/diffsol/src/ode_solver/tableau.rs")).read()
body = src[src.index("pub fn tsit45("):]
body = body[: body.index("pub fn new(")]
body = re.sub(r"//[^\n]*", "", body)  # the commented matrices are not data


def num(tok):
    tok = tok.strip()
    if tok.endswith("zero()"):
        return 0.0
    if tok.endswith("one()"):
        return 1.0
    m = re.search(r"from_f64\(\s*(-?[0-9_.eE+-]+)\s*\)", tok)
    return float(m.group(1).replace("_", ""))


def vec_after(name):
    m = re.search(r"let\s+(?:mut\s+)?%s\s*=\s*M::(?:V::)?from_vec\((?:\s*\d+\s*,\s*\d+\s*,)?\s*vec!\[(.*?)\]\s*," % name, body, re.S)
    items = re.findall(r"M::T::(?:zero\(\)|one\(\)|from_f64\([^)]*\)\s*\.unwrap\(\))", m.group(1))
    return [num(t) for t in items]


c, b, d, beta_flat = vec_after("c"), vec_after("b"), vec_after("d"), vec_after("beta")
assert len(c) == len(b) == len(d) == 7 and len(beta_flat) == 28
a = [[0.0] * 7 for _ in range(7)]
for i, j, v in re.findall(r"a\.set_index\(\s*(\d)\s*,\s*(\d)\s*,\s*M::T::from_f64\(\s*(-?[0-9_.eE+-]+)\s*\)", body):
    a[int(i)][int(j)] = float(v.replace("_", ""))
for i in range(1, 7):
    a_sum = 0.0
    for j in range(1, i):
        a_sum += a[i][j]
    a[i][0] = c[i] - a_sum
for j in range(6):
    a[6][j] = b[j]
beta = [beta_flat[q * 7:(q + 1) * 7] for q in range(4)]  # column-major 7 x 4 in the source: one power of theta per block
order = int(re.search(r"let order = (\d+);", body).group(1))


def seqsum(v):
    s = 0.0
    for x in v:
        s += x
    return s


resid = {"sum_b_minus_1": abs(seqsum(b) - 1.0), "max_row_sum_a_minus_c": max(abs(seqsum(a[i]) - c[i]) for i in range(7)), "abs_sum_d": abs(seqsum(d))}

ex = open(os.path.join(ref, "crates/diffsol/src/ode_solver/explicit_rk.rs")).read()
blk = ex[ex.index("fn test_tsit45_nalgebra_exponential_decay()"):]
blk = blk[: blk.index("#[test]")]
snap = {k: int(v) for k, v in re.findall(r"(number_of_[a-z_]+): (\d+)", blk)}
out = {"tableau": {"a": a, "b": b, "c": c, "d": d, "beta": beta, "order": order, "stages": 7}, "order_condition_residuals": resid,
       "snapshots": {"exponential_decay": {"reference_test": "ode_solver/explicit_rk.rs::test_tsit45_nalgebra_exponential_decay", **snap}}}
dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_tsit45.json")
with open(dst, "w") as f:
    json.dump(out, f, indent=1)
print(dst, resid, snap)
