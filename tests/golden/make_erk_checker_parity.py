"""Record what the Tsit45 checkers (tests/erk_ref.py, erk_sens_ref.py, erk_out_ref.py) compute into tests/golden/erk_checker_parity.json, as hashes:

    python -m diffsol_amd.build && python tests/golden/make_erk_checker_parity.py

The fixture was recorded ONCE, at the commit before the three checker programs became one, and is not regenerated: tests/test_erk_checker_parity.py runs the cases
below again and compares, so a change of the checker that moves one bit of one array shows.  Only the public functions of the three modules are used.

Every case runs with the portable pow (set_det_pow(True)) on a model whose right-hand side, outputs and parameter derivatives are + - * / alone, so no byte depends
on libm and the fixture holds on any x86-64 host.  Runs with libm's pow stay pinned by the golden tests against the reference's snapshots.

Per case: the sha256 of the raw bytes of every returned array (prefixed with its dtype and shape), by name in the order returned; in clear `failed` and the first
member's `stats` row (solve_ensemble) or the counters (solve_to_points)."""
import hashlib
import json
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(_HERE), os.path.dirname(os.path.dirname(_HERE))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import erk_out_ref as EO  # noqa: E402
import erk_ref as E  # noqa: E402
import erk_sens_ref as S  # noqa: E402
from helpers import ORACLE_MODEL  # noqa: E402
from test_erk_ref_options import DYDT_Y2  # noqa: E402

FIXTURE = os.path.join(_HERE, "erk_checker_parity.json")
MODS = {"plain": E, "sens": S, "out": EO}

# OSC_OUT of tests/test_gpu_erk_out.py, character for character (one output of three states, which reads t; no exp, no pow)
OSC_OUT = """
in = [w]
w { 1 }
u_i { x = 1, y = 0, z = 0.5 }
F_i { w * y, -w * x, -0.3 * z + 0.1 * x }
out_i { x * y + t }
"""
TWINS = {"dydt_y2_twin": DYDT_Y2, "osc_out": OSC_OUT}

P5 = np.array([[0.1, 1.0], [1.0, 2.0], [2.0, 0.5], [0.5, 1.5], [0.25, 3.0]])          # exponential_decay: (k, y0); five members, so group 3 ends ragged
P5_AGREE = np.array([[0.1, 1.0]] * 3 + [[0.25, 3.0]] * 2)                              # the members of a lock-step group agree on the root's step
A5 = np.array([[1.0], [0.05], [0.8], [0.02], [1.2]])                                   # dy/dt = a y^2: blow-up at t = 0.5 / a
W5 = np.array([[0.5], [0.8], [1.0], [1.3], [1.5]])
T = [0.5, 1.0, 2.5, 6.0]
T_BLOW = [0.2, 0.4, 0.45, 0.6]
ATOL_ROWS = np.array([1e-6, 1e-6])[None, :] * np.array([[1.0], [0.1], [10.0], [3.0], [0.3]])
BLOW_TOL = dict(rtol=1e-6, atol=[1e-8] * 3)


def _cases():
    c = []

    def ens(name, mode, model, p, t_eval, **kw):
        c.append(dict(name=name, mode=mode, fn="solve_ensemble", model=model, args=(p, t_eval), kw=kw))

    def pts(name, mode, model, p, t_points, **kw):
        c.append(dict(name=name, mode=mode, fn="solve_to_points", model=model, args=(p, t_points), kw=kw))

    for mode in MODS:
        for g in (1, 3):
            tag = f"{mode}/g{g}"
            ens(f"decay/{tag}", mode, "exponential_decay", P5, T, group=g)
            ens(f"decay/{tag}/member_atol_t0", mode, "exponential_decay", P5, [1.5 + t for t in T], group=g, atol=ATOL_ROWS, t0=1.5)
            ens(f"decay/{tag}/max_steps_cuts_some", mode, "exponential_decay", P5, T, group=g, options=dict(max_steps=16))
            ens(f"blow_up/{tag}/max_error_test_failures_1", mode, "dydt_y2_twin", A5, T_BLOW, group=g, options=dict(max_steps=100000, max_error_test_failures=1), **BLOW_TOL)
        ens(f"decay/{mode}/g3/stop_time_at_t0", mode, "exponential_decay", P5, [1.5], group=3, t0=1.5)
        ens(f"decay/{mode}/g1/stop_time_behind_h0", mode, "exponential_decay", P5, [2.5], group=1, t0=1.5, h0=-1.0)
    for mode in ("plain", "out"):
        for g in (1, 3):
            tag = f"{mode}/g{g}"
            ens(f"decay/{tag}/steps_cap_4", mode, "exponential_decay", P5, [6.0], group=g, steps_cap=4)
            ens(f"decay/{tag}/steps_cap_64", mode, "exponential_decay", P5, [6.0], group=g, steps_cap=64)
            ens(f"root/{tag}", mode, "exponential_decay_with_root", P5 if g == 1 else P5_AGREE, T, group=g)
            ens(f"osc_out/{tag}/t0", mode, "osc_out", W5, [-2.0, -1.0, 1.0], group=g, rtol=1e-6, atol=[1e-8] * 3, t0=-2.0)
        ens(f"root/{mode}/g3/members_disagree", mode, "exponential_decay_with_root", P5, T, group=3)
        ens(f"root/{mode}/g3/steps_cap_64", mode, "exponential_decay_with_root", P5_AGREE, [6.0], group=3, steps_cap=64)
        ens(f"root/{mode}/g1/steps_cap_4", mode, "exponential_decay_with_root", P5, [6.0], group=1, steps_cap=4)
        ens(f"decay/{mode}/g3/steps_cap_4/stop_time_behind_h0", mode, "exponential_decay", P5, [1.0], group=3, steps_cap=4, h0=-1.0)
    for label, sa in (("none", None), ("scalar", 1e-9), ("per_state", [1e-9, 1e-7])):
        ens(f"decay/sens/g3/sens_atol_{label}", "sens", "exponential_decay", P5, T, group=3, sens_rtol=1e-8, sens_atol=sa)
        pts(f"points/sens/sens_atol_{label}", "sens", "exponential_decay", [0.1, 1.0], [0.0, 1.0, 2.0, 5.0], sens_rtol=1e-8, sens_atol=sa)
    ens("blow_up/sens/g3/sens_atol_none", "sens", "dydt_y2_twin", A5, T_BLOW, group=3, sens_atol=None, options=dict(max_steps=100000, max_error_test_failures=3), rtol=0.1, atol=[1e-2] * 3)
    for label, oa in (("scalar", 1e-12), ("per_output", [1e-12, 1e-11])):
        ens(f"decay/out/g3/out_atol_{label}", "out", "exponential_decay", P5, T, group=3, out_rtol=1e-10, out_atol=oa)
        ens(f"decay/out/g1/steps_cap_64/out_atol_{label}", "out", "exponential_decay", P5, [6.0], group=1, steps_cap=64, out_rtol=1e-10, out_atol=oa)
    ens("osc_out/out/g3/out_atol_scalar", "out", "osc_out", W5, [1.0, 4.0], group=3, rtol=1e-6, atol=[1e-8] * 3, out_rtol=1e-9, out_atol=1e-11)
    ens("osc_out/out/g3/out_atol_per_output", "out", "osc_out", W5, [1.0, 4.0], group=3, rtol=1e-6, atol=[1e-8] * 3, out_rtol=1e-9, out_atol=[1e-11])
    for g in (1, 3):
        ens(f"decay/out/g{g}/integrate_out_off", "out", "exponential_decay", P5, T, group=g, integrate_out=False)
        ens(f"root/out/g{g}/steps_cap_64/integrate_out_off", "out", "exponential_decay_with_root", P5_AGREE, [6.0], group=g, steps_cap=64, integrate_out=False)
    for tstop in (False, True):
        pts(f"points/plain/use_tstop_{tstop}", "plain", "exponential_decay", [0.1, 1.0], [0.0, 1.0, 2.0, 5.0], use_tstop=tstop)
        pts(f"points/plain/dydt_y2/use_tstop_{tstop}", "plain", "dydt_y2_twin", [0.3], [0.25, 0.5, 1.0], use_tstop=tstop, **BLOW_TOL)
    for on in (False, True):
        pts(f"points/out/integrate_out_{on}", "out", "exponential_decay", [0.1, 1.0], [0.0, 1.0, 2.0, 5.0], integrate_out=on)
    pts("points/out/osc_out/out_atol", "out", "osc_out", [1.3], [0.5, 4.0], rtol=1e-8, atol=[1e-10] * 3, out_rtol=1e-9, out_atol=[1e-11])
    pts("points/sens/osc_out/t0", "sens", "osc_out", [1.3], [1.0, 4.0], rtol=1e-8, atol=[1e-10] * 3, t0=0.5)
    assert len({k["name"] for k in c}) == len(c)
    return c


CASES = _cases()

_ids = {}


def model_id(mod, name):
    """a built-in model's id, or the id of a DiffSL text's host twin in the registry behind `mod`"""
    if name in ORACLE_MODEL:
        return ORACLE_MODEL[name]
    if (mod, name) not in _ids:
        import diffsl_models as DM
        _ids[mod, name] = mod.load_external_model(DM.host_model_so(TWINS[name])[0])
    return _ids[mod, name]


def _hash(a):
    a = np.asarray(a)
    return "%s%s:%s" % (a.dtype, list(a.shape), hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest())


def run_case(case):
    """one case through its module, as the fixture records it: dict(name, arrays {name: hash or None}, and failed / stats0 or counters in clear)"""
    mod = MODS[case["mode"]]
    mod.set_det_pow(True)
    try:
        r = getattr(mod, case["fn"])(model_id(mod, case["model"]), *case["args"], **case["kw"])
    finally:
        mod.set_det_pow(False)
    if case["fn"] == "solve_ensemble":
        arrays = {k: (None if v is None else _hash(v)) for k, v in r.items() if k != "failed"}
        return dict(name=case["name"], arrays=arrays, failed=int(r["failed"]), stats0=[int(v) for v in r["stats"][0]])
    names = {"plain": ("y",), "sens": ("y", "sens"), "out": ("y", "g")}[case["mode"]]
    arrays = {k: (None if v is None else _hash(v)) for k, v in zip(names, r[:-1])}
    return dict(name=case["name"], arrays=arrays, counters={k: int(v) for k, v in r[-1].items()})


if __name__ == "__main__":
    out = [run_case(k) for k in CASES]
    with open(FIXTURE, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(o) for o in out) + "\n]\n")
    print("wrote", FIXTURE, len(out), "cases")
