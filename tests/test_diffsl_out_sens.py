"""Output sensitivities in the DiffSL front end (diffsol_amd/host/diffsl.hpp, targets HipOutSens / HostOutSens): the tangents of out_i along a state direction
(out.jac_mul of the reference) and along a parameter direction (out.sens_mul), which solve_dense_sensitivities adds per save point and parameter
(crates/diffsol/src/ode_solver/sensitivities.rs:360-397).  No GPU: the generated host twin is compiled with g++ and evaluated."""
import hashlib
import json
import os

import numpy as np
import pytest

import diffsl_models as D
import out_sens_models as M

EPS = np.finfo(float).eps
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "diffsl_target_sha256.json")


def _points(seed, count=50):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.5, 2.0, (count, 4))  # x, y, k, y0


def _directions(rng, dim):
    return [np.eye(dim)[i] for i in range(dim)] + [rng.uniform(-1.0, 1.0, dim) for _ in range(3)]


def test_rational_model_tangents_equal_the_hand_written_derivatives():
    """out_i { k*x*y + y0, x / (y + k), x + y }: only + - * / occur, so a different association order of the same derivative differs by at most a few roundings of
    the sum of the absolute terms: 16 eps sum|terms|."""
    tw = M.HostTwin(M.RATIONAL)
    assert (tw.n, tw.np, tw.nout) == (2, 2, 3)
    rng = np.random.default_rng(1)
    for x, y, k, y0 in _points(2):
        d = y + k
        # rows: outputs; columns: (x, y) and (k, y0)
        jx = np.array([[k * y, k * x], [1.0 / d, -x / (d * d)], [1.0, 1.0]])
        jp = np.array([[x * y, 1.0], [-x / (d * d), 0.0], [0.0, 0.0]])
        assert np.array_equal(tw.out(0.0, [x, y], [k, y0]), np.array([k * x * y + y0, x / (y + k), x + y]))
        for v in _directions(rng, 2):
            for got, jac in ((tw.jac_mul(0.0, [x, y], [k, y0], v), jx), (tw.sens_mul(0.0, [x, y], [k, y0], v), jp)):
                terms = jac * v[None, :]
                want, bound = terms.sum(axis=1), 16 * EPS * np.abs(terms).sum(axis=1)
                print("rational", got, want, bound)
                assert (np.abs(got - want) <= bound).all(), (got, want, bound)


def test_transcendental_model_tangents_equal_central_differences_of_the_generated_out():
    """out_i { exp(-k*x) * sin(y + y0), sqrt(x*x + k) / (1 + y*y), pow(x, 1.5) * tanh(k*y) } on [0.5, 2]^4: central differences of dsl_out itself with the step
    1e-5 max(1, |argument|).  Third derivatives are of order 10, so the truncation error is about 1e-9 and the rounding error about 1e-11: the tolerance
    1e-7 max(1, |value|) leaves two orders of margin (a direction of up to two components of size <= 1 adds at most a factor of two)."""
    tw = M.HostTwin(M.TRANSCENDENTAL)
    rng = np.random.default_rng(3)
    for x, y, k, y0 in _points(4):
        st, par = np.array([x, y]), np.array([k, y0])
        jx, jp = np.empty((3, 2)), np.empty((3, 2))
        for i in range(2):
            h = 1e-5 * max(1.0, abs(st[i]))
            e = np.eye(2)[i] * h
            jx[:, i] = (tw.out(0.0, st + e, par) - tw.out(0.0, st - e, par)) / (2 * h)
            h = 1e-5 * max(1.0, abs(par[i]))
            e = np.eye(2)[i] * h
            jp[:, i] = (tw.out(0.0, st, par + e) - tw.out(0.0, st, par - e)) / (2 * h)
        for v in _directions(rng, 2):
            for got, jac in ((tw.jac_mul(0.0, st, par, v), jx), (tw.sens_mul(0.0, st, par, v), jp)):
                want = jac @ v
                tol = 1e-7 * np.maximum(1.0, np.abs(got))
                print("transcendental", got, want, np.abs(got - want))
                assert (np.abs(got - want) <= tol).all(), (got, want)


@pytest.mark.parametrize("name", ["ROBERTSON_ODE", "spm(20)", "spm_dae(20)"])
def test_the_three_existing_targets_generate_the_bytes_of_the_parent_commit(name):
    """Cached code objects and recorded JIT manifests are keyed by the generated text: the new targets must not change a byte of the old ones.  The digests were taken
    from the front end before the output-sensitivity targets existed."""
    from diffsol_amd import diffsl
    code = {"ROBERTSON_ODE": D.ROBERTSON_ODE, "spm(20)": D.spm(20), "spm_dae(20)": D.spm_dae(20)}[name]
    with open(GOLDEN) as f:
        want = json.load(f)[name]
    assert hashlib.sha256(code.encode()).hexdigest() == want["text_sha256"], "the DiffSL text itself changed: the recorded digests no longer describe it"
    for target in (diffsl.TARGET_HIP_STATIC, diffsl.TARGET_HIP_DYNAMIC, diffsl.TARGET_HOST_C):
        src = diffsl.generate(code, target)[0]
        assert hashlib.sha256(src.encode()).hexdigest() == want["target_%d" % target], (name, target)


def test_models_without_outputs_or_without_inputs_are_refused_by_name():
    from diffsol_amd import diffsl
    from diffsol_amd._ffi import DiffsolHipError
    no_out = "in = [k]\nu_i { x = 1 }\nF_i { -k * x }\n"
    no_in = "u_i { x = 1 }\nF_i { -x }\nout_i { 2 * x }\n"
    for target in (diffsl.TARGET_HIP_OUT_SENS, diffsl.TARGET_HOST_OUT_SENS):
        with pytest.raises(DiffsolHipError, match="no out_i") as e:
            diffsl.generate(no_out, target)
        assert "no inputs" not in str(e.value)
        with pytest.raises(DiffsolHipError, match="no inputs") as e:
            diffsl.generate(no_in, target)
        assert "no out_i" not in str(e.value)
    # the other targets still take both
    assert diffsl.generate(no_out, diffsl.TARGET_HOST_C)[1]["nout"] == 0 and diffsl.generate(no_in, diffsl.TARGET_HOST_C)[1]["no_inputs"]


def test_device_source_has_the_three_component_functions_and_separate_roots():
    """the device form: accessor style, one switch per function; a root that is the structural zero is the literal 0.0 (the kernel still adds it)"""
    from diffsol_amd import diffsl
    src, d, _ = diffsl.generate(M.RATIONAL, diffsl.TARGET_HIP_OUT_SENS)
    assert (d["n"], d["nparams"], d["nout"]) == (2, 2, 3)
    for fn in ("jit_out_component", "jit_out_jac_component", "jit_out_sens_component"):
        assert src.count("double " + fn + "(") == 1
    assert "kOutSensN = 2, kOutSensNP = 2, kOutSensNOut = 3" in src
    sens_part = src[src.index("jit_out_sens_component"):]
    assert "return 0.0;" in sens_part and "X(" in sens_part and "x[" not in src
