"""Device-resident Tsit45 (k_erk_resident, dsh_erk_kernel.hpp) against the CPU checkers with everything the other three Tsit45 files hold fixed let loose: the
start time and the first-step hint, the solver options the kernel reads (max_steps, max_error_test_failures, min_timestep, the two controller constants), the four it
ignores, and every exit — StepSizeTooSmall (1), TooManyErrorTestFailures (2), StopTimeBeforeCurrentTime (5), StopTimeAtCurrentTime (6), RootBatchMismatch (20),
MaxStepsExceeded (99) — on the plain kernel, the kernel with sensitivities and the kernel with integrated outputs, at save points and in steps mode.

Everything is bitwise: status, the five counters, ncols, root_idx, t_root, the columns (NaN where NaN), the step times, and the totals of the launch.  A member that
fails is part of the result like one that succeeds.  Every case asserts on the CHECKER's result that it reaches the exit it is about (and, where it is meant to mix,
that members of one wavefront end differently) before the device is compared: a case that no longer exercises its exit fails.

Ensembles have 1, 65 or 130 members (130: the third wavefront has 2 live lanes and 62 that shadow its first member).  The DiffSL texts are those of the other files,
character for character, with shared atol and more than one member: the kernels they instantiate are the ones those files compile.  Per-member atol and the single
member run on the built-in models, which are compiled into the library."""
import numpy as np
import pytest

import erk_out_ref as EO
import erk_ref as E
import erk_sens_ref as S
import out_sens_models as OSM
import test_gpu_erk as P
import test_gpu_erk_out as PO
import test_gpu_erk_sens as PS
from helpers import ORACLE_MODEL

pytestmark = pytest.mark.gpu

ENTRIES = ("plain", "steps", "sens", "out", "steps_out")
STEPS_CAP = 48          # columns of the steps entries: runs with more accepted steps count them and store the first 48, on both sides
DECAY_T = [0.5, 1.0, 2.5, 6.0]
DECAY_TOL = dict(rtol=1e-6, atol=[1e-6, 1e-6])
PI_PAIR = dict(pi_control_integral=0.3, pi_control_proportional=0.4)   # the proportional term reads the previous error norm: the defaults (0.5, 0) never do


@pytest.fixture(scope="module")
def H():
    import diffsol_amd
    return diffsol_amd


@pytest.fixture(autouse=True)
def det_pow():
    for m in (E, S, EO):
        m.set_det_pow(True)
    yield
    for m in (E, S, EO):
        m.set_det_pow(False)


_models = {}
_TEXTS = {"dydt_y2": P.DYDT_Y2, "osc_out": PO.OSC_OUT, "transcendental": OSM.TRANSCENDENTAL}


def model_of(H, name):
    """dict(dev, size, ref (the checker's id), nout) of a built-in model or of one of the DiffSL texts above (compiled once per session, its host twin loaded
    into the registry of the checker library)"""
    if name not in _models:
        if name not in _TEXTS:   # (the registry has a run-time-sized dydt_y2 of its own: the texts go first)
            _models[name] = dict(dev=H.MODELS[name], size=0, ref=ORACLE_MODEL[name], keep=None)
        else:
            import diffsl_models as DM
            from diffsol_amd import diffsl
            m = diffsl.DiffslModel(_TEXTS[name])
            so, _ = DM.host_model_so(_TEXTS[name])
            _models[name] = dict(dev=m.model_id, size=0, ref=E.load_external_model(so), keep=m)
        _models[name]["nout"] = EO.model_dims(_models[name]["ref"])["nout"]
    return _models[name]


def solve_pair(H, entry, name, p, t_eval, group, *, rtol, atol, t0=0.0, h0=1.0, options=None, device_only=None, reference=True, sens_atol=(1e-6,)):
    """(device result, checker result, name of the column array) of one entry.  options: the five the checker takes, given to both sides; device_only: further
    fields of dsh_adaptive_options.  The steps entries integrate to t_eval[-1].  The sensitivities take part in the error test unless sens_atol is None, the integrated
    outputs do not."""
    m = model_of(H, name)
    dopt = dict(options or {}, **(device_only or {}))
    kw = dict(rtol=rtol, atol=atol, t0=t0, h0=h0, group=group, options=options)
    steps = entry.startswith("steps")
    cap = STEPS_CAP if steps else 0
    te = [t_eval[-1]] if steps else list(t_eval)
    if entry in ("plain", "steps"):
        dev = P.device_solve(H, m["dev"], m["size"], p, te, rtol, atol, group, steps_cap=cap, t0=t0, h0=h0, options=dopt)
        ref = E.solve_ensemble(m["ref"], p, te, steps_cap=cap, **kw) if reference else None
        return dev, ref, "y"
    if entry == "sens":
        dev = PS.device_solve(m["dev"], m["size"], p, te, rtol, atol, group, sens_atol=sens_atol, t0=t0, h0=h0, options=dopt)
        ref = S.solve_ensemble(m["ref"], p, te, sens_atol=sens_atol, **kw) if reference else None
        return dev, ref, "y"
    dev = PO.device_solve(m["dev"], m["size"], m["nout"], p, te, rtol, atol, group, steps_cap=cap, t0=t0, h0=h0, options=dopt)
    ref = EO.solve_ensemble(m["ref"], p, te, steps_cap=cap, **kw) if reference else None
    return dev, ref, "g"


def assert_exits_same(dev, ref, key, steps=False):
    """assert_same of the three Tsit45 files without the line that every member succeeds: the device against the checker, failing members included"""
    assert np.array_equal(dev["status"], ref["status"]), (np.flatnonzero(dev["status"] != ref["status"])[:8], dev["status"][:8], ref["status"][:8])
    assert np.array_equal(dev["stats"], ref["stats"]), np.flatnonzero((dev["stats"] != ref["stats"]).any(axis=1))[:8]
    for k in ("ncols", "root_idx"):   # the entry with sensitivities has neither (no root functions, no column count)
        if k in dev:
            assert np.array_equal(dev[k], ref[k]), (k, dev[k][:8], ref[k][:8])
    if "t_root" in dev:
        assert np.array_equal(dev["t_root"], ref["t_root"], equal_nan=True)
    assert np.array_equal(dev[key], ref[key], equal_nan=True), np.flatnonzero([not np.array_equal(a, b, equal_nan=True) for a, b in zip(dev[key], ref[key])])[:8]
    if "sens" in dev:
        assert np.array_equal(dev["sens"], ref["sens"], equal_nan=True)
    if steps:
        assert np.array_equal(dev["t"], ref["t"], equal_nan=True)
    assert dev["totals"][0] == int(dev["stats"][:, 0].sum()) and dev["totals"][3] == int(dev["stats"][:, 3].sum())
    assert dev["totals"][5] == int((dev["status"] != 0).sum()) == ref["failed"], (dev["totals"][5], int((dev["status"] != 0).sum()), ref["failed"])


def compare(H, entry, name, p, t_eval, group, **kw):
    dev, ref, key = solve_pair(H, entry, name, p, t_eval, group, **kw)
    assert_exits_same(dev, ref, key, steps=entry.startswith("steps"))
    return dev, ref, key


def same_result(a, b):
    """two device results bit for bit: every array, and the totals of the launch"""
    return set(a) == set(b) and all(a[k] == b[k] if k == "totals" else np.array_equal(a[k], b[k], equal_nan=True) for k in a)


def entries_of(name):
    return tuple(e for e in ENTRIES if not (e == "sens" and name.endswith("with_root")))


def decay_params(name, nb, group):
    """test_gpu_erk's sweep; in lock-step the members of a wavefront of the model with a root share one parameter set (they must agree on the crossing)"""
    if name.endswith("with_root") and group == 64:
        return np.repeat(P.params(name, (nb + 63) // 64), 64, axis=0)[:nb]
    return P.params(name, nb)


def member_atol(nb, name, group):
    f = 10.0 ** np.random.default_rng(nb).uniform(-1, 1, (nb, 1))
    if name.endswith("with_root") and group == 64:
        f = np.repeat(f[: (nb + 63) // 64], 64, axis=0)[:nb]
    return np.asarray(DECAY_TOL["atol"])[None, :] * f


# ------------------------------------------------------------------------------------------------------------------ a. start time
@pytest.mark.parametrize("group", [1, 64])
@pytest.mark.parametrize("at_t0", [True, False], ids=["first_save_point_is_t0", "first_save_point_after_t0"])
@pytest.mark.parametrize("t0", [1.5, -2.0])
def test_a_start_time_other_than_zero(H, t0, at_t0, group):
    """t0 enters the stage times, handle_tstop's round-off, theta of the dense output and the save-point comparisons.  OSC_OUT's output reads t: a stage time that
    started from zero shows in g"""
    t_eval = [t0 if at_t0 else t0 + 0.25, t0 + 1.0, t0 + 3.0]
    for nb in (65, 130):
        rng = np.random.default_rng(nb)
        for name, p, entries in (("osc_out", rng.uniform(0.5, 1.5, (nb, 1)), ("plain", "steps", "out", "steps_out")), ("transcendental", rng.uniform(0.5, 2.0, (nb, 2)), ("sens",))):
            for entry in entries:
                dev, ref, key = solve_pair(H, entry, name, p, t_eval, group, rtol=1e-6, atol=[1e-8] * (3 if name == "osc_out" else 2), t0=t0)
                assert ref["failed"] == 0 and not ref["status"].any()
                if entry == "out":   # the case is about t0: the same save points counted from zero give another integral
                    zero = EO.solve_ensemble(model_of(H, name)["ref"], p, [t - t0 for t in t_eval], rtol=1e-6, atol=[1e-8] * 3, group=group)
                    assert not np.array_equal(zero["g"][:, -1], ref["g"][:, -1])
                    assert np.array_equal(ref["g"][:, 0] == 0.0, np.full((nb, 1), at_t0))
                assert_exits_same(dev, ref, key, steps=entry.startswith("steps"))
    for name in ("exponential_decay", "exponential_decay_with_root"):   # one member, and per-member atol, on the built-in models
        for nb, atol in ((1, DECAY_TOL["atol"]), (65, member_atol(65, name, group))):
            for entry in entries_of(name):
                dev, ref, key = compare(H, entry, name, decay_params(name, nb, group), [t0 + t for t in ([0.0] if at_t0 else []) + DECAY_T], group, rtol=1e-6, atol=atol, t0=t0)
                assert ref["failed"] == 0 and not ref["status"].any()


# ------------------------------------------------------------------------------------------------------------------ b. first-step hint
@pytest.mark.parametrize("group", [1, 64])
@pytest.mark.parametrize("nb", [1, 130])
def test_b_the_first_step_hint_counts_by_its_sign_only(H, nb, group):
    """set_step_size (state.rs:1209-1277) computes the first step from the problem and takes the sign of h0: every positive hint gives the run of h0 = 1, on both sides"""
    p = decay_params("exponential_decay", nb, group)
    for entry in ENTRIES:
        base = None
        for h0 in (1e-3, 1.0, 10.0):
            dev, ref, key = compare(H, entry, "exponential_decay", p, DECAY_T, group, h0=h0, **DECAY_TOL)
            assert ref["failed"] == 0
            base = base or dev
            assert same_result(dev, base)


# ------------------------------------------------------------------------------------------------------------------ c. controller constants
@pytest.mark.parametrize("group", [1, 64])
@pytest.mark.parametrize("nb", [1, 65, 130])
def test_c_controller_constants_other_than_the_defaults(H, nb, group):
    p = decay_params("exponential_decay", nb, group)
    atol = member_atol(nb, "exponential_decay", group) if nb == 65 else DECAY_TOL["atol"]
    for entry in ENTRIES:
        dev, ref, key = solve_pair(H, entry, "exponential_decay", p, DECAY_T, group, rtol=1e-6, atol=atol, options=PI_PAIR)
        default = solve_pair(H, entry, "exponential_decay", p, DECAY_T, group, rtol=1e-6, atol=atol)[1]
        assert ref["failed"] == 0 and not ref["status"].any()                      # every member succeeds ...
        assert (ref["stats"][:, 0] != default["stats"][:, 0]).any()                # ... on another step sequence than the default pair's
        assert_exits_same(dev, ref, key, steps=entry.startswith("steps"))


# ------------------------------------------------------------------------------------------------------------------ d. ignored bounds
@pytest.mark.parametrize("group", [1, 64])
def test_d_the_four_step_size_bounds_of_the_options_are_not_read(H, group):
    """dsh_adaptive_options carries the BDF / SDIRK bounds of the step-size factor; the Tsit45 driver uses ExplicitRkConfig::default() (config.rs:141-160) whatever
    they hold: other values change no bit"""
    other = dict(max_timestep_growth=1.3, min_timestep_growth=1.1, max_timestep_shrink=0.7, min_timestep_shrink=0.2)
    nb = 130
    p = decay_params("exponential_decay", nb, group)
    for entry in ENTRIES:
        dev, ref, key = compare(H, entry, "exponential_decay", p, DECAY_T, group, device_only=other, **DECAY_TOL)
        default = solve_pair(H, entry, "exponential_decay", p, DECAY_T, group, reference=False, **DECAY_TOL)[0]
        assert ref["failed"] == 0 and same_result(dev, default)


# ------------------------------------------------------------------------------------------------------------------ e. step cap
def mixing_cap(need, nb, group):
    """a max_steps under which, per member (group 1), each of the first two wavefronts holds a member that finishes and one that does not; per group (group 64),
    one group finishes and another does not.  One member: one step short of what it needs."""
    if nb == 1:
        return int(need[0]) - 1
    if group == 64:
        return int(np.unique(need)[0])
    return int(np.median(need[:64]))


@pytest.mark.parametrize("group", [1, 64])
@pytest.mark.parametrize("nb", [1, 65, 130])
@pytest.mark.parametrize("name", ["exponential_decay", "exponential_decay_with_root"])
def test_e_step_cap(H, name, nb, group):
    """max_steps = 1, and a cap under which finishing members and capped members (status 99) share a wavefront; with the root model some members reach their root
    before the cap and others do not.  In lock-step the count is the group's"""
    p = decay_params(name, nb, group)
    atol = member_atol(nb, name, group) if nb == 65 else DECAY_TOL["atol"]
    for entry in entries_of(name):
        free = solve_pair(H, entry, name, p, DECAY_T, group, rtol=1e-6, atol=atol, reference=True)[1]
        need = free["stats"][:, 0]
        assert free["failed"] == 0
        k = mixing_cap(need, nb, group)
        for cap in (1, k) + ((k + 1,) if nb == 1 else ()):
            dev, ref, key = solve_pair(H, entry, name, p, DECAY_T, group, rtol=1e-6, atol=atol, options=dict(max_steps=cap))
            assert np.array_equal(ref["status"], np.where(need > cap, 99, 0)) and np.array_equal(ref["stats"][:, 0], np.minimum(need, cap))
            if cap == 1:
                assert (ref["status"] == 99).all()
            elif nb == 1:
                assert ref["status"][0] == (99 if cap == k else 0)
            else:
                waves = [ref["status"][:64], ref["status"][64:128]] if group == 1 and nb >= 128 else [ref["status"][:64] if group == 1 else ref["status"]]
                for w in waves:
                    assert (w == 0).any() and (w == 99).any()
                if name.endswith("with_root"):
                    assert (ref["root_idx"][ref["status"] == 0] == 0).any() and (ref["root_idx"][ref["status"] == 99] == -1).all()
            assert_exits_same(dev, ref, key, steps=entry.startswith("steps"))


def test_e_the_python_surface_takes_max_steps_and_reports_the_members_that_stopped(H):
    """Solver(options=dict(max_steps=k)) reaches the launch: solve_dense_adaptive returns the arrays of the C entry for a mixed ensemble, failed_members counts
    the members with a status"""
    nb = 130
    p = decay_params("exponential_decay", nb, 1)
    free = E.solve_ensemble(ORACLE_MODEL["exponential_decay"], p, DECAY_T, **DECAY_TOL)
    k = mixing_cap(free["stats"][:, 0], nb, 1)
    dev, ref, _ = compare(H, "plain", "exponential_decay", p, DECAY_T, 1, options=dict(max_steps=k), **DECAY_TOL)
    assert (ref["status"][:64] == 0).any() and (ref["status"][:64] == 99).any()
    s = H.Solver("exponential_decay", p, nbatch=nb, method=H.METHOD_TSIT45, options=dict(max_steps=k), **DECAY_TOL)
    y, tot, mem = s.solve_dense_adaptive(DECAY_T, want_member_stats=True, group=1)
    assert np.array_equal(np.transpose(y, (1, 0, 2)), dev["y"], equal_nan=True) and np.array_equal(mem["stats"].T, dev["stats"])
    assert np.array_equal(mem["status"], dev["status"]) and np.array_equal(mem["ncols"], dev["ncols"])
    assert tot["failed_members"] == int((mem["status"] != 0).sum()) == ref["failed"] and tot["number_of_steps"] == int(dev["stats"][:, 0].sum())
    with pytest.raises(H.DiffsolHipError):   # a name the options do not have is refused, not dropped
        H.Solver("exponential_decay", p, nbatch=nb, method=H.METHOD_TSIT45, options=dict(max_step=k), **DECAY_TOL)


# ------------------------------------------------------------------------------------------------------------------ f. rejections and their exits
# dy/dt = a y^2 from (1, 2, 0.5): y = 1 / (1/y0 - a t), the second state leaves every bound at t = 1 / (2 a).  Half of the members are gentle (a <= 0.1: no rejected
# step, they finish), half meet the blow-up between the save points (a >= 0.45: t = 1.11 .. 0.33).  At these tolerances a step towards the blow-up is rejected up to
# three times in a row and no more (measured with the checker, asserted below): max_error_test_failures = 3 ends such a member with status 2, the default 40 lets the
# step size fall below min_timestep (status 1).
BLOW_T = [0.1, 0.2, 0.3, 0.5, 0.8, 1.2]
BLOW_TOL = dict(rtol=0.1, atol=[1e-2] * 3)
BLOW_CASES = {
    "default": (dict(), 1),
    "max_error_test_failures_1": (dict(max_error_test_failures=1), 2),
    "max_error_test_failures_3": (dict(max_error_test_failures=3), 2),
    "min_timestep_raised": (dict(min_timestep=1e-2), 1),
    "both_limits_at_the_first_rejection": (dict(max_error_test_failures=1, min_timestep=1e30), 2),
    "both_limits_raised": (dict(max_error_test_failures=3, min_timestep=1e-2), None),
    "other_controller_constants": (dict(PI_PAIR), 1),
}


def blow_params(nb):
    rng = np.random.default_rng(11)
    return np.where(rng.uniform(size=nb) < 0.5, rng.uniform(0.01, 0.1, nb), rng.uniform(0.45, 1.5, nb))[:, None]


@pytest.mark.parametrize("group", [1, 64])
@pytest.mark.parametrize("nb", [65, 130])
@pytest.mark.parametrize("case", list(BLOW_CASES))
def test_f_rejected_steps_and_the_exits_behind_them(H, case, nb, group):
    """the rejection branch of the step loop (explicit_rk.rs:227-239) and error_test_fail's two exits in their order (runge_kutta.rs:852 before :861), with members of
    one wavefront that finish beside members that fail; columns drained before the exit hold the checker's bits, the others NaN.
    (*) At these loose tolerances a few gentle members end their last step one rounding below t_eval[-1]: handle_tstop (runge_kutta.rs:752-781) calls that reached,
    `t_eval[col] <= t` does not, and the member reports status 0 with its last column NaN — on the device and in the checker alike.  The reference asserts at this
    point (method.rs:771, "this should not happen"); neither side restates the assertion, and this test holds them to each other there, not to a rule."""
    opts, status = BLOW_CASES[case]
    opts = dict(opts, max_steps=100000)
    p = blow_params(nb)
    for entry in ENTRIES:
        # with the sensitivities in the error test no step of these members is rejected three times in a row: the two cases with a limit of 3 leave them out of it
        kw = dict(BLOW_TOL, sens_atol=None if "3" in case or "raised" in case else (1e-6,))
        dev, ref, key = solve_pair(H, entry, "dydt_y2", p, BLOW_T, group, options=opts, **kw)
        default = ref if case == "default" else solve_pair(H, entry, "dydt_y2", p, BLOW_T, group, options=dict(max_steps=100000), reference=True, **kw)[1]
        failing = ref["status"] != 0
        assert ref["stats"][failing, 3].min() > 0 and (ref["status"] != 99).all()            # every failing member went through the rejection branch
        assert failing.any() and set(ref["status"][failing].tolist()) <= {1, 2}
        if status is not None:   # the exit the case is about is the one every failing member takes
            assert (ref["status"][failing] == status).all()
        if case != "default":
            assert not np.array_equal(ref["stats"], default["stats"])                         # the option bites
        if case == "max_error_test_failures_1":
            assert (ref["stats"][failing, 3] == 1).all()
        if case == "max_error_test_failures_3":                                                 # three in one step, with earlier single ones before
            assert (ref["stats"][ref["status"] == 2, 3] >= 3).all() and (default["status"][failing] == 1).all()
        if case == "both_limits_at_the_first_rejection":
            assert (ref["stats"][failing, 3] == 1).all()
        if group == 1:   # members of the first wavefront end differently
            assert (ref["status"][:64] == 0).any() and failing[:64].any()
            if not entry.startswith("steps"):
                cols = np.isfinite(ref[key][:, :, 0]).sum(axis=1)
                assert (cols[failing] < len(BLOW_T)).all() and ((cols[failing] > 0).any() or "1" in case or "first" in case) and (cols[~failing] >= len(BLOW_T) - 1).all()   # (*)
        assert_exits_same(dev, ref, key, steps=entry.startswith("steps"))


# ------------------------------------------------------------------------------------------------------------------ g. stop-time exits
@pytest.mark.parametrize("group", [1, 64])
@pytest.mark.parametrize("nb", [1, 130])
@pytest.mark.parametrize("t0", [0.0, 1.5])
def test_g_stop_time_exits_before_the_first_step(H, t0, nb, group):
    """set_stop_time (runge_kutta.rs:436-444): the last save point at t0 is StopTimeAtCurrentTime (6), a negative h0 with the save points ahead
    StopTimeBeforeCurrentTime (5).  Nothing is integrated; in steps mode column 0 (t0, y0 — g = 0 with integrated outputs) is written all the same"""
    p = decay_params("exponential_decay", nb, group)
    for entry in ENTRIES:
        for t_eval, h0, status in (([t0], 1.0, 6), ([t0 + 1.0, t0 + 2.0], -1.0, 5)):
            dev, ref, key = solve_pair(H, entry, "exponential_decay", p, t_eval, group, t0=t0, h0=h0, **DECAY_TOL)
            assert (ref["status"] == status).all() and not ref["stats"].any() and ref["failed"] == nb
            if entry.startswith("steps"):
                assert (ref["ncols"] == 1).all() and (ref["t"][:, 0] == t0).all() and np.isfinite(ref[key][:, 0]).all() and np.isnan(ref[key][:, 1:]).all()
            else:
                assert np.isnan(ref[key]).all() and ("ncols" not in ref or not ref["ncols"].any())
            assert_exits_same(dev, ref, key, steps=entry.startswith("steps"))


# ------------------------------------------------------------------------------------------------------------------ h. root disagreement
@pytest.mark.parametrize("entry", ["plain", "steps", "out", "steps_out"])
def test_h_members_of_a_lock_step_group_that_disagree_on_the_crossing(H, entry):
    """group 64 with per-member parameters: the first wavefront shares one parameter set and stops at its root, the others disagree on the step of the crossing and
    stop with RootBatchMismatch (20) where the checker's batched root finder does"""
    nb = 130
    p = P.params("exponential_decay_with_root", nb)
    p[:64] = p[0]
    dev, ref, key = solve_pair(H, entry, "exponential_decay_with_root", p, DECAY_T, 64, **DECAY_TOL)
    assert (ref["status"][:64] == 0).all() and (ref["root_idx"][:64] == 0).all() and (ref["status"][64:] == 20).all() and ref["failed"] == nb - 64
    assert ref["stats"][64:, 0].min() > 1   # the disagreement comes after steps that agreed
    assert_exits_same(dev, ref, key, steps=entry.startswith("steps"))


# ------------------------------------------------------------------------------------------------------------------ i. non-finite members
@pytest.mark.parametrize("group", [1, 64])
@pytest.mark.parametrize("lane", [0, 37, 129])
@pytest.mark.parametrize("bad", [np.nan, np.inf], ids=["nan", "inf"])
def test_i_a_member_with_a_non_finite_parameter(H, bad, lane, group):
    """one decay rate NaN or infinite, in lane 0, in a middle lane and in the short last wavefront, under max_steps = 50 (never the default cap: a member whose step
    size is NaN accepts every step and never reaches the stop time).  Per member the bad member ends as the checker's does and nobody else notices; in lock-step its
    whole group ends as the checker's group does"""
    nb = 130
    opts = dict(max_steps=50)
    p = decay_params("exponential_decay", nb, group)
    clean = p.copy()
    p[lane, 0] = bad
    others = np.arange(nb) != lane
    for entry in ENTRIES:
        dev, ref, key = solve_pair(H, entry, "exponential_decay", p, DECAY_T, group, options=opts, **DECAY_TOL)
        assert ref["status"][lane] != 0 and ref["failed"] == (1 if group == 1 else min(64, nb - 64 * (lane // 64)))
        assert_exits_same(dev, ref, key, steps=entry.startswith("steps"))
        if group == 1:
            sound = solve_pair(H, entry, "exponential_decay", clean, DECAY_T, group, options=opts, reference=False, **DECAY_TOL)[0]
            assert not sound["status"].any()
            for k in ("status", "stats", "ncols", "root_idx", "t_root", key, "t"):
                if k in dev and (k != "t" or entry.startswith("steps")):
                    assert np.array_equal(dev[k][others], sound[k][others], equal_nan=True), k
            if "sens" in dev:
                assert np.array_equal(dev["sens"][:, others], sound["sens"][:, others])
