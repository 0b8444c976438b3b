"""first_step / step_t / min_step / max_step of the dopri5 solves, the parts that need no GPU: the step-wise solver against
the oracle's restatement of torchdiffeq (oracle/odeint.py: _Dopri5.integrate), the C boundary of the fused kernels' form of
them (cde_dopri5_step_options and the *_options entry points) and the option normalisation of cdeint."""
import ctypes
import os
import re
import sys

import pytest
import torch

import torchcde_amd
from torchcde_amd import _lib, stepwise
from oracle import odeint as oracle_ode

cdeint_module = sys.modules["torchcde_amd.cdeint"]        # (the package attribute of that name is the function)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL, ATOL = 1e-5, 1e-7
T = torch.tensor([0.0, 1.3, 3.0], dtype=torch.float64)
KNOTS = [0.5, 1.0, 1.5, 2.0, 2.5]


def _matrix():
    gen = torch.Generator().manual_seed(3)
    return 0.8 * torch.randn(6, 6, generator=gen, dtype=torch.float64)


def field(t, y):
    """A plain tensor field with a kink in t at every entry of KNOTS (as a piecewise-linear control gives a CDE) and a fast
    burst around t = 2.2 that makes the controller reject."""
    ramp = sum(torch.clamp(t - k, min=0.0) * ((-1.0) ** i) for i, k in enumerate(KNOTS))
    burst = 40.0 * torch.exp(-((t - 2.2) / 0.05) ** 2)
    return torch.tanh(y @ _matrix().to(y.dtype)) * (1.0 + 2.0 * ramp) + burst * torch.cos(3.0 * y)


def _y0():
    return torch.linspace(-1.0, 1.0, 4 * 6, dtype=torch.float64).reshape(4, 6)


CASES = {
    "none": {},
    "first_step": dict(first_step=0.2),
    "max_step": dict(max_step=0.11),
    "min_step": dict(min_step=0.04),
    "step_t": dict(step_t=[0.3, 1.3, 2.2, 2.9, 5.0]),
    "all": dict(first_step=0.01, min_step=0.02, max_step=0.25, step_t=[-1.0, 0.3, 0.75, 2.2, 2.9, 5.0], jump_t=KNOTS),
}


def _both(options, t=T, reverse=False):
    """(oracle solver after integrate, its output, step-wise attempts, its output) for one option set."""
    y0 = _y0()
    oracle = oracle_ode._Dopri5(oracle_ode._Field(field, None, reverse), y0, RTOL, ATOL, oracle_ode._rms, **options)
    want = oracle.integrate(t)
    attempts = []
    got = stepwise._solve_dopri5(stepwise._Wrapped(field, None, reverse), y0, t, RTOL, ATOL, stepwise._rms, record=attempts,
                                 **options)
    return oracle, want, attempts, got


@pytest.mark.parametrize("name", sorted(CASES))
def test_stepwise_dopri5_takes_the_oracles_steps(name):
    options = CASES[name]
    oracle, want, attempts, got = _both(options)
    accepted = [(t0, t1, j) for t0, t1, j, ok in attempts if ok]
    assert accepted == oracle.accepted
    assert len(attempts) - len(accepted) == oracle.n_reject
    assert (got - want).abs().max().item() <= 1e-12
    # the case proves its rule only if the rule fires
    lengths = [t1 - t0 for t0, t1, _ in accepted]
    if "first_step" in options:
        lo, hi = options.get("min_step", 0.0), options.get("max_step", float("inf"))
        assert attempts[0][1] - attempts[0][0] == min(max(options["first_step"], lo), hi)
    if "max_step" in options:
        # (t1 - t0 of an attempt planned at max_step: within a rounding of it)
        assert max(lengths) <= options["max_step"] + 1e-12
        assert sum(abs(length - options["max_step"]) <= 1e-12 for length in lengths) >= (1 if "step_t" in options else 3)
    if "min_step" in options:
        assert any(length <= options["min_step"] for length in lengths)
        assert oracle.n_reject > 0
    if "step_t" in options:
        ends = {t1 for _, t1, j in accepted if j == 0.0}
        inside = [s for s in options["step_t"] if T[0] < s < T[-1]]
        assert inside and all(s in ends for s in inside)
    if "jump_t" in options:
        assert {t1 for _, t1, j in accepted if j == 1.0} == set(KNOTS)


def test_a_forced_accept_overrides_the_error_ratio():
    """min_step above what the burst needs: the oracle accepts attempts whose error ratio is above 1, and so must we."""
    options = dict(min_step=0.08, max_step=0.3)
    oracle, want, attempts, got = _both(options)
    assert [(t0, t1, j) for t0, t1, j, ok in attempts if ok] == oracle.accepted
    free = oracle_ode._Dopri5(oracle_ode._Field(field, None, False), _y0(), RTOL, ATOL, oracle_ode._rms)
    free.integrate(T)
    assert min(t1 - t0 for t0, t1, _ in free.accepted) < 0.08          # unforced, the solve needs shorter steps here
    assert (got - want).abs().max().item() <= 1e-12


def test_stepwise_dopri5_in_reversed_time():
    """Decreasing t: step_t is negated and flipped next to jump_t, by the front end (odeint) and by hand alike."""
    t = T.flip(0)
    options = dict(step_t=torch.tensor([0.3, 0.75, 2.2], dtype=torch.float64), jump_t=torch.tensor(KNOTS, dtype=torch.float64),
                   max_step=0.3)
    mirrored = dict(options, step_t=(-options["step_t"]).flip(0), jump_t=(-options["jump_t"]).flip(0))
    oracle, want, attempts, got = _both(mirrored, t=-t, reverse=True)
    assert [(t0, t1, j) for t0, t1, j, ok in attempts if ok] == oracle.accepted
    assert {-0.3, -0.75, -2.2} <= {t1 for _, t1, j in oracle.accepted if j == 0.0}
    assert (got - want).abs().max().item() <= 1e-12
    front = stepwise.odeint(field, _y0(), t, method="dopri5", options=dict(options), rtol=RTOL, atol=ATOL)
    front_oracle = oracle_ode.odeint(field, _y0(), t, rtol=RTOL, atol=ATOL, method="dopri5", options=dict(options))
    assert (front - front_oracle).abs().max().item() <= 1e-12
    assert torch.equal(front, got)


def test_a_time_shared_by_step_t_and_jump_t_is_refused():
    message = "`step_t` and `jump_t` must not have any repeated elements between them."
    for solve in (lambda o: stepwise.odeint(field, _y0(), T, method="dopri5", options=o, rtol=RTOL, atol=ATOL),
                  lambda o: oracle_ode.odeint(field, _y0(), T, rtol=RTOL, atol=ATOL, method="dopri5", options=o)):
        with pytest.raises(ValueError) as err:
            solve(dict(step_t=[0.3, 1.5], jump_t=KNOTS))
        assert str(err.value) == message
        solve(dict(step_t=[-1.5, 0.3], jump_t=[-1.5, 1.0]))                # a shared time before t[0] is dropped first


# ------------------------------------------------------------------ the boundary
TWINS = {
    "cde_dopri5_advance_options": "cde_dopri5_advance",
    "cde_dopri5_advance_mlp_options": "cde_dopri5_advance_mlp",
    "cde_dopri5_adjoint_advance_options": "cde_dopri5_adjoint_advance",
    "cde_dopri5_adjoint_advance_dcontrol_options": "cde_dopri5_adjoint_advance_dcontrol",
    "cde_dopri5_adjoint_mlp_advance_options": "cde_dopri5_adjoint_mlp_advance",
    "cde_dopri5_adjoint_mlp_advance_dcontrol_options": "cde_dopri5_adjoint_mlp_advance_dcontrol",
}


def test_step_option_symbols_are_declared_exported_and_bound():
    lib = torchcde_amd.load()
    header = open(os.path.join(ROOT, "include", "cde_mi355x.h")).read()
    raw = ctypes.CDLL(_lib.SO_PATH)
    for name in list(TWINS) + ["cde_dopri5_step_state_bytes"]:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(raw, name) and hasattr(lib, name)
    assert lib.cde_abi_version() == 3
    assert header.index("} cde_dopri5_status;") < header.index("} cde_dopri5_step_options;")
    # the struct's mirror: same fields in the same order with the same widths
    body = re.search(r"typedef struct \{([^}]*)\} cde_dopri5_step_options;", header).group(1)
    fields = []
    for ctype, names in re.findall(r"(double|int64_t|const double\*|void\*)\s+([^;]+);", body):
        fields += [(n.strip(), ctype) for n in names.split(",")]
    widths = {"double": ctypes.c_double, "int64_t": ctypes.c_int64, "const double*": ctypes.c_void_p, "void*": ctypes.c_void_p}
    assert [(n, widths[c]) for n, c in fields] == list(_lib.StepOptions._fields_)
    assert lib.cde_dopri5_step_state_bytes() == 80          # six 8-byte option words, two 16-byte states
    # a twin is its entry point with one more pointer ahead of the stream (the affine backward: without the sharded pair)
    for twin, plain in TWINS.items():
        args = list(_lib._SIGNATURES[plain][1])
        if plain == "cde_dopri5_adjoint_advance":
            args = args[:-3] + args[-1:]
        assert _lib._SIGNATURES[twin] == (ctypes.c_int, args[:-1] + [ctypes.c_void_p, ctypes.c_void_p]), twin


def _twin_args(twin, block):
    """A call every other check of `twin` would let through as far as the workspace size (rejected_calls.py's arguments for
    the entry point it extends), with `block` as its options."""
    from rejected_calls import CALLS, build_args
    plain = TWINS[twin]
    args = list(build_args(CALLS[plain]))
    if plain == "cde_dopri5_adjoint_advance":
        args = args[:-3] + args[-1:]
    return args[:-1] + [None if block is None else ctypes.addressof(block), args[-1]]


@pytest.mark.parametrize("twin", sorted(TWINS))
def test_invalid_step_options_come_back_as_codes_without_a_gpu(twin):
    lib = torchcde_amd.load()
    nan, inf = float("nan"), float("inf")
    state, times = 0x1000, 0x2000          # never dereferenced: every call here is turned away on the host
    invalid = [
        (_lib.StepOptions(nan, -0.1, inf, None, 0, state), -3),            # min_step < 0
        (_lib.StepOptions(nan, nan, inf, None, 0, state), -3),
        (_lib.StepOptions(nan, 0.5, 0.25, None, 0, state), -3),            # max_step < min_step
        (_lib.StepOptions(nan, 0.0, nan, None, 0, state), -3),
        (_lib.StepOptions(nan, 0.0, inf, times, -1, state), -3),           # n_step < 0
        (_lib.StepOptions(nan, 0.0, inf, None, 2, state), -1),             # step times announced, none given
        (_lib.StepOptions(nan, 0.0, inf, times, 2, None), -1),             # nowhere to keep the controller's state
    ]
    for block, code in invalid:
        assert getattr(lib, twin)(*_twin_args(twin, block)) == code, (block.min_step, block.max_step, block.n_step)


def test_twins_answer_like_their_entry_points_without_options():
    """`options` == NULL is the entry point itself: every rejected call of the table comes back with the same code."""
    from rejected_calls import CALLS, REJECTED, build_args
    lib = torchcde_amd.load()
    for twin, plain in TWINS.items():
        for code, cases in REJECTED[plain].items():
            for overrides in cases:
                args = list(build_args(CALLS[plain], overrides))
                if plain == "cde_dopri5_adjoint_advance":
                    if "reduced_sums" in overrides or "B_global" in overrides:
                        continue
                    args = args[:-3] + args[-1:]
                assert getattr(lib, twin)(*(args[:-1] + [None, args[-1]])) == code, (twin, overrides)


def test_existing_boundary_is_unchanged():
    import test_host
    test_host.test_library_builds_loads_and_exports_every_declared_symbol()
    test_host.test_ctypes_signatures_match_the_header_prototypes()
    test_host.test_status_struct_mirror_matches_the_header()
    test_host.test_argument_errors_come_back_as_codes_without_a_gpu()
    test_host.test_adaptive_workspace_layouts_keep_their_recorded_sizes_and_offsets()


# ------------------------------------------------------------------ option normalisation
def test_step_options_are_fused_requests_and_none_is_absent():
    strip = cdeint_module._strip_noops
    assert strip(dict(first_step=None, step_t=None, min_step=None, max_step=None, jump_t=None), fixed=False) == {}
    kept = strip(dict(first_step=0.1, step_t=[1.0], min_step=0.0, max_step=None), fixed=False)
    assert set(kept) == {"first_step", "step_t", "min_step"}
    assert set(cdeint_module._STEP_KEYS) == {"first_step", "step_t", "min_step", "max_step"}
    source = open(os.path.join(ROOT, "torchcde_amd", "cdeint.py")).read()
    assert re.search(r"adaptive_keys = \{\"step_size\"\}, \{[^}]*\*_STEP_KEYS\}", source)


def test_step_option_values_are_parsed_like_torchdiffeqs():
    parse = lambda o, jump=None: cdeint_module._StepOptions(dict(o), jump, torch.device("cpu"), lambda times: times >= 0.0)   # noqa: E731
    none = parse(dict(first_step=None, max_step=None))
    assert not none.given and none.first_step != none.first_step and (none.min_step, none.max_step) == (0.0, float("inf"))
    some = parse(dict(first_step=torch.tensor(0.25), min_step=0.125, max_step=torch.tensor(2.0, dtype=torch.float64),
                      step_t=(3.0, 1.0, 2.0)))
    assert some.given and (some.first_step, some.min_step, some.max_step, some.n_step) == (0.25, 0.125, 2.0, 3)
    assert some.step_t.tolist() == [1.0, 2.0, 3.0] and some.step_s.tolist() == [-3.0, -2.0, -1.0]
    assert parse(dict(step_t=torch.tensor([0.5, 1.5])), jump=[-0.5, 1.0]).n_step == 2
    with pytest.raises(ValueError, match="must not have any repeated elements between them"):
        parse(dict(step_t=[0.5, 1.0]), jump=torch.tensor([1.0, 2.0]))
    parse(dict(step_t=[-1.0, 0.5]), jump=[-1.0, 2.0])                      # shared, but before the solve starts: dropped
    with pytest.raises(ValueError):
        parse(dict(min_step=0.5, max_step=0.25))
