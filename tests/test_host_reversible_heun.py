"""backend="torchsde", method="reversible_heun" without a GPU: the C ABI's argument checks, the step-wise solve and its
reconstructing backward pass against autograd through the restated recurrences (tests/revheun_reference.py), and the
keyword handling of the front end."""
import pytest
import torch

import torchcde_amd
from torchcde_amd import _lib
from torchcde_amd import dispatch as D
from torchcde_amd.fields import probe
from helpers import LinearField, TwoLayerField, make_series
from rejected_calls import build_args
import revheun_reference as ref


# ------------------------------------------------------------------------------------------------ the C ABI
CALLS_RH = {
    "cde_revheun_supported": "C=8 H=32 dtype=0 act=1",
    "cde_revheun_forward_linear": "coeffs knots n_intervals=4 degree=3 W bias act=1 z0 grid n_grid=5 t_out n_out=2 z_out zhat_out "
                                  "B=64 C=8 H=32 dtype=0 time_dtype=0 node_index node_frac stream=0",
    "cde_revheun_adjoint_workspace_bytes": "B=64 n_grid=5",
    "cde_revheun_adjoint_linear": "coeffs knots n_intervals=4 degree=3 W bias act=1 y_final zhat_final grad_out grid n_grid=5 "
                                  "node_ptr node_out node_weight n_out=2 grad_z0 grad_W grad_b B=64 C=8 H=32 dtype=0 time_dtype=0 "
                                  "workspace workspace_bytes=1073741824 stream=0",
}
# entry point -> {code: overrides of the valid call above that must return it}: the ORDER of the checks -- sizes (-3), unknown
# dtype (-2), the forward solve's empty batch (0), the envelope (-4), pointers (-1), the workspace one byte short (-5; the
# size is asked of the library below)
REJECTED_RH = {
    "cde_revheun_forward_linear": {
        -3: ["C=0", "H=0", "n_intervals=0", "B=-1", "n_out=0", "n_grid=0", "C=0 dtype=7", "H=0 coeffs=0"],
        -2: ["dtype=7", "time_dtype=7", "dtype=7 H=33", "dtype=7 B=0"],
        0: ["B=0", "B=0 H=33", "B=0 coeffs=0", "B=0 dtype=1"],
        -4: ["dtype=1", "H=33", "C=9", "act=2", "act=-1", "act=16", "degree=2", "H=33 coeffs=0", "dtype=1 W=0"],
        -1: ["coeffs=0", "knots=0", "W=0", "bias=0", "z0=0", "grid=0", "t_out=0", "z_out=0", "zhat_out=0", "node_index=0",
             "node_frac=0"],
    },
    "cde_revheun_adjoint_linear": {
        -3: ["C=0", "H=0", "n_intervals=0", "B=0", "B=-1", "n_out=0", "n_grid=0", "B=0 dtype=7", "H=0 coeffs=0"],
        -2: ["dtype=7", "time_dtype=7", "dtype=7 H=33"],
        -4: ["dtype=1", "H=33", "C=9", "act=2", "act=-1", "act=16", "degree=2", "H=33 coeffs=0", "dtype=1 workspace=0"],
        -1: ["coeffs=0", "knots=0", "W=0", "bias=0", "y_final=0", "zhat_final=0", "grad_out=0", "grid=0", "node_ptr=0",
             "node_out=0", "node_weight=0", "grad_z0=0", "grad_W=0", "grad_b=0", "workspace=0", "workspace=0 workspace_bytes=0"],
        -5: ["workspace_bytes=SHORT", "workspace_bytes=0"],
    },
}


def test_reversible_heun_entry_points_reject_bad_calls_without_a_gpu():
    """Dummy pointers, no device: every row fails a check that comes before the first HIP call (tests/rejected_calls.py)."""
    lib = torchcde_amd.load()
    need = lib.cde_revheun_adjoint_workspace_bytes(64, 5)
    # [node index: 5 int64][node frac: 5 f32], each rounded up to 256 bytes, then one (32, 8, 32) + (32, 8) partial per 32 series
    assert need == 256 + 256 + 2 * 4 * (32 * 8 * 32 + 32 * 8) and need % 256 == 0
    assert lib.cde_revheun_adjoint_workspace_bytes(0, 5) == 512
    assert lib.cde_revheun_adjoint_workspace_bytes(1, 1) == lib.cde_revheun_adjoint_workspace_bytes(32, 32) == 512 + 4 * (32 * 8 * 32 + 32 * 8)
    assert set(REJECTED_RH) | {"cde_revheun_supported", "cde_revheun_adjoint_workspace_bytes"} == set(CALLS_RH) <= set(_lib.EXPORTED_SYMBOLS)
    wrong = []
    for name, by_code in REJECTED_RH.items():
        call = getattr(lib, name)
        assert call(*build_args(CALLS_RH[name], "coeffs=0")) == -1                  # valid but for one pointer
        for code, cases in by_code.items():
            for overrides in cases:
                got = call(*build_args(CALLS_RH[name], overrides.replace("SHORT", str(need - 1))))
                if got != code:
                    wrong.append("%s(%s): %d, expected %d" % (name, overrides, got, code))
    assert not wrong, "\n".join(wrong)
    assert lib.cde_abi_version() == 3 == _lib.ABI_VERSION                          # the change is additive


def test_reversible_heun_envelope():
    lib = torchcde_amd.load()
    for C, H, dtype, act, ok in [(8, 32, 0, 0, 1), (8, 32, 0, 1, 1), (1, 1, 0, 1, 1), (3, 6, 0, 0, 1), (9, 32, 0, 0, 0),
                                 (8, 33, 0, 0, 0), (8, 32, 1, 0, 0), (8, 32, 0, 2, 0), (0, 32, 0, 0, 0), (8, 0, 0, 0, 0)]:
        assert lib.cde_revheun_supported(C, H, dtype, act) == ok, (C, H, dtype, act)
    assert D.TORCHSDE_PATHS == ("reversible_heun", "reversible_heun_stepwise")
    assert not set(D.TORCHSDE_PATHS) & (set(D.FUSED_PATHS) | {D.STEPWISE})


# ------------------------------------------------------------------------------------------------ the step-wise solve
class CpuContract:                                        # cde_contract needs the GPU; the formula is all that matters here
    @staticmethod
    def apply(F, dX):
        return (F * dX.unsqueeze(-2)).sum(-1)


class Path:
    """A smooth control with a batch of slopes: dX/dt(t) = slope * (1 + t)."""

    def __init__(self, slope):
        self.slope = slope

    def derivative(self, t):
        return self.slope * (1 + t)


class Sigmoid(torch.nn.Module):
    """An unrecognised module with a parameter of its own (the form of the reference's test/test_tricks.py field)."""

    def __init__(self, H, C):
        super().__init__()
        self.H, self.C = H, C
        self.offset = torch.nn.Parameter(torch.rand(C, generator=torch.Generator().manual_seed(5), dtype=torch.float64))

    def forward(self, t, z):
        return z.sigmoid().unsqueeze(-1) * (1 + 0.1 * t) + self.offset


def _reconstructs(out):
    """Is the reconstructing backward pass (stepwise._ReversibleHeun) the autograd node behind `out`?"""
    todo, seen = [out.grad_fn], set()
    while todo:
        node = todo.pop()
        if node is None or node in seen:
            continue
        seen.add(node)
        if "ReversibleHeun" in type(node).__name__:
            return True
        todo += [n for n, _ in node.next_functions]
    return False


def _fields(H, C):
    return {"unrecognised": Sigmoid(H, C),
            "affine": LinearField(H, C, torch.float64, scale=0.5, seed=3),
            "affine_tanh": LinearField(H, C, torch.float64, scale=0.5, tanh=True, seed=4),
            "two_layer": TwoLayerField(H, C, 9, torch.float64, seed=6)}


@pytest.mark.parametrize("lead", [(7,), (2, 4)])
@pytest.mark.parametrize("kind", ["unrecognised", "affine", "affine_tanh", "two_layer"])
@pytest.mark.parametrize("t,dt", [([0.0, 2.0], 0.5), ([0.0, 0.6, 1.0, 1.7], 0.5), ([0.3], 0.5)])
def test_stepwise_reversible_heun_equals_autograd_through_the_recurrences(monkeypatch, kind, lead, t, dt):
    """stepwise.solve_reversible_heun in float64 on the CPU: the solution equals the restated recurrences, and the gradients
    its reconstructing backward pass returns for z0 and the parameters equal autograd through them (rtol 1e-11) -- closed-form
    node evaluations for the recognised fields, autograd per node for the module nobody recognises; one and two batch
    dimensions; output times on grid points, between them, and a clipped last step."""
    from torchcde_amd import stepwise
    monkeypatch.setattr(stepwise, "_Contract", CpuContract)
    H, C = 5, 3
    gen = torch.Generator().manual_seed(11)
    func = _fields(H, C)[kind]
    X = Path(torch.randn(*lead, C, generator=gen, dtype=torch.float64))
    z0 = torch.randn(*lead, H, generator=gen, dtype=torch.float64)
    times = torch.tensor(t, dtype=torch.float64)
    lw = torch.rand(*lead, len(t), H, generator=gen, dtype=torch.float64) + 0.5
    params = tuple(func.parameters())

    zr = z0.clone().requires_grad_(True)
    want = ref.solve(X, func, zr, times, dt)
    want_grads = torch.autograd.grad((want * lw).sum(), (zr,) + params, allow_unused=True)

    recognised, _ = probe(func, times[0], z0)
    assert (recognised is None) == (kind == "unrecognised")
    zs = z0.clone().requires_grad_(True)
    got = stepwise.solve_reversible_heun(X, func, zs, times, dt, True, None, recognised=recognised)
    assert got.shape == want.shape == (*lead, len(t), H)
    assert torch.allclose(got, want.detach(), rtol=1e-13, atol=1e-14)
    assert _reconstructs(got)
    got_grads = torch.autograd.grad((got * lw).sum(), (zs,) + params, allow_unused=True)
    def same(g, w):
        if w is None:                                     # (a single output time: no step, no parameter is reached)
            return g is None or not g.any()
        return torch.allclose(g, w, rtol=1e-11, atol=1e-11 * w.abs().max().item())
    assert all(same(g, w) for g, w in zip(got_grads, want_grads))

    # adjoint=False asks for the same gradient and takes the same sweep; `through`: plain autograd through the steps
    zf = z0.clone().requires_grad_(True)
    again = stepwise.solve_reversible_heun(X, func, zf, times, dt, False, None, recognised=recognised)
    assert torch.equal(again, got)
    for g, w in zip(torch.autograd.grad((again * lw).sum(), (zf,) + params, allow_unused=True), got_grads):
        assert (g is None and w is None) or torch.equal(g, w)
    zt = z0.clone().requires_grad_(True)
    plain = stepwise.solve_reversible_heun(X, func, zt, times, dt, False, None, recognised=recognised, through=True)
    assert torch.equal(plain, got) and not _reconstructs(plain)
    assert all(same(g, w) for g, w in zip(torch.autograd.grad((plain * lw).sum(), (zt,) + params, allow_unused=True), want_grads))


def test_stepwise_reversible_heun_honours_adjoint_params(monkeypatch):
    """A subset of the parameters in adjoint_params: those get their gradient, the others none."""
    from torchcde_amd import stepwise
    monkeypatch.setattr(stepwise, "_Contract", CpuContract)
    H, C = 5, 3
    gen = torch.Generator().manual_seed(2)
    func = LinearField(H, C, torch.float64, scale=0.5, tanh=True, seed=4)
    X = Path(torch.randn(6, C, generator=gen, dtype=torch.float64))
    z0 = torch.randn(6, H, generator=gen, dtype=torch.float64)
    times = torch.tensor([0.0, 1.3], dtype=torch.float64)
    want = ref.solve(X, func, z0, times, 0.4)
    want_b, = torch.autograd.grad(want.sum(), (func.linear.bias,))
    got = stepwise.solve_reversible_heun(X, func, z0, times, 0.4, True, (func.linear.bias,))
    got.sum().backward()
    assert func.linear.weight.grad is None
    assert torch.allclose(func.linear.bias.grad, want_b, rtol=1e-11, atol=1e-11 * want_b.abs().max().item())


# ------------------------------------------------------------------------------------------------ keywords (CPU tensors)
def _cpu_call(**kw):
    x = make_series(2, 5, 3)
    X = torchcde_amd.LinearInterpolation(x)
    func = LinearField(4, 3)
    return torchcde_amd.cdeint(X, func, torch.zeros(2, 4), X.interval, **kw)


@pytest.mark.parametrize("kw,named", [
    (dict(method="srk"), "srk"), (dict(method="euler"), "euler"), (dict(), "None"),
    (dict(method="reversible_heun", adaptive=True), "adaptive"),
    (dict(method="reversible_heun", adjoint_adaptive=True), "adjoint_adaptive"),
    (dict(method="reversible_heun", bm=object()), "bm"), (dict(method="midpoint", bm=object()), "bm"),
    (dict(method="reversible_heun", names={"drift": "f"}), "names"), (dict(method="reversible_heun", logqp=True), "logqp"),
    (dict(method="reversible_heun", dt_min=1e-5), "dt_min"), (dict(method="reversible_heun", extra_solver_state=()), "extra_solver_state"),
    (dict(method="reversible_heun", adjoint_method="midpoint"), "adjoint_method"),
    (dict(method="midpoint", adjoint_method="adjoint_reversible_heun"), "adjoint_method"),
    (dict(method="reversible_heun", options={"step_size": 1.0}), "options"),
])
def test_torchsde_keywords_outside_the_solver_are_named(kw, named):
    with pytest.raises(NotImplementedError, match=named):
        _cpu_call(backend="torchsde", **kw)
    with pytest.raises(NotImplementedError, match=named):       # the tuple front end parses the same keywords
        x = make_series(2, 5, 3)
        X = torchcde_amd.LinearInterpolation(x)
        torchcde_amd.cdeint(X, LinearField(4, 3), (torch.zeros(2, 4),), X.interval, backend="torchsde", **kw)


def test_torchsde_calls_reach_the_device_check_and_other_backends_the_value_error():
    """The accepted spellings pass the keyword checks and stop, on CPU tensors, where every call of this package stops; the
    midpoint spelling stops exactly where its torchdiffeq spelling does."""
    with pytest.raises(RuntimeError, match="no CPU fallback") as sde:
        _cpu_call(backend="torchsde", method="midpoint", dt=1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback") as ode:
        _cpu_call(backend="torchdiffeq", method="midpoint", options={"step_size": 1.0})
    assert str(sde.value) == str(ode.value)
    for kw in (dict(method="reversible_heun", dt=1.0), dict(method="reversible_heun"),
               dict(method="reversible_heun", dt=0.5, adjoint_method="adjoint_reversible_heun", adaptive=False,
                    adjoint_adaptive=False, options=None, adjoint_options={}, rtol=1e-3, atol=1e-3, adjoint_rtol=1e-3,
                    adjoint_atol=1e-3, adjoint_params=()),
               dict(method="reversible_heun", dt=1.0, adjoint=False)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            _cpu_call(backend="torchsde", **kw)
    with pytest.raises(ValueError, match="Unrecognised backend=foo"):
        _cpu_call(backend="foo", method="reversible_heun")
    with pytest.raises(ValueError, match="Unrecognised backend=foo"):
        x = make_series(2, 5, 3)
        X = torchcde_amd.LinearInterpolation(x)
        torchcde_amd.cdeint(X, LinearField(4, 3), (torch.zeros(2, 4),), X.interval, backend="foo")
