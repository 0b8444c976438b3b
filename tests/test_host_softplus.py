"""The two-layer field with a softplus hidden layer, as far as it goes without a GPU: the probe's verdicts, the hidden
activation's code in the C ABI's `int act`, and the closed-form adjoint dynamics of the step-wise path."""
import pytest
import torch
import torch.nn.functional as F

import torchcde_amd
from torchcde_amd import _lib
from torchcde_amd.fields import probe
from rejected_calls import CALLS, build_args


class TwoLayer(torch.nn.Module):
    def __init__(self, inner, final_tanh, H=6, C=3, width=10, dtype=torch.float32):
        super().__init__()
        self.H, self.C, self.inner, self.final_tanh = H, C, inner, final_tanh
        self.linear1 = torch.nn.Linear(H, width).to(dtype)
        self.linear2 = torch.nn.Linear(width, H * C).to(dtype)

    def forward(self, t, z):
        y = self.linear2(self.inner(self.linear1(z)))
        return (y.tanh() if self.final_tanh else y).view(*z.shape[:-1], self.H, self.C)


def _probe(func, seed=0):
    z = torch.randn(9, func.H, generator=torch.Generator().manual_seed(seed))
    return probe(func, torch.tensor(0.25), z)[0]


@pytest.mark.parametrize("final_tanh", [False, True])
@pytest.mark.parametrize("inner", [F.softplus, torch.nn.Softplus(), lambda x: F.softplus(x, beta=1, threshold=20)],
                         ids=["functional", "module", "defaults_spelled_out"])
def test_probe_recognises_the_softplus_field(inner, final_tanh):
    torch.manual_seed(1)
    found = _probe(TwoLayer(inner, final_tanh))
    assert found is not None and found.kind == "mlp2"
    assert found.hidden_act == _lib.HIDDEN_SOFTPLUS
    assert found.act == (_lib.ACT_TANH if final_tanh else _lib.ACT_NONE)
    assert found.code == found.act | (1 << 4)                     # what the two-layer entry points get as `act`


def test_relu_field_keeps_its_verdict_and_its_code():
    torch.manual_seed(1)
    for final_tanh in (False, True):
        found = _probe(TwoLayer(torch.relu, final_tanh))
        assert found is not None and found.kind == "mlp2" and found.hidden_act == _lib.HIDDEN_RELU
        assert found.code == found.act == (_lib.ACT_TANH if final_tanh else _lib.ACT_NONE)


@pytest.mark.parametrize("name,inner", [
    ("beta_2", lambda x: F.softplus(x, beta=2)),
    ("threshold_5", lambda x: F.softplus(x, threshold=5)),
    # (in float32 this one computes what the default computes: refused on its arguments, not on its values)
    ("threshold_30", lambda x: F.softplus(x, threshold=30)),
    ("module_beta_half", torch.nn.Softplus(beta=0.5)),
    ("silu", F.silu), ("elu", F.elu), ("gelu", F.gelu), ("sigmoid", torch.sigmoid), ("leaky_relu", F.leaky_relu),
    ("softplus_scaled", lambda x: F.softplus(x) * 1.5),
    ("softplus_shifted", lambda x: F.softplus(x) - 0.6931471805599453),
])
def test_probe_refuses_every_other_hidden_activation(name, inner):
    torch.manual_seed(2)
    for final_tanh in (False, True):
        assert _probe(TwoLayer(inner, final_tanh)) is None, name


def test_probes_far_input_separates_softplus_thresholds_by_value_too():
    """The second line of defence behind the argument check: on the probe's far input (z * 37 + 11) a softplus with threshold
    5 differs bitwise from the default one, because pre-activations land between 5 and 16."""
    torch.manual_seed(2)
    func = TwoLayer(F.softplus, True)
    z = torch.randn(9, func.H, generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        pre = func.linear1(z * 37.0 + 11.0)
    assert ((pre > 5) & (pre < 16)).any()
    assert not torch.equal(F.softplus(pre), F.softplus(pre, threshold=5))


# ------------------------------------------------------------------------------------------------ the C ABI
# the adaptive two-layer entry points (their valid calls: tests/rejected_calls.py)
_ADAPTIVE = ["cde_dopri5_advance_mlp", "cde_dopri5_advance_mlp_sharded", "cde_dopri5_adjoint_mlp_advance",
             "cde_dopri5_adjoint_mlp_advance_dcontrol", "cde_dopri5_adjoint_mlp_advance_sharded"]
_FIXED = ["cde_rk4_forward_mlp", "cde_rk4_forward_mlp_stages", "cde_rk4_adjoint_mlp_sweep", "cde_rk4_backprop_mlp_sweep",
          "cde_rk4_backprop_mlp_sweep_dcontrol"]


def _args(name, overrides):
    return build_args(CALLS[name], overrides)


def test_abi_keeps_its_version_and_the_python_mirror_of_the_codes():
    assert torchcde_amd.load().cde_abi_version() == 3 == _lib.ABI_VERSION
    assert (_lib.HIDDEN_RELU, _lib.HIDDEN_SOFTPLUS) == (0, 1)
    assert _lib.field_act(_lib.ACT_TANH) == 1 and _lib.field_act(_lib.ACT_NONE, _lib.HIDDEN_SOFTPLUS) == 16
    assert _lib.field_act(_lib.ACT_TANH, _lib.HIDDEN_SOFTPLUS) == 17


@pytest.mark.parametrize("name", _FIXED + sorted(_ADAPTIVE))
def test_two_layer_entry_points_turn_unknown_hidden_codes_away_without_a_gpu(name):
    """Dummy pointers, no device: an unknown hidden code (bits 4-7 of `act` = 2..15, with either final activation) is
    CDE_ERR_UNSUPPORTED from the argument checks; the known ones pass them -- the call then ends at the checks behind,
    exactly as with act = 0 / 1 before: -1 for a NULL pointer, 0 for the fixed-grid forward solves' empty batch."""
    call = getattr(torchcde_amd.load(), name)
    for hidden in range(2, 16):
        for final in (0, 1):
            assert call(*_args(name, "act=%d" % (final | hidden << 4))) == -4, (hidden, final)
    assert call(*_args(name, "act=%d" % (1 | 1 << 8))) == -4                  # nothing lives above bit 7
    for code in (0, 1, 16, 17):
        assert call(*_args(name, "act=%d coeffs=0" % code)) == -1, code
        if name.startswith("cde_rk4_forward_mlp"):
            assert call(*_args(name, "act=%d B=0" % code)) == 0, code


@pytest.mark.parametrize("name", ["cde_rk4_forward_linear", "cde_rk4_adjoint_linear", "cde_rk4_backprop_linear"])
def test_one_layer_entry_points_still_know_two_activations_only(name):
    call = getattr(torchcde_amd.load(), name)
    for act in (16, 17, 2, 32):
        assert call(*build_args(CALLS[name], "act=%d" % act)) == -4, act


# ------------------------------------------------------------------------------------------------ step-wise closed form
def test_closed_form_adjoint_dynamics_of_the_softplus_field_equal_autograd(monkeypatch):
    """stepwise._explicit_dynamics for Linear -> softplus -> Linear (-> tanh) against torch.autograd.grad in float64, as
    tests/test_host.py does for the relu field; one layer-1 bias puts pre-activations above torch's threshold of 20 (slope
    exactly 1 there) and far below zero."""
    from torchcde_amd import stepwise

    class CpuContract:                                    # cde_contract needs the GPU; the formula is all that matters here
        @staticmethod
        def apply(Fm, dX):
            return (Fm * dX.unsqueeze(-2)).sum(-1)

    monkeypatch.setattr(stepwise, "_Contract", CpuContract)

    class Path:
        def __init__(self, slope):
            self.slope = slope

        def derivative(self, t):
            return self.slope * (1 + t)

    torch.manual_seed(3)
    H, C, width = 5, 3, 9
    for lead in ((7,), (2, 4)):
        for final_tanh in (True, False):
            func = TwoLayer(F.softplus, final_tanh, H, C, width, torch.float64)
            with torch.no_grad():
                func.linear1.bias[0] = 25.0
                func.linear1.bias[1] = -30.0
            y = torch.randn(*lead, H, dtype=torch.float64)
            a = torch.randn(*lead, H, dtype=torch.float64)
            t = torch.tensor(0.3, dtype=torch.float64)
            with torch.no_grad():
                pre = func.linear1(y)
            assert (pre > 20).any() and (pre < -15).any()
            recognised, _ = probe(func, t, y)
            assert recognised is not None and recognised.hidden_act == _lib.HIDDEN_SOFTPLUS
            field = stepwise.ControlledField(Path(torch.randn(*lead, C, dtype=torch.float64)), func)
            field.recognised = recognised
            params = tuple(reversed([p for p in func.parameters()]))
            saved = tuple(p.detach().view_as(p) for p in params)
            run = stepwise._explicit_dynamics(field, saved)
            assert run is not None
            with torch.no_grad():
                fe, vy, vp = run(t, y, a)
            yy = y.clone().requires_grad_(True)
            want_f = field(t, yy)
            want = torch.autograd.grad(want_f, (yy,) + params, -a)
            assert torch.allclose(fe, want_f.detach(), rtol=1e-12, atol=1e-13)
            assert torch.allclose(vy, want[0], rtol=1e-11, atol=1e-12)
            for got, ref, p in zip(vp, want[1:], params):
                assert got.shape == p.shape
                assert torch.allclose(got, ref, rtol=1e-11, atol=1e-12)
