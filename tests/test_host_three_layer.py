"""The three-layer field Linear -> hid -> Linear -> hid -> Linear -> act as far as it goes without a GPU: the probe's verdicts,
the dispatch rows of kind "mlp3", the argument checks of its four entry points, the closed-form adjoint dynamics of the
step-wise path, and a lane-level emulation of the two middle-layer images of csrc/cde_mlp3.h."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import torchcde_amd
from torchcde_amd import _lib
from torchcde_amd import dispatch as D
from torchcde_amd.fields import probe
from rejected_calls import build_args


class ThreeLayer(torch.nn.Module):
    def __init__(self, hid1, final_tanh, H=6, C=3, w1=10, w2=7, hid2=None, dtype=torch.float32):
        super().__init__()
        self.H, self.C, self.final_tanh = H, C, final_tanh
        self.hid1, self.hid2 = hid1, hid1 if hid2 is None else hid2
        self.first = torch.nn.Linear(H, w1).to(dtype)
        self.middle = torch.nn.Linear(w1, w2).to(dtype)
        self.last = torch.nn.Linear(w2, H * C).to(dtype)

    def forward(self, t, z):
        y = self.last(self.hid2(self.middle(self.hid1(self.first(z)))))
        return (y.tanh() if self.final_tanh else y).view(*z.shape[:-1], self.H, self.C)


def _probe(func, H=6, seed=0):
    z = torch.randn(9, H, generator=torch.Generator().manual_seed(seed))
    return probe(func, torch.tensor(0.25), z)[0]


# ------------------------------------------------------------------------------------------------ the probe
@pytest.mark.parametrize("final_tanh", [False, True])
@pytest.mark.parametrize("hidden", ["relu", "softplus"])
def test_probe_recognises_the_three_layer_field(hidden, final_tanh):
    torch.manual_seed(1)
    func = ThreeLayer(torch.relu if hidden == "relu" else F.softplus, final_tanh)
    found = _probe(func)
    assert found is not None and found.kind == "mlp3"
    assert found.linears == (func.first, func.middle, func.last)              # evaluation order, not registration order
    assert (found.hidden, found.middle, found.output) == found.linears
    assert found.act == (_lib.ACT_TANH if final_tanh else _lib.ACT_NONE)
    assert found.hidden_act == (_lib.HIDDEN_RELU if hidden == "relu" else _lib.HIDDEN_SOFTPLUS)
    assert found.code == found.act | (found.hidden_act << 4) == _lib.field_act(found.act, found.hidden_act)
    assert found.weight is func.last.weight and found.bias is func.last.bias
    assert _probe(func) is found                                              # the verdict is cached per fingerprint


def test_probe_orders_the_layers_by_evaluation():
    class Shuffled(ThreeLayer):                                               # registered last -> first
        def __init__(self):
            torch.nn.Module.__init__(self)
            self.H, self.C, self.final_tanh, self.hid1, self.hid2 = 6, 3, True, torch.relu, torch.relu
            self.last, self.middle, self.first = torch.nn.Linear(7, 18), torch.nn.Linear(10, 7), torch.nn.Linear(6, 10)

    torch.manual_seed(1)
    func = Shuffled()
    found = _probe(func)
    assert found is not None and found.kind == "mlp3" and found.linears == (func.first, func.middle, func.last)


def test_probe_refuses_the_three_layer_lookalikes():
    torch.manual_seed(2)

    class NoBias(ThreeLayer):
        def __init__(self, which):
            super().__init__(torch.relu, True)
            old = getattr(self, which)
            setattr(self, which, torch.nn.Linear(old.in_features, old.out_features, bias=False))

    class FourLayers(ThreeLayer):
        def __init__(self):
            super().__init__(torch.relu, True)
            self.extra = torch.nn.Linear(7, 7)

        def forward(self, t, z):
            y = self.last(self.extra(self.middle(self.first(z).relu()).relu()).relu())
            return y.tanh().view(*z.shape[:-1], self.H, self.C)

    class Skip(ThreeLayer):
        def forward(self, t, z):
            u1 = self.first(z).relu()
            y = self.last(self.middle(u1).relu() + u1[..., :7])
            return y.tanh().view(*z.shape[:-1], self.H, self.C)

    class Scaled(ThreeLayer):
        def forward(self, t, z):
            return super().forward(t, z) * 1.0001

    class MiddleScaled(ThreeLayer):
        def forward(self, t, z):
            y = self.last((self.middle(self.first(z).relu()) * 0.5).relu())
            return y.tanh().view(*z.shape[:-1], self.H, self.C)

    class TimeDependent(ThreeLayer):
        def forward(self, t, z):
            return super().forward(t, z) * (1 + t)

    class SharedLayer(torch.nn.Module):                                       # one Linear applied twice (tests/test_host.py)
        def __init__(self):
            super().__init__()
            self.l, self.out = torch.nn.Linear(6, 6), torch.nn.Linear(6, 18)

        def forward(self, t, z):
            return self.out(self.l(self.l(z).relu()).relu()).view(*z.shape[:-1], 6, 3)

    class SharedOfThree(ThreeLayer):                                          # three Linears owned, the middle one applied twice
        def __init__(self):
            super().__init__(torch.relu, True, w1=7, w2=7)

        def forward(self, t, z):
            y = self.last(self.middle(self.middle(self.first(z).relu()).relu()).relu())
            return y.tanh().view(*z.shape[:-1], self.H, self.C)

    class ExtraParameter(ThreeLayer):
        def __init__(self):
            super().__init__(torch.relu, True)
            self.scale = torch.nn.Parameter(torch.ones(()))

    bad = {
        "mixed_relu_softplus": ThreeLayer(torch.relu, True, hid2=F.softplus),
        "mixed_softplus_relu": ThreeLayer(F.softplus, False, hid2=torch.relu),
        "tanh_hidden": ThreeLayer(torch.tanh, True),
        "tanh_second_hidden": ThreeLayer(torch.relu, True, hid2=torch.tanh),
        "silu_hidden": ThreeLayer(F.silu, False),
        "softplus_beta_2": ThreeLayer(lambda x: F.softplus(x, beta=2), True),
        "relu6_hidden": ThreeLayer(F.relu6, True),
        "no_hidden_activation": ThreeLayer(lambda x: x, True),
        "shared_layer": SharedLayer(), "shared_of_three": SharedOfThree(), "four_layers": FourLayers(),
        "no_bias_first": NoBias("first"), "no_bias_middle": NoBias("middle"), "no_bias_last": NoBias("last"),
        "skip": Skip(torch.relu, True), "scaled": Scaled(torch.relu, True), "middle_scaled": MiddleScaled(torch.relu, True),
        "time_dependent": TimeDependent(F.softplus, False), "extra_parameter": ExtraParameter(),
    }
    for name, func in bad.items():
        assert _probe(func) is None, name


def test_one_and_two_layer_modules_classify_as_before():
    """The modules of tests/test_host.py::test_probe_accepts_exactly_the_fused_families, next to the new kind."""
    torch.manual_seed(0)
    z = torch.randn(4, 3)
    t = torch.tensor(0.0)

    class Readme(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.linear = torch.nn.Linear(3, 6)

        def forward(self, t, z):
            return self.linear(z).view(4, 3, 2)

    class Irregular(Readme):
        def forward(self, t, z):
            return self.linear(z).tanh().view(*z.shape[:-1], 3, 2)

    class TwoLayer(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.l1, self.l2 = torch.nn.Linear(3, 5), torch.nn.Linear(5, 6)

        def forward(self, t, z):
            return self.l2(self.l1(z).relu()).tanh().view(4, 3, 2)

    class TwoLayerUnusedThird(TwoLayer):                                      # owns a Linear it never applies: no family
        def __init__(self):
            super().__init__()
            self.l3 = torch.nn.Linear(5, 5)

    field, system = probe(Readme(), t, z)
    assert field.kind == "affine" and field.act == _lib.ACT_NONE and system.shape == (4, 3, 2)
    assert probe(Irregular(), t, z)[0].act == _lib.ACT_TANH
    field = probe(torchcde_amd.LinearCDEFunc(2, 3, tanh=True), t, z)[0]
    assert field.kind == "affine" and field.act == _lib.ACT_TANH
    field = probe(TwoLayer(), t, z)[0]
    assert field.kind == "mlp2" and field.act == _lib.ACT_TANH and field.hidden_act == _lib.HIDDEN_RELU
    assert field.hidden.out_features == 5 and field.output.out_features == 6 and len(field.linears) == 2
    assert probe(TwoLayerUnusedThird(), t, z)[0] is None


# ------------------------------------------------------------------------------------------------ dispatch
def test_dispatch_rows_of_the_three_layer_field():
    """select_path for kind "mlp3" over every flag, three methods and the three parameter kinds (contradictory requests pruned
    as tests/test_host.py::test_dispatch_table_is_exhaustively_consistent prunes them: no MFMA-shape / reverse-mode / identity
    flags for this kind).  Fused exactly under the stated conditions, a reason with every step-wise verdict."""
    flags = ["prod", "tiles_ok", "adjoint", "wants_grad", "wants_t", "wants_control", "adjoint_method_ok", "options_ok",
             "adjoint_options_ok", "t_ok", "variant_generic", "shared", "narrow_control", "control_block"]
    seen = {}
    n = 0
    for method in ("rk4", "dopri5", "midpoint"):
        for params in ("default", "own", "foreign"):
            for bits in itertools.product((False, True), repeat=len(flags)):
                f = dict(zip(flags, bits))
                if (f["wants_t"] or f["wants_control"]) and not f["wants_grad"]:
                    continue
                if f["control_block"] and not (f["wants_control"] and f["adjoint"] and params == "own"):
                    continue
                q = D.Request(kind="mlp3", method=method, params=params, mfma_shape=False, backprop_ok=False, identity=False, **f)
                c = D.select_path(q)
                n += 1
                seen[c.path] = seen.get(c.path, 0) + 1
                base = (not f["prod"] and f["tiles_ok"] and f["t_ok"] and method == "rk4" and f["options_ok"]
                        and not f["variant_generic"])
                want = D.STEPWISE
                if base and not f["wants_grad"]:
                    want = "mlp_rk4_forward"
                elif (base and f["adjoint"] and f["adjoint_method_ok"] and f["adjoint_options_ok"] and params != "foreign"
                      and not f["wants_t"] and not f["wants_control"]):
                    want = "mlp_rk4_adjoint"
                assert c.path == want, (q, c)
                assert (c.path == D.STEPWISE) == bool(c.reason)
    assert n > 10000 and set(seen) == {"mlp_rk4_forward", "mlp_rk4_adjoint", D.STEPWISE}

    def ask(**kw):
        base = dict(prod=False, kind="mlp3", tiles_ok=True, mfma_shape=False, method="rk4", adjoint=True, wants_grad=True,
                    wants_t=False, wants_control=False, params="default", adjoint_method_ok=True, options_ok=True,
                    adjoint_options_ok=True, t_ok=True, variant_generic=False, shared=False, narrow_control=True,
                    backprop_ok=False, identity=False, control_block=False)
        base.update(kw)
        return D.select_path(D.Request(**base))
    assert ask().path == "mlp_rk4_adjoint" and ask(params="own").path == "mlp_rk4_adjoint"
    assert ask(wants_grad=False).path == ask(wants_grad=False, adjoint=False).path == "mlp_rk4_forward"
    # the default method, the other fixed-grid methods, adjoint=False, time / control gradients, the shared controller
    for kw in (dict(method="dopri5"), dict(method="dopri5", wants_grad=False), dict(method="dopri5", shared=True),
               dict(method="midpoint"), dict(method="euler", wants_grad=False), dict(adjoint=False), dict(wants_t=True),
               dict(wants_control=True, params="own"), dict(params="foreign"), dict(adjoint_method_ok=False),
               dict(adjoint_options_ok=False), dict(options_ok=False)):
        verdict = ask(**kw)
        assert verdict.path == D.STEPWISE and "three-layer" in verdict.reason and "rk4" in verdict.reason, (kw, verdict)
    assert "generic" in ask(variant_generic=True).reason
    assert "tiles" in ask(tiles_ok=False).reason and "increasing" in ask(t_ok=False).reason
    # nothing moved for the other kinds
    assert ask(kind="mlp2", backprop_ok=True).path == "mlp_rk4_adjoint"
    assert ask(kind="mlp2", backprop_ok=True, adjoint=False).path == "mlp_rk4_backprop"
    assert ask(kind="mlp2", method="dopri5").path == "mlp_dopri5_adjoint"
    assert ask(kind="affine", mfma_shape=True, identity=True, backprop_ok=True).path == "rk4"


# ------------------------------------------------------------------------------------------------ the C ABI
CALLS3 = {
    "cde_rk4_forward_mlp3": "coeffs knots n_intervals=4 degree=3 W1 bias1 width1=32 Wm biasm width2=24 W2 bias2 act=1 z0 grid "
                            "n_grid=5 t_out n_out=2 z_out B=64 C=8 H=32 dtype=0 time_dtype=0 stage_index stage_frac stream=0",
    "cde_rk4_adjoint_mlp3_workspace_bytes": "n_sgrid=5",
    "cde_rk4_adjoint_mlp3_prepare": "knots n_intervals=4 sgrid n_sgrid=5 W1 bias1 width1=32 Wm biasm width2=24 W2 bias2 C=8 H=32 "
                                    "dtype=0 time_dtype=0 workspace workspace_bytes=1073741824 stream=0",
    "cde_rk4_adjoint_mlp3_sweep": "coeffs knots n_intervals=4 degree=3 act=1 y_state a_state sgrid n_sgrid=5 k_begin=0 k_end=4 U "
                                  "U1 G2 Gm G1 Z B=64 C=8 H=32 dtype=0 time_dtype=0 workspace workspace_bytes=1073741824 stream=0",
}
# entry point -> {code: overrides of the valid call above that must return it}: the ORDER of the checks -- sizes (-3), unknown
# dtype (-2), the forward solve's empty batch (0), the envelope (-4), pointers (-1), the workspace one byte short (-5; the
# size is asked of the library below)
REJECTED3 = {
    "cde_rk4_forward_mlp3": {
        -3: ["C=0", "H=0", "n_intervals=0", "B=-1", "width1=0", "width2=0", "n_out=0", "n_grid=0", "C=0 dtype=7", "H=0 coeffs=0"],
        -2: ["dtype=7", "time_dtype=7", "dtype=7 H=33", "dtype=7 B=0"],
        0: ["B=0", "B=0 H=33", "B=0 coeffs=0", "B=0 dtype=1"],
        -4: ["dtype=1", "H=33", "C=9", "width1=129", "width2=129", "act=5", "act=33", "act=256", "H=33 coeffs=0",
             "dtype=1 Wm=0", "C=16 H=16"],
        -1: ["coeffs=0", "knots=0", "W1=0", "bias1=0", "Wm=0", "biasm=0", "W2=0", "bias2=0", "z0=0", "grid=0", "t_out=0",
             "z_out=0", "stage_index=0", "stage_frac=0"],
    },
    "cde_rk4_adjoint_mlp3_prepare": {
        -3: ["C=0", "H=0", "n_intervals=0", "width1=0", "width2=0", "n_sgrid=-1", "C=0 dtype=7"],
        -2: ["dtype=7", "dtype=7 H=33"],
        -4: ["dtype=1", "H=33", "C=9", "width1=129", "width2=129", "H=33 knots=0", "C=16 H=16"],
        -1: ["knots=0", "sgrid=0", "W1=0", "bias1=0", "Wm=0", "biasm=0", "W2=0", "bias2=0", "workspace=0",
             "workspace=0 workspace_bytes=0"],
        -5: ["workspace_bytes=SHORT"],
    },
    "cde_rk4_adjoint_mlp3_sweep": {
        -3: ["C=0", "H=0", "n_intervals=0", "B=0", "B=-1", "k_begin=-1", "k_begin=3 k_end=2", "k_end=5", "B=0 dtype=7"],
        -2: ["dtype=7", "dtype=7 act=5"],
        -4: ["dtype=1", "H=33", "C=9", "act=5", "act=33", "act=256", "act=5 coeffs=0", "C=16 H=16"],
        -1: ["coeffs=0", "knots=0", "y_state=0", "a_state=0", "sgrid=0", "U=0", "U1=0", "G2=0", "Gm=0", "G1=0", "Z=0",
             "workspace=0", "workspace=0 workspace_bytes=0"],
        -5: ["workspace_bytes=SHORT"],
    },
}


def test_three_layer_entry_points_reject_bad_calls_without_a_gpu():
    """Dummy pointers, no device: every row fails a check that comes before the first HIP call (tests/rejected_calls.py)."""
    lib = torchcde_amd.load()
    need = lib.cde_rk4_adjoint_mlp3_workspace_bytes(5)
    # [stage_index: 16 int64][stage_frac: 16 f32][images]: K3m's LDS images, bm, W1^T and the two middle-layer images
    images = (4096 + 128 + 256 * 132 + 256) + 128 + 2 * 8 * 64 * 4 + 2 * 8 * 8 * 64 * 4
    assert need == 256 + 256 + 4 * images and need % 256 == 0
    assert lib.cde_rk4_adjoint_mlp3_workspace_bytes(1) == lib.cde_rk4_adjoint_mlp3_workspace_bytes(0) == 4 * images
    assert set(REJECTED3) | {"cde_rk4_adjoint_mlp3_workspace_bytes"} == set(CALLS3) <= set(_lib.EXPORTED_SYMBOLS)
    wrong = []
    for name, by_code in REJECTED3.items():
        call = getattr(lib, name)
        assert call(*build_args(CALLS3[name], "coeffs=0" if "coeffs" in CALLS3[name] else "knots=0")) == -1   # valid but for one pointer
        for code, cases in by_code.items():
            for overrides in cases:
                got = call(*build_args(CALLS3[name], overrides.replace("SHORT", str(need - 1))))
                if got != code:
                    wrong.append("%s(%s): %d, expected %d" % (name, overrides, got, code))
    assert not wrong, "\n".join(wrong)
    assert lib.cde_abi_version() == 3 == _lib.ABI_VERSION                     # the change is additive


# ------------------------------------------------------------------------------------------------ step-wise closed form
@pytest.mark.parametrize("final_tanh", [True, False])
@pytest.mark.parametrize("hidden", ["relu", "softplus"])
def test_closed_form_adjoint_dynamics_of_the_three_layer_field_equal_autograd(monkeypatch, hidden, final_tanh):
    """stepwise._explicit_dynamics on a three-layer module against torch.autograd.grad through the module, float64 on the CPU
    (as tests/test_host.py::test_closed_form_adjoint_dynamics_equal_autograd): all six parameters reversed, and a subset."""
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
    H, C = 5, 3
    for lead in ((7,), (2, 4)):
        func = ThreeLayer(torch.relu if hidden == "relu" else F.softplus, final_tanh, H, C, 9, 6, dtype=torch.float64)
        if hidden == "softplus":
            with torch.no_grad():                         # pre-activations above torch's threshold of 20 and far below zero
                func.first.bias[0] = 25.0
                func.middle.bias[1] = -30.0
                func.middle.bias[2] = 28.0
        y = torch.randn(*lead, H, dtype=torch.float64)
        a = torch.randn(*lead, H, dtype=torch.float64)
        t = torch.tensor(0.3, dtype=torch.float64)
        recognised, _ = probe(func, t, y)
        assert recognised is not None and recognised.kind == "mlp3"
        field = stepwise.ControlledField(Path(torch.randn(*lead, C, dtype=torch.float64)), func)
        field.recognised = recognised
        every = tuple(reversed(list(func.parameters())))
        for params in (every, (func.middle.bias, func.first.weight, func.last.weight), (func.middle.weight,), ()):
            saved = tuple(p.detach().view_as(p) for p in params)          # same memory, different tensor objects
            run = stepwise._explicit_dynamics(field, saved)
            assert run is not None
            with torch.no_grad():
                fe, vy, vp = run(t, y, a)
            yy = y.clone().requires_grad_(True)
            want_f = field(t, yy)
            want = torch.autograd.grad(want_f, (yy,) + params, -a)
            assert torch.allclose(fe, want_f.detach(), rtol=1e-12, atol=1e-13)
            assert torch.allclose(vy, want[0], rtol=1e-11, atol=1e-12)
            assert len(vp) == len(params)
            for got, ref, p in zip(vp, want[1:], params):
                assert got.shape == p.shape
                assert torch.allclose(got, ref, rtol=1e-11, atol=1e-12)
        stranger = torch.nn.Parameter(torch.zeros(3, dtype=torch.float64))
        assert stepwise._explicit_dynamics(field, (func.middle.weight, stranger)) is None


# ------------------------------------------------------------------------------------------------ the middle-layer images
def _mfma_16x16x4(a_lane, b_lane, acc):
    """v_mfma_f32_16x16x4_f32: lane l supplies A[i=l&15][k=l>>4], B[k=l>>4][j=l&15]; register r of lane l holds
    D[4*(l>>4)+r][l&15] (tests/test_host.py)."""
    A = np.zeros((16, 4)); Bm = np.zeros((4, 16))
    for l in range(64):
        A[l & 15, l >> 4] = a_lane[l]
        Bm[l >> 4, l & 15] = b_lane[l]
    P = A @ Bm
    for l in range(64):
        for r in range(4):
            acc[l, r] += P[4 * (l >> 4) + r, l & 15]


def _wm_image(Wm, transposed):
    """csrc/cde_mlp3.h: wm_image as a flat array [output tile][K tile][lane][r], zero outside the real (width2, width1).
    forward:     A[i][kq] of (output tile T', K step (T1, r)) = Wm[16 T' + i][16 T1 + 4 kq + r]
    transposed:  A[i][kq] of (output tile T1, K step (T', r)) = Wm[16 T' + 4 kq + r][16 T1 + i]"""
    w2, w1 = Wm.shape
    img = np.zeros(8 * 8 * 64 * 4)
    for e in range(img.size):
        r, l, g = e & 3, (e >> 2) & 63, e >> 8
        i, kq, To, Tk = l & 15, l >> 4, g >> 3, g & 7
        row, col = (16 * Tk + 4 * kq + r, 16 * To + i) if transposed else (16 * To + i, 16 * Tk + 4 * kq + r)
        if row < w2 and col < w1:
            img[e] = Wm[row, col]
    return img


@pytest.mark.parametrize("w1,w2", [(20, 12), (100, 36), (128, 128)])
def test_middle_layer_images_chain_from_layer_ones_fragment(w1, w2):
    """The kernels' reads of the two images -- float4 number (8 To + Tk) * 64 + lane, component r -- fed to the 16x16x4 chain
    with layer 1's C/D fragment as the B operand: lane (n, q) holds u1[4 T1 + r] = unit 16 T1 + 4 q + r of series n.  The
    chain must leave Wm u1 + bm in the same fragment form (the B operand of layer 2), and Wm^T g in the form of u1; padded
    units are fed with a non-zero value, as softplus(0) = ln 2 is, and must not leak through the zero padding."""
    rng = np.random.default_rng(7)
    Wm = rng.standard_normal((w2, w1)) * 0.3
    bm = rng.standard_normal(w2)
    u1_real = rng.standard_normal((16, w1))
    g_real = rng.standard_normal((16, w2))
    u1_pad = np.full((16, 128), np.log(2.0)); u1_pad[:, :w1] = u1_real
    g_pad = np.full((16, 128), 0.75); g_pad[:, :w2] = g_real
    lanes = [(l & 15, l >> 4) for l in range(64)]
    fwd, tr = _wm_image(Wm, False), _wm_image(Wm, True)
    assert np.count_nonzero(fwd) == np.count_nonzero(tr) == np.count_nonzero(Wm)
    assert np.allclose(np.sort(fwd[fwd != 0]), np.sort(Wm.ravel())) and np.allclose(np.sort(tr[tr != 0]), np.sort(Wm.ravel()))

    def fragment(x):                                                          # per-lane registers x[4 T + r]
        reg = np.zeros((64, 32))
        for l, (n, q) in enumerate(lanes):
            for T in range(8):
                reg[l, 4 * T:4 * T + 4] = x[n, 16 * T + 4 * q:16 * T + 4 * q + 4]
        return reg

    def chain(img, b_reg, init):
        out = np.zeros((64, 32))
        for To in range(8):
            acc = np.zeros((64, 4))
            for l, (n, q) in enumerate(lanes):
                for r in range(4):
                    acc[l, r] = init(16 * To + 4 * q + r)
            for Tk in range(8):
                for r in range(4):
                    a_lane = [img[((8 * To + Tk) * 64 + l) * 4 + r] for l in range(64)]
                    _mfma_16x16x4(a_lane, b_reg[:, 4 * Tk + r], acc)
            out[:, 4 * To:4 * To + 4] = acc
        return out

    # bias image [tile][q][r] = bm[16 T' + 4 q + r], zero beyond width2: the accumulator's initial value
    pre2 = chain(fwd, fragment(u1_pad), lambda unit: bm[unit] if unit < w2 else 0.0)
    want = np.zeros((16, 128)); want[:, :w2] = u1_real @ Wm.T + bm
    assert np.allclose(pre2, fragment(want), rtol=1e-12, atol=1e-12)
    gu1 = chain(tr, fragment(g_pad), lambda unit: 0.0)
    want = np.zeros((16, 128)); want[:, :w1] = g_real @ Wm
    assert np.allclose(gu1, fragment(want), rtol=1e-12, atol=1e-12)
