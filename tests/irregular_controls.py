"""Inputs, references and bars shared by tests/test_host_irregular_knots.py and tests/test_gpu_24_irregular_knots.py: the fused
fixed-step solves on a control whose knots are irregular and do not start at zero.

Every fused kernel forms the control's slope itself: interval index and fractional part from the stage (node) table, and for a
linear control a division by knots[idx + 1] - knots[idx].  On the default knots arange(L) every width is 1, idx == floor(t) and
the solve starts at knot 0 with index 0, so a kernel that drops the division, pairs a coefficient row with its neighbour's
width, reads the wrong knot pointer or assumes interval 0 at the first stage computes the right numbers there.  Here:

    KNOTS   2.5 3.25 3.5 5.0 5.5 5.75 7.5 9.0 9.5 11.5     widths .75 .25 1.5 .5 .25 1.75 1.5 .5 2.0 -- none is 1
    T_OUT   2.75 4.0 6.125 11.0                             starts inside interval 0 at frac 0.25, ends before the last knot
    STEPS   0.5    grid points on the knots 3.25 and 5.75, the others between knots, several steps inside one interval
            0.75   stage times on knots (3.25, 3.5, 5.0, ...): `locate` resolves them to the interval on their left
            2.0    two or three knots crossed per step, the last step clipped to 0.25
            None   one step per output interval (1.25, 2.125, 4.875)

All of these are dyadic rationals, exact in float32: the float32 kernels and the float64 oracle see the same grid and choose the
same intervals, and no time sits on a knot by rounding.

A case is (family, shape, degree, step).  `reference(case)` holds its inputs, the float64 oracle's adjoint=True run (for
reversible Heun: tests/revheun_reference.py with autograd through it) and the same run in float32 on the CPU; `mutants(case)`
the float64 run on two wrong controls -- the slope of interval i divided by the width of interval i + 1, and the same
coefficients read on uniform knots -- which the host test requires to lie far outside the bars below.

Bars (the project's existing ones).  Trajectories: rtol 1e-4 with atol max(5e-6, 4 x the CPU float32 oracle's error of the
case).  Gradients: rtol 1e-3 with atol max(1e-3 max|want|, 4 x the CPU float32 error), against float64.  Reversible Heun
(tests/test_gpu_18_reversible_heun.py): rtol 1e-4 / atol 1e-5 and gradients rtol 1e-3 / atol 1e-3 max|want|.
"""
import collections
import functools

import torch
import torch.nn.functional as F

from oracle import cde as oracle_cde, interp as oracle_interp
from helpers import LinearField, TwoLayerField, make_series
import revheun_reference

KNOTS = (2.5, 3.25, 3.5, 5.0, 5.5, 5.75, 7.5, 9.0, 9.5, 11.5)
T_OUT = (2.75, 4.0, 6.125, 11.0)
STEPS = (0.5, 0.75, 2.0, None)
L = len(KNOTS)

Case = collections.namedtuple("Case", ["family", "shape", "degree", "step"])

# family -> (series per call, shapes, step sizes).  Shapes: (H, C, final tanh) for the one-layer field, (H, C, widths ..., hidden
# activation, final tanh) for the others.  33 series: one full 32-series tile and one series; 35: two 16-series tiles and three.
FAMILIES = {
    "affine": (33, [(H, C, tanh) for H, C in ((32, 8), (31, 7), (1, 8), (19, 5)) for tanh in (False, True)], STEPS),
    "mlp2": (35, [(32, 8, 128, "softplus", True), (16, 14, 64, "softplus", False)], STEPS),
    "mlp3": (35, [(32, 8, 128, 128, "relu", True), (5, 3, 20, 33, "softplus", False)], STEPS),
    "mlp2w": (35, [(16, 21, 100, "relu", False), (32, 64, 128, "softplus", True)], STEPS),
    "mlp2h": (35, [(40, 5, 64, "relu", False), (64, 32, 128, "softplus", True)], STEPS),
    "mlp2b": (35, [(5, 3, 129, "softplus", False), (32, 32, 200, "relu", True)], STEPS),
    "revheun": (33, [(H, C, tanh) for H, C in ((6, 3), (32, 8)) for tanh in (False, True)], STEPS[:3]),
}
# (family, shape, degree) -> series seed, where the default draw misses the host test's conditions.  This one: an identity field
# on 14 channels under a cubic control; at step 2.0 the default draw's states reach 440 and the float32 oracle is 2.5e-5 off.
SEEDS = {("mlp2", (16, 14, 64, "softplus", False), 3): 1003}
# (family, shape) -> factor on the output layer's weight and bias.  The shapes at the edge of an envelope sum 32 to 64 channels
# per hidden unit: unscaled, the coarse steps (2.0 and output to output) take their states to 60 .. 100, where float32 itself is
# 3e-5 .. 2.5e-4 of the largest entry away from float64 on dL/dz0 with every series seed tried (no kink: the field is smooth).
OUTPUT_SCALE = {("mlp2w", (32, 64, 128, "softplus", True)): 0.25, ("mlp2h", (64, 32, 128, "softplus", True)): 0.25,
                ("mlp2b", (32, 32, 200, "relu", True)): 0.25}


def cases(family, shapes=None):
    _, all_shapes, steps = FAMILIES[family]
    return [Case(family, shape, degree, step) for shape in (all_shapes if shapes is None else shapes) for degree in (3, 1)
            for step in steps]


def case_id(case):
    shape = "x".join("tanh" if v is True else "id" if v is False else str(v) for v in case.shape)
    return "%s_%s_deg%d_step%s" % (case.family, shape, case.degree, "out" if case.step is None else str(case.step).replace(".", "p"))


ALL_CASES = [c for family in FAMILIES for c in cases(family)]


# ------------------------------------------------------------------------------------------------ fields
class HiddenChoiceField(TwoLayerField):
    """helpers.TwoLayerField with the hidden activation as a choice: relu or torch's default softplus"""

    def __init__(self, H, C, width, dtype=torch.float32, seed=0, final_tanh=True, hidden="relu", scale=1.0):
        super().__init__(H, C, width, torch.float64, seed, final_tanh)
        self.hidden = hidden
        with torch.no_grad():
            self.linear2.weight.mul_(scale)
            self.linear2.bias.mul_(scale)
        self.to(dtype)

    def forward(self, t, z):
        y = self.linear2((F.softplus if self.hidden == "softplus" else torch.relu)(self.linear1(z)))
        if self.final_tanh:
            y = y.tanh()
        return y.view(*z.shape[:-1], self.H, self.C)


class ThreeLayerField(torch.nn.Module):
    def __init__(self, H, C, w1, w2, dtype=torch.float32, seed=0, final_tanh=True, hidden="relu"):
        super().__init__()
        self.H, self.C, self.final_tanh, self.hidden = H, C, final_tanh, hidden
        gen = torch.Generator().manual_seed(seed)
        self.first = torch.nn.Linear(H, w1).to(dtype)
        self.middle = torch.nn.Linear(w1, w2).to(dtype)
        self.last = torch.nn.Linear(w2, H * C).to(dtype)
        with torch.no_grad():
            for lin in (self.first, self.middle, self.last):
                bound = 1 / lin.in_features ** 0.5
                lin.weight.copy_((torch.rand(lin.weight.shape, generator=gen, dtype=torch.float64) * 2 - 1) * bound)
                lin.bias.copy_((torch.rand(lin.bias.shape, generator=gen, dtype=torch.float64) * 2 - 1) * bound)

    def forward(self, t, z):
        hid = F.softplus if self.hidden == "softplus" else torch.relu
        y = self.last(hid(self.middle(hid(self.first(z)))))
        if self.final_tanh:
            y = y.tanh()
        return y.view(*z.shape[:-1], self.H, self.C)


def make_field(case, dtype=torch.float32):
    """The case's vector field (the same weights in either precision: drawn in float64, then rounded)."""
    shape = case.shape
    if case.family in ("affine", "revheun"):
        return LinearField(shape[0], shape[1], dtype, scale=0.3, tanh=shape[2], seed=3)
    if case.family == "mlp3":
        H, C, w1, w2, hidden, final_tanh = shape
        return ThreeLayerField(H, C, w1, w2, dtype, seed=5, final_tanh=final_tanh, hidden=hidden)
    H, C, width, hidden, final_tanh = shape
    return HiddenChoiceField(H, C, width, dtype, seed=5, final_tanh=final_tanh, hidden=hidden,
                             scale=OUTPUT_SCALE.get((case.family, shape), 1.0))


# ------------------------------------------------------------------------------------------------ inputs and references
def knots(dtype=torch.float32):
    return torch.tensor(KNOTS, dtype=dtype)


def options(step):
    return None if step is None else dict(step_size=step)


def _seed(family, shape, degree):
    return SEEDS.get((family, shape, degree), 900 + 7 * shape[0] + shape[1])


@functools.lru_cache(maxsize=None)
def inputs(family, shape, degree):
    """(x, coeffs, z0, lw) of a (family, shape, degree), in float32 on the CPU; the step sizes share them."""
    B = FAMILIES[family][0]
    H, C = shape[:2]
    seed = _seed(family, shape, degree)
    x = make_series(B, L, C, torch.float32, seed=seed)
    coeffs = oracle_interp.hermite_bdiff_coeffs(x, knots()) if degree == 3 else oracle_interp.linear_coeffs(x, knots())
    gen = torch.Generator().manual_seed(seed + 1)
    z0 = torch.randn(B, H, generator=gen)
    lw = torch.rand(B, len(T_OUT), H, generator=gen) + 0.5
    return x, coeffs, z0, lw


def _path(case, coeffs, t):
    return (oracle_interp.CubicPath if case.degree == 3 else oracle_interp.LinearPath)(coeffs, t)


def _run(case, path, dtype, with_gradients=True, adjoint=True):
    """One solve of the case on `path` in `dtype`: out, and with gradients dL/dz0 (`z`) and dL/dparameter by name."""
    _, _, z0, lw = inputs(case.family, case.shape, case.degree)
    func = make_field(case, dtype)
    t = torch.tensor(T_OUT, dtype=dtype)
    z = z0.to(dtype).clone().requires_grad_(with_gradients)
    with torch.set_grad_enabled(with_gradients):
        if case.family == "revheun":
            out = revheun_reference.solve(path, func, z, t, case.step)
        else:
            out = oracle_cde.cdeint(path, func, z, t, adjoint=adjoint, method="rk4", options=options(case.step))
    run = dict(out=out.detach())
    if with_gradients:
        (out * lw.to(dtype)).sum().backward()
        run.update(z=z.grad, **{name: p.grad for name, p in func.named_parameters()})
    return run


@functools.lru_cache(maxsize=None)
def reference(case, adjoint=True):
    """The case's inputs and its two oracle runs, computed once and never modified.  f64: out, z (dL/dz0) and every parameter's
    gradient by name; f32: the same from the float32 run on the CPU (reversible Heun: the trajectory alone).  adjoint=False:
    autograd through the oracle's own steps, which is what cdeint(..., adjoint=False) is compared with under rk4."""
    x, coeffs, z0, lw = inputs(case.family, case.shape, case.degree)
    f64 = _run(case, _path(case, coeffs.double(), knots(torch.float64)), torch.float64, adjoint=adjoint)
    f32 = _run(case, _path(case, coeffs, knots()), torch.float32, with_gradients=case.family != "revheun", adjoint=adjoint)
    return dict(x=x, coeffs=coeffs, z0=z0, lw=lw, f64=f64, f32=f32, names=[n for n in f64 if n not in ("out", "z")])


def _shifted_widths_path(coeffs, t):
    """A LinearPath whose slope in interval i is divided by the width of interval i + 1 (the last: of interval 0)"""
    path = oracle_interp.LinearPath(coeffs, t)
    widths = torch.roll(t[1:] - t[:-1], -1)
    path._derivs = (coeffs[..., 1:, :] - coeffs[..., :-1, :]) / widths.unsqueeze(-1)
    return path


@functools.lru_cache(maxsize=None)
def mutants(case):
    """{name: float64 run} of the case on the wrong controls: "uniform_knots" (both degrees: the same coefficient tensor read on
    linspace(2.5, 11.5, 10) -- a kernel that ignores the knot tensor) and "shifted_widths" (linear: an off-by-one width)."""
    coeffs = inputs(case.family, case.shape, case.degree)[1].double()
    uniform = torch.linspace(KNOTS[0], KNOTS[-1], L, dtype=torch.float64)
    runs = {"uniform_knots": _run(case, _path(case, coeffs, uniform), torch.float64)}
    if case.degree == 1:
        runs["shifted_widths"] = _run(case, _shifted_widths_path(coeffs, knots(torch.float64)), torch.float64)
    return runs


# ------------------------------------------------------------------------------------------------ bars
def _gap(a, b):
    return (a.double() - b.double()).abs().max().item()


def cpu32_error(ref, name):
    """largest |float32 oracle - float64 oracle| of one result of the case (0 where the float32 run has none)"""
    return _gap(ref["f32"][name], ref["f64"][name]) if name in ref["f32"] else 0.0


def out_bar(case, ref):
    """(rtol, atol) of the trajectory"""
    if case.family == "revheun":
        return 1e-4, 1e-5
    return 1e-4, max(5e-6, 4 * cpu32_error(ref, "out"))


def grad_bar(case, ref, name):
    """(rtol, atol) of dL/dz0 (name "z") or of a parameter's gradient"""
    scale = ref["f64"][name].abs().max().item()
    if case.family == "revheun":
        return 1e-3, 1e-3 * scale
    return 1e-3, max(1e-3 * scale, 4 * cpu32_error(ref, name))


def widest(bar, want):
    """the bar at the largest entry, atol + rtol max|want|: no entry is allowed more"""
    return bar[1] + bar[0] * want.abs().max().item()
