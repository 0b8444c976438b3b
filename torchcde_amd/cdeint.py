"""``cdeint``: the drop-in solver front-end (host side of K2 / K3).

Mirrors reference ``torchcde/solver.py:144-245`` -- same signature, defaults, ValueError messages
and output layout ``(..., len(t), hidden)`` -- and replaces what lies behind it
(``_VectorField.forward`` solver.py:117-135 and ``torchdiffeq.odeint[_adjoint]`` solver.py:226-227)
by ONE fused HIP kernel per direction.  What the native path covers is stated explicitly; anything
else raises ``NotImplementedError`` -- it never falls back to an eager/CPU computation.

Native scope (round 1):
  * X: ``torchcde_amd.CubicSpline`` or ``torchcde_amd.LinearInterpolation``
  * func: the affine family recognised by ``torchcde_amd.fields`` (Linear(H, H*C) [+ tanh] viewed (..., H, C))
  * backend "torchdiffeq", ``method='rk4'`` (torchdiffeq's 3/8-rule), ``options={'step_size': h}`` or no options
    (grid = t, torchdiffeq's behaviour), increasing ``t``, tensor state; gradients by the continuous adjoint
    (``adjoint=True``) for z0 and the field's weight / bias
  * ``method='dopri5'`` (also the default when no method is passed, as in the reference): adaptive solve with
    torchdiffeq's batch-global controller, ``rtol/atol`` and ``options={'jump_t': ...}``; fused forward
  * backend "torchsde": ``method='reversible_heun'`` (arXiv 2105.13493; fused for the affine family in float32, csrc/revheun.hip,
    step-wise otherwise) and ``method='midpoint'`` (rewritten as the torchdiffeq request with ``step_size=dt``)
  * everything else -- arbitrary ``func`` modules (MLPs ...), ``midpoint``/``euler``, ``adjoint=False`` backprop,
    gradients through ``dopri5`` -- runs step-wise (``torchcde_amd/stepwise.py``): host-driven stepping on the GPU
    with the native control-derivative and contraction kernels under every vector-field evaluation
"""
import ctypes
import sys
import threading
import types
import warnings
import weakref

import torch
from torch.autograd.function import once_differentiable as _once_differentiable

from . import _lib, dispatch
from .fields import probe
from .paths import _NativePath

_GRAD_WARNING = ("One of the inputs to the control path X requires gradients but "
                 "`kwargs['adjoint_params']` has not been passed. This is probably a mistake: these "
                 "inputs will not receive a gradient when using the adjoint method. Either have the input "
                 "not require gradients (if that was unintended), or include it (and every other "
                 "parameter needing gradients) in `adjoint_params`. For example:\n"
                 "```\n"
                 "coeffs = ...\n"
                 "func = ...\n"
                 "X = CubicSpline(coeffs)\n"
                 "adjoint_params = tuple(func.parameters()) + (coeffs,)\n"
                 "cdeint(X=X, func=func, ..., adjoint_params=adjoint_params)\n"
                 "```")


# ------------------------------------------------------------------------------------------ per-thread call state
class _CallState:
    """What a caller may ask about / configure for ITS OWN cdeint calls: the step statistics of its most recent adaptive
    solve and fused adaptive backward, whether the step traces are fetched as well (tests), and the list bench.py hands
    in to receive HIP events around the K2 / K3 C-ABI calls.  One per calling thread (like dispatch.last()); a plan
    remembers the state of the thread that built it, because autograd runs its backward on an engine thread."""
    __slots__ = ("dopri5", "dopri5_adjoint", "record", "event_log")

    def __init__(self):
        self.dopri5, self.dopri5_adjoint, self.record, self.event_log = {}, {}, False, None


_tls = threading.local()


def _state():
    st = getattr(_tls, "state", None)
    if st is None:
        st = _tls.state = _CallState()
    return st


# ------------------------------------------------------------------------------------------ time grids
def _fixed_grid(t, step_size):
    """torchdiffeq's fixed-grid constructor, evaluated with the same torch ops on
    the host: ``n = ceil((t[-1]-t[0])/h + 1)``; ``grid = arange(n)*h + t[0]``; ``grid[-1] = t[-1]``."""
    if step_size is None:
        grid = t.clone()
    else:
        n = torch.ceil((t[-1] - t[0]) / step_size + 1).item()
        grid = torch.arange(0, n, dtype=t.dtype, device=t.device) * step_size + t[0]
        grid[-1] = t[-1]
    if not (grid[0] == t[0] and grid[-1] == t[-1]):
        raise AssertionError("time grid does not span [t[0], t[-1]]")
    return grid


def _parse_fixed_options(options, what):
    options = {} if options is None else dict(options)
    step_size = options.pop("step_size", None)
    if options.pop("grid_constructor", None) is not None:
        raise NotImplementedError("torchcde_amd: %s option 'grid_constructor' is not supported natively" % what)
    if options.pop("perturb", False):
        raise NotImplementedError("torchcde_amd: %s option 'perturb' is not supported natively" % what)
    if options.pop("interp", "linear") != "linear":
        raise NotImplementedError("torchcde_amd: only interp='linear' is supported natively")
    options.pop("norm", None)  # only used by adaptive solvers
    if options:
        raise NotImplementedError("torchcde_amd: unsupported %s options %s" % (what, sorted(options)))
    return step_size


def _strip_noops(opts, fixed):
    """Options as the fused paths see them: keys whose value is None are absent (torchdiffeq's `options.get(key)`
    semantics), and for the fixed-grid methods so are torchdiffeq's defaults spelled out -- interp='linear',
    perturb=False -- and `norm`, which only adaptive solvers read.  ADVICE round 3: the dispatch test and the plans used
    to judge these differently (a fused call went step-wise over interp='linear'; safety=None raised a TypeError)."""
    if not isinstance(opts, dict):
        return opts
    out = {k: v for k, v in opts.items() if v is not None}
    if fixed:
        if out.get("interp") == "linear":
            del out["interp"]
        if out.get("perturb") is False:
            del out["perturb"]
        out.pop("norm", None)
    return out


_host_copies = {}      # id(time tensor) -> (weakref, version, host copy): avoids a D2H sync per call
_grid_cache = {}       # (times, dtype, steps, device) -> device-resident solver grids


def _to_host(t):
    """CPU copy of a (small) time tensor.  A GPU tensor costs one synchronising D2H copy the first time it is
    seen; ``CubicSpline.interval`` hands out one cached tensor object, so steady-state calls do not sync.
    (Keyed by id + weakref: tensors cannot be WeakKeyDictionary keys because ``==`` is elementwise.)"""
    if not t.is_cuda:
        return t.detach()
    key = id(t)
    hit = _host_copies.get(key)
    if hit is not None and hit[0]() is t and hit[1] == t._version:
        return hit[2]
    host = t.detach().cpu()
    if len(_host_copies) > 256:
        for k in [k for k, v in _host_copies.items() if v[0]() is None]:
            del _host_copies[k]
    _host_copies[key] = (weakref.ref(t), t._version, host)
    return host


class _Grids:
    """Solver grids for one (output times, step sizes) combination, resident on the device."""

    def __init__(self, t_host, step_size, adjoint_step_size, device):
        self.n_out = t_host.numel()
        self.time_dtype = t_host.dtype
        self.t_out = t_host.to(device)
        self.grid = _fixed_grid(t_host, step_size).to(device)
        # reversed-time grids, one per output interval, in processing order i = T-1 .. 1
        pieces, offsets = [], [0]
        for i in range(self.n_out - 1, 0, -1):
            seg_t = -(t_host[i - 1:i + 1].flip(0))     # torchdiffeq: t[i-1:i+1].flip(0) is decreasing -> solved on -t
            pieces.append(_fixed_grid(seg_t, adjoint_step_size))
            offsets.append(offsets[-1] + pieces[-1].numel())
        sgrid = torch.cat(pieces) if pieces else torch.zeros(0, dtype=t_host.dtype)
        self.n_sgrid = sgrid.numel()
        self.sgrid = sgrid.to(device)
        self.seg_off = torch.tensor(offsets, dtype=torch.int64).to(device)
        self.seg_off_host = offsets
        self.seg_off_c = (ctypes.c_int64 * len(offsets))(*offsets)      # host copy handed to the C ABI (wide shapes)
        self._t_host, self._step_size, self._device = t_host, step_size, device
        self._backprop = None

    def backprop_lists(self):
        """What the discrete backward (adjoint=False, cde_rk4_backprop_linear) needs besides the stored stages: the step
        sizes as the forward kernel rounds them, and per grid node the (output index, weight) pairs of torchdiffeq's linear
        output interpolation transposed (fixed-grid solvers: out = y0 + (t - t0) / (t1 - t0) * (y1 - y0), end points
        returned as they are) -- the same walk over (grid, t_out) the forward kernel makes."""
        if self._backprop is None:
            grid, t_out = _fixed_grid(self._t_host, self._step_size), self._t_host
            n_steps = grid.numel() - 1
            nodes = [[] for _ in range(n_steps + 1)]
            nodes[0].append((0, 1.0))
            jout = 1
            for k in range(n_steps):
                t0, t1 = grid[k], grid[k + 1]
                while jout < self.n_out and bool(t1 >= t_out[jout]):
                    tj = t_out[jout]
                    if bool(tj == t0):
                        nodes[k].append((jout, 1.0))
                    elif bool(tj == t1):
                        nodes[k + 1].append((jout, 1.0))
                    else:
                        slope = ((tj - t0) / (t1 - t0)).to(torch.float32)
                        nodes[k].append((jout, float(torch.ones((), dtype=torch.float32) - slope)))
                        nodes[k + 1].append((jout, float(slope)))
                    jout += 1
            ptr, outs, weights = [0], [], []
            for entries in nodes:
                outs += [j for j, _ in entries]
                weights += [w for _, w in entries]
                ptr.append(len(outs))
            dev = self._device
            self.backprop_nodes = nodes                    # host copy: the two-layer sweep runs in chunks that end on these nodes
            self._backprop = (
                (grid[1:] - grid[:-1]).to(torch.float32).to(dev) if n_steps > 0 else torch.zeros(1, dtype=torch.float32, device=dev),
                torch.tensor(ptr, dtype=torch.int64).to(dev), torch.tensor(outs, dtype=torch.int64).to(dev),
                torch.tensor(weights, dtype=torch.float32).to(dev), n_steps)
        return self._backprop


def _grids_for(t_host, step_size, adjoint_step_size, device):
    key = (t_host.numpy().tobytes(), str(t_host.dtype), step_size, adjoint_step_size, str(device))
    hit = _grid_cache.get(key)
    if hit is None:
        if len(_grid_cache) > 64:
            _grid_cache.clear()
        hit = _grid_cache[key] = _Grids(t_host, step_size, adjoint_step_size, device)
    return hit


def _field_values(act, weights, z):
    """F(z) of a fused field, (..., H * C): Linear(H, H * C) -- weights (W, b) -- or the two-layer Linear -> relu | softplus ->
    Linear -- weights (W1, b1, W2, b2) -- followed by the field's activation.  `act`: the field's `code` (final activation in
    bits 0-3, the two-layer field's hidden one in bits 4-7)."""
    if len(weights) == 4:
        z = torch.nn.functional.linear(z, weights[0], weights[1])
        z = torch.nn.functional.softplus(z) if (act >> 4) == _lib.HIDDEN_SOFTPLUS else z.relu()
    y = torch.nn.functional.linear(z, weights[-2], weights[-1])
    return y.tanh() if (act & 15) == _lib.ACT_TANH else y


def _abi_act(field):
    """The `int act` of the C ABI for a recognised field: its final activation, and in bits 4-7 the hidden activation of a
    two-layer field (include/cde_mi355x.h: CDE_FIELD_ACT; an affine field has none)."""
    return _lib.field_act(field.act, getattr(field, "hidden_act", _lib.HIDDEN_RELU))


def _weight_args(weights):
    """The weight arguments of the C ABI: (W, b) of the affine field, or (W1, b1, width, W2, b2) of the two-layer one."""
    if len(weights) == 2:
        return _lib.ptr(weights[0]), _lib.ptr(weights[1])
    w1, b1, w2, b2 = weights
    return _lib.ptr(w1), _lib.ptr(b1), w1.size(0), _lib.ptr(w2), _lib.ptr(b2)


def _time_gradients(plan, z_saved, grad_out, weights, grad_x, t, want_t, want_knots):
    """Gradients with respect to times from what the adjoint sweep already produced (torchdiffeq's odeint_adjoint,
    SURVEY appendix A.4, for f(t, z) = F(z) dX/dt(t)):
      dL/dt_i (i >= 1) = f(t_i, z_i) . dL/dz_i                       -- one field evaluation per output time
      dL/dt_0          = - sum_i dL/dt_i + int a^T F(z) d2X/dt2 dt    -- the integral in the solver's own quadrature
      dL/d knot_j      = - int_{interval j} a^T F(z) d2X/dt2 dt       -- the reference's `frac = t - t_j` chain
    With a cubic control d2X/dt2 = 2c + 2 (3d) frac, so both integrals are per-interval contractions of the control
    gradient the sweep accumulates anyway: sum_c (2c . dL/db + 2 (3d) . dL/d(2c)).  A piecewise-linear control has no
    such term; its slopes (x_{j+1} - x_j) / h_j depend on the knot times through the widths h_j instead
    (interpolation_linear.py:189): with G_j = dL/d(slope_j), dL/dh_j = -G_j . slope_j / h_j, and G_j / h_j is minus the
    running sum of the knot-value gradient the sweep produced (dL/dx_j = G_{j-1} / h_{j-1} - G_j / h_j telescopes)."""
    B, H, C = plan.B, plan.H, plan.C
    coeffs = plan.coeffs                                              # (B, rows, width)
    if plan.degree == _lib.PATH_CUBIC:
        per_interval = (coeffs[..., 2 * C:3 * C] * grad_x[..., C:2 * C]
                        + 2 * coeffs[..., 3 * C:] * grad_x[..., 2 * C:3 * C]).sum(-1).sum(0)      # (intervals,)
    else:
        per_interval = torch.zeros(coeffs.size(1) - 1, dtype=coeffs.dtype, device=plan.device)
    grad_t = grad_knots = None
    if want_t:
        zs = z_saved.reshape(B, plan.n_out, H)
        go = grad_out.reshape(B, plan.n_out, H)
        vals = [None] * plan.n_out
        total = torch.zeros((), dtype=coeffs.dtype, device=plan.device)
        for i in range(1, plan.n_out):
            y = _field_values(plan.act, weights, zs[:, i])
            dX = plan.path.derivative(plan.t_out[i]).reshape(B, C)
            vals[i] = ((y.view(B, H, C) * dX.unsqueeze(1)).sum(-1) * go[:, i]).sum()
            total = total + vals[i]
        vals[0] = per_interval.sum() - total
        # on `t`'s own device: cdeint accepts a CPU `t` next to GPU data (as the reference does)
        grad_t = torch.stack(vals).to(device=t.device, dtype=t.dtype) if plan.n_out > 1 else torch.zeros_like(t)
    if want_knots and plan.degree == _lib.PATH_CUBIC:
        grad_knots = torch.cat([-per_interval, per_interval.new_zeros(1)])
    elif want_knots:
        knots = plan.knots.double()
        values = coeffs.double()
        slopes = (values[:, 1:] - values[:, :-1]) / (knots[1:] - knots[:-1]).unsqueeze(-1)
        dh = (grad_x.double().cumsum(1)[:, :-1] * slopes).sum((0, 2))            # dL/dh_j
        zero = dh.new_zeros(1)
        grad_knots = (torch.cat([zero, dh]) - torch.cat([dh, zero])).to(coeffs.dtype)
    return grad_t, grad_knots


class _Plan:
    """Everything one cdeint call needs besides the differentiable tensors."""

    # bench.py sets `torchcde_amd.cdeint.event_log` (of its thread) to a list to receive ("forward" | "adjoint",
    # start_event, end_event) around the C-ABI calls, recorded on the stream the kernels are launched on.
    def _mark(self):
        if self.owner.event_log is None:
            return None
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        return ev

    def __init__(self, path, field, batch, H, C, t, step_size, adjoint_step_size, adjoint, variant, method=_lib.METHOD_RK4):
        self.owner = _state()
        self.method = method             # _lib.METHOD_*: rk4 (3/8 rule), or midpoint / euler on the same kernels
        coeffs, knots, _ = path._native_inputs()
        self.coeffs, self.knots = coeffs, knots
        self.path = path
        self.n_intervals = path._n_intervals()
        self.degree = path._degree
        self.act = field.act
        self.batch, self.B, self.H, self.C = batch, coeffs.size(0), H, C
        self.dtype = coeffs.dtype
        self.device = coeffs.device
        self.adjoint = adjoint
        self.variant = variant
        grids = _grids_for(_to_host(t), step_size, adjoint_step_size, self.device)
        self.grids = grids
        self.time_dtype, self.n_out = grids.time_dtype, grids.n_out
        self.t_out, self.grid = grids.t_out, grids.grid
        self.stage_index = None
        self.stage_frac = None

    time_gradients = _time_gradients

    def _log(self, kind, begin):
        if begin is not None:
            self.owner.event_log.append((kind, begin, self._mark()))

    def _parameter_gradients(self):
        """dL/dW and dL/db as two views of ONE flat buffer: a data-parallel caller can all-reduce that buffer in a single
        collective without gather/scatter copies (torchcde_amd.distributed.allreduce_gradients)."""
        n_w = self.H * self.C * self.H
        flat = torch.empty(n_w + self.H * self.C, dtype=self.dtype, device=self.device)
        return flat[:n_w].view(self.H * self.C, self.H), flat[n_w:]

    # forward: K2.  stages (adjoint=False): K2 also stores every stage state for the reverse-mode sweep (K3d), and
    # (out, stages) is returned
    def run_forward(self, z0, weight, bias, stages=False):
        lib = _lib.load()
        out = torch.empty(self.B, self.n_out, self.H, dtype=self.dtype, device=self.device)
        n_steps = max(self.grid.numel() - 1, 0)
        self.stage_index = torch.empty(max(4 * n_steps, 1), dtype=torch.int64, device=self.device)
        self.stage_frac = torch.empty(max(4 * n_steps, 1), dtype=self.dtype, device=self.device)
        z0c = z0.detach().reshape(self.B, self.H).contiguous()
        w = weight.detach().contiguous()
        b = bias.detach().contiguous()
        head = (_lib.ptr(self.coeffs), _lib.ptr(self.knots), self.n_intervals, self.degree, _lib.ptr(w), _lib.ptr(b))
        grid = (_lib.ptr(z0c), _lib.ptr(self.grid), self.grid.numel(), _lib.ptr(self.t_out), self.n_out, _lib.ptr(out))
        shape = (self.B, self.C, self.H, _lib.dtype_enum(self.dtype), _lib.dtype_enum(self.time_dtype))
        tail = (_lib.ptr(self.stage_index), _lib.ptr(self.stage_frac), _lib.stream_ptr(self.device))
        stages = torch.empty(self.B, max(n_steps, 1), 4, 32, dtype=torch.float32, device=self.device) if stages else None
        begin = self._mark()
        if stages is not None:
            _lib.check(lib.cde_rk4_forward_linear_stages(*head, self.act, *grid, _lib.ptr(stages), *shape, *tail),
                       "cde_rk4_forward_linear_stages")
        elif self.method != _lib.METHOD_RK4:
            _lib.check(lib.cde_fixed_forward_linear(self.method, *head, *grid, *shape, *tail), "cde_fixed_forward_linear")
        else:
            _lib.check(lib.cde_rk4_forward_linear(*head, self.act, *grid, *shape, self.variant, *tail),
                       "cde_rk4_forward_linear")
        self._log("forward", begin)
        return out if stages is None else (out, stages)

    def run_backprop(self, stages, grad_out, weight, bias, want_control=False):
        lib = _lib.load()
        step_dt, node_ptr, node_out, node_weight, n_steps = self.grids.backprop_lists()
        nbytes = lib.cde_rk4_backprop_workspace_bytes(self.B)
        workspace = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=self.device)
        grad_z0 = torch.empty(self.B, self.H, dtype=self.dtype, device=self.device)
        grad_w, grad_b = self._parameter_gradients()
        go = grad_out.detach().reshape(self.B, self.n_out, self.H).contiguous()
        w, b = weight.detach().contiguous(), bias.detach().contiguous()
        head = (_lib.ptr(self.coeffs), _lib.ptr(self.knots), self.n_intervals, self.degree, _lib.ptr(w), _lib.ptr(b),
                self.act, _lib.ptr(stages), _lib.ptr(go), self.n_out, _lib.ptr(step_dt), n_steps, _lib.ptr(node_ptr),
                _lib.ptr(node_out), _lib.ptr(node_weight), _lib.ptr(grad_z0), _lib.ptr(grad_w), _lib.ptr(grad_b))
        tail = (self.B, self.C, self.H, _lib.dtype_enum(self.dtype), _lib.ptr(self.stage_index), _lib.ptr(self.stage_frac),
                _lib.ptr(workspace), workspace.numel(), _lib.stream_ptr(self.device))
        begin = self._mark()
        grad_x = None
        if want_control:
            # the control's tensors require a gradient (autograd reaches them through X.derivative at every stage)
            grad_x = torch.zeros_like(self.coeffs)          # (B, rows, width) like the packed coefficients
            _lib.check(lib.cde_rk4_backprop_linear_dcontrol(*head, _lib.ptr(grad_x), *tail), "cde_rk4_backprop_linear_dcontrol")
        else:
            _lib.check(lib.cde_rk4_backprop_linear(*head, *tail), "cde_rk4_backprop_linear")
        self._log("backprop", begin)
        return grad_z0, grad_w, grad_b, grad_x

    # backward: K3
    def run_adjoint(self, z_saved, grad_out, weight, bias, want_control=False):
        lib = _lib.load()
        g = self.grids
        dt = _lib.dtype_enum(self.dtype)
        variant = _lib.VARIANT_MFMA if want_control else self.variant
        fixed = self.method != _lib.METHOD_RK4
        nbytes = (lib.cde_fixed_adjoint_workspace_bytes(self.B, g.n_sgrid) if fixed else
                  lib.cde_rk4_adjoint_workspace_bytes(self.B, self.C, self.H, g.n_sgrid, dt, variant))
        workspace = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=self.device)
        grad_z0 = torch.empty(self.B, self.H, dtype=self.dtype, device=self.device)
        grad_w, grad_b = self._parameter_gradients()
        zs = z_saved.detach().contiguous()
        go = grad_out.detach().reshape(self.B, self.n_out, self.H).contiguous()
        w, b = weight.detach().contiguous(), bias.detach().contiguous()
        head = (_lib.ptr(self.coeffs), _lib.ptr(self.knots), self.n_intervals, self.degree, _lib.ptr(w), _lib.ptr(b))
        sweep = (_lib.ptr(zs), _lib.ptr(go), _lib.ptr(g.sgrid), g.n_sgrid, _lib.ptr(g.seg_off))
        grads = (_lib.ptr(grad_z0), _lib.ptr(grad_w), _lib.ptr(grad_b))
        shape = (self.B, self.C, self.H, dt, _lib.dtype_enum(self.time_dtype))
        tail = (_lib.ptr(workspace), workspace.numel(), _lib.stream_ptr(self.device))
        begin = self._mark()
        grad_x = None
        if fixed:
            _lib.check(lib.cde_fixed_adjoint_linear(self.method, *head, *sweep, self.n_out, *grads, *shape, *tail),
                       "cde_fixed_adjoint_linear")
        elif want_control:
            grad_x = torch.zeros_like(self.coeffs)          # (B, rows, width) like the packed coefficients
            _lib.check(lib.cde_rk4_adjoint_linear_dcontrol(*head, self.act, *sweep, self.n_out, *grads, _lib.ptr(grad_x),
                                                           *shape, *tail), "cde_rk4_adjoint_linear_dcontrol")
        else:
            _lib.check(lib.cde_rk4_adjoint_linear(*head, self.act, *sweep, ctypes.cast(g.seg_off_c, ctypes.c_void_p),
                                                  self.n_out, *grads, *shape, self.variant, *tail), "cde_rk4_adjoint_linear")
        self._log("adjoint", begin)
        return grad_z0, grad_w, grad_b, grad_x


def _mlp_gradients(acc1, acc2, H, C, width):
    """(dL/dW1, dL/db1, dL/dW2, dL/db2) from the reduced images.  acc1: (128, >= 33), hidden units x (H inputs, bias in
    column 32).  acc2: (halves, 256, >= 129), rows = the padded (hidden unit, channel) layout of the G2 rows -- 32 units x 8
    channels, or 16 x 16 per half (two halves: hidden units 0..15 and 16..31) -- bias in column 128."""
    units, channels = (32, 8) if C <= 8 else (16, 16)
    w2 = acc2[:, :, :width].reshape(acc2.size(0) * units, channels, width)[:H, :C].reshape(H * C, width)
    b2 = acc2[:, :, 128].reshape(acc2.size(0) * units, channels)[:H, :C].reshape(H * C)
    return acc1[:width, :H].contiguous(), acc1[:width, 32].contiguous(), w2, b2


class _MlpPlan:
    """Fused RK4 solves for the two-layer field: forward (K2m, cde_rk4_forward_mlp) and continuous-adjoint backward
    (K3m sweep + two library GEMMs, cde_rk4_adjoint_mlp_*)."""

    scratch_budget = 3 << 30        # bytes of HBM the backward sweep may use for its per-stage factors

    def __init__(self, path, field, batch, H, C, t, step_size, adjoint_step_size=None):
        coeffs, knots, _ = path._native_inputs()
        self.coeffs, self.knots = coeffs, knots
        self.n_intervals, self.degree = path._n_intervals(), path._degree
        self.field, self.act, self.batch, self.B, self.H, self.C = field, _abi_act(field), batch, coeffs.size(0), H, C
        self.path = path
        self.device = coeffs.device
        self.grids = _grids_for(_to_host(t), step_size, step_size if adjoint_step_size is None else adjoint_step_size,
                                self.device)
        self.n_out, self.t_out = self.grids.n_out, self.grids.t_out

    def _weights(self, saved=None):
        f = self.field
        tensors = (f.hidden.weight, f.hidden.bias, f.output.weight, f.output.bias) if saved is None else saved
        return tuple(p.detach().contiguous() for p in tensors)

    # stages (adjoint=False): K2m also stores every stage state for K3m's sweep as reverse mode through the steps, and
    # (out, stages) is returned
    def run(self, z0, stages=False):
        lib = _lib.load()
        g = self.grids
        out = torch.empty(self.B, g.n_out, self.H, dtype=torch.float32, device=self.device)
        n_steps = max(g.grid.numel() - 1, 0)
        stage_index = torch.empty(max(4 * n_steps, 1), dtype=torch.int64, device=self.device)
        stage_frac = torch.empty(max(4 * n_steps, 1), dtype=torch.float32, device=self.device)
        z0c = z0.detach().reshape(self.B, self.H).contiguous()
        weights = self._weights()
        head = (_lib.ptr(self.coeffs), _lib.ptr(self.knots), self.n_intervals, self.degree, *_weight_args(weights), self.act,
                _lib.ptr(z0c), _lib.ptr(g.grid), g.grid.numel(), _lib.ptr(g.t_out), g.n_out, _lib.ptr(out))
        tail = (self.B, self.C, self.H, _lib.dtype_enum(torch.float32), _lib.dtype_enum(g.time_dtype), _lib.ptr(stage_index),
                _lib.ptr(stage_frac), _lib.stream_ptr(self.device))
        if stages:
            stages = torch.empty(self.B, max(n_steps, 1), 4, 32, dtype=torch.float32, device=self.device)
            _lib.check(lib.cde_rk4_forward_mlp_stages(*head, _lib.ptr(stages), *tail), "cde_rk4_forward_mlp_stages")
            return out.reshape(*self.batch, g.n_out, self.H), stages
        _lib.check(lib.cde_rk4_forward_mlp(*head, *tail), "cde_rk4_forward_mlp")
        return out.reshape(*self.batch, g.n_out, self.H)

    def _sweep_and_reduce(self, width, longest, sweeps):
        """The sweep's per-stage factor rows, reduced chunk by chunk into the parameter gradients by the split-K MFMA
        reduction (cde_mlp_grad_reduce; the bias gradients are the column sums of the same factors).  `sweeps(chunk, rows)`
        is a generator that launches the sweep over at most `chunk` steps at a time into rows = (U, G2, G1, Z) and yields
        the number of steps of each launch; `longest`: the most steps one launch can take (0: none)."""
        lib = _lib.load()
        B, dev = self.B, self.device
        upper = _mlp_upper_half(self.H, self.C)     # 32 units x 16 channels: the sweep leaves the upper unit groups' dL/dY2
        halves = 2 if upper else 1                  # rows BEHIND the lower groups' in G2 (rows n .. 2n - 1); each half is
        acc2 = torch.zeros(halves, 256, 132, dtype=torch.float32, device=dev)            # reduced into its own image
        acc1 = torch.zeros(128, 36, dtype=torch.float32, device=dev)
        if longest > 0:
            row_bytes = (132 + 256 * halves + 128 + 36) * 4
            chunk = max(1, min(longest, self.scratch_budget // (row_bytes * 4 * B)))
            rows = chunk * 4 * B
            U = torch.zeros(rows, 132, dtype=torch.float32, device=dev)
            U[:, 128] = 1
            Z = torch.zeros(rows, 36, dtype=torch.float32, device=dev)
            Z[:, 32] = 1
            G2 = torch.empty(halves * rows, 256, dtype=torch.float32, device=dev)
            G1 = torch.empty(rows, 128, dtype=torch.float32, device=dev)
            reduce_ws = torch.empty(lib.cde_mlp_grad_reduce_workspace_bytes(), dtype=torch.uint8, device=dev)
            stream = _lib.stream_ptr(dev)
            for steps in sweeps(chunk, (_lib.ptr(U), _lib.ptr(G2), _lib.ptr(G1), _lib.ptr(Z))):
                n = 4 * steps * B
                for half in range(halves):
                    _lib.check(lib.cde_mlp_grad_reduce(_lib.ptr(G2[half * n:]), _lib.ptr(U), n, 2, _lib.ptr(acc2[half]),
                                                       _lib.ptr(reduce_ws), reduce_ws.numel(), stream), "cde_mlp_grad_reduce")
                _lib.check(lib.cde_mlp_grad_reduce(_lib.ptr(G1), _lib.ptr(Z), n, 1, _lib.ptr(acc1), _lib.ptr(reduce_ws),
                                                   reduce_ws.numel(), stream), "cde_mlp_grad_reduce")
        return _mlp_gradients(acc1, acc2, self.H, self.C, width)

    def run_adjoint(self, z_saved, grad_out, w1, b1, w2, b2, want_control=False):
        """torchdiffeq's odeint_adjoint backward for this field: per output interval (last to first) the augmented
        state is integrated in reversed time by K3m in chunks of steps, each chunk's factors reduced into the parameter
        gradients (_sweep_and_reduce).
        The weights: the parameter tensors saved by the forward pass (an in-place update between forward and backward
        then trips autograd's version check instead of silently using the new values)."""
        lib = _lib.load()
        g = self.grids
        B, H, C = self.B, self.H, self.C
        dev, f32 = self.device, _lib.dtype_enum(torch.float32)
        weights = self._weights((w1, b1, w2, b2))
        nbytes = lib.cde_rk4_adjoint_mlp_workspace_bytes(g.n_sgrid)
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        stream = _lib.stream_ptr(dev)
        tdt = _lib.dtype_enum(g.time_dtype)
        z_saved = z_saved.detach().reshape(B, self.n_out, H)
        grad_out = grad_out.detach().reshape(B, self.n_out, H)
        # the sweep integrates (y, a) IN PLACE: private copies -- for a single series `[:, -1]` is already contiguous and
        # .contiguous() would hand the kernel the caller's own output / gradient tensors
        y = z_saved[:, -1].clone(memory_format=torch.contiguous_format)
        a = grad_out[:, -1].to(torch.float32).clone(memory_format=torch.contiguous_format)
        grad_x = torch.zeros_like(self.coeffs) if want_control else None     # accumulated by the sweep launches
        if g.n_sgrid > 1:
            _lib.check(lib.cde_rk4_adjoint_mlp_prepare(
                _lib.ptr(self.knots), self.n_intervals, _lib.ptr(g.sgrid), g.n_sgrid, *_weight_args(weights), C, H, f32, tdt,
                _lib.ptr(workspace), nbytes, stream), "cde_rk4_adjoint_mlp_prepare")

        def sweeps(chunk, rows):
            for p in range(self.n_out - 1):
                k, k_end = g.seg_off_host[p], g.seg_off_host[p + 1] - 1
                while k < k_end:
                    ke = min(k_end, k + chunk)
                    _lib.check(lib.cde_rk4_adjoint_mlp_sweep(
                        _lib.ptr(self.coeffs), _lib.ptr(self.knots), self.n_intervals, self.degree, self.act, _lib.ptr(y),
                        _lib.ptr(a), _lib.ptr(g.sgrid), g.n_sgrid, k, ke, *rows, _lib.ptr(grad_x), B, C, H, f32, tdt,
                        _lib.ptr(workspace), nbytes, stream), "cde_rk4_adjoint_mlp_sweep")
                    yield ke - k
                    k = ke
                i_out = self.n_out - 1 - p
                y.copy_(z_saved[:, i_out - 1])                 # torchdiffeq: re-seed z from the stored forward solution
                a.add_(grad_out[:, i_out - 1])                 # and add the incoming gradient at that output time
        longest = max((g.seg_off_host[p + 1] - 1 - g.seg_off_host[p] for p in range(self.n_out - 1)), default=0)
        grads = self._sweep_and_reduce(weights[0].size(0), longest if g.n_sgrid > 1 else 0, sweeps)
        return (a.reshape(*self.batch, H),) + grads + (grad_x,)

    def run_backprop(self, stages, grad_out, w1, b1, w2, b2, want_control=False):
        """Reverse mode through the 3/8-rule steps (the gradient `loss.backward()` through torchdiffeq's own operations
        gives, reference solver.py:144 with adjoint=False): the sweep walks the forward grid backwards in chunks of steps
        that end on the grid nodes an output gradient lands on (the transpose of torchdiffeq's linear output
        interpolation, `_Grids.backprop_lists`); each chunk's factor rows go through the same split-K reduction as the
        continuous adjoint's."""
        lib = _lib.load()
        g = self.grids
        B, H, C = self.B, self.H, self.C
        dev, f32 = self.device, _lib.dtype_enum(torch.float32)
        weights = self._weights((w1, b1, w2, b2))
        _, _, _, _, n_steps = g.backprop_lists()
        nodes = g.backprop_nodes
        n_grid = n_steps + 1
        go = grad_out.detach().reshape(B, self.n_out, H).to(torch.float32)
        gy = torch.zeros(B, H, dtype=torch.float32, device=dev)

        def land(m):                                                # output gradients that land on grid node m
            for j, wgt in nodes[m]:
                gy.add_(go[:, j], alpha=wgt)
        land(n_steps)                                               # (a single output time: node 0 is node n_steps)
        grad_x = torch.zeros_like(self.coeffs) if want_control else None     # accumulated by the sweep launches
        if n_steps > 0:
            stream = _lib.stream_ptr(dev)
            tdt = _lib.dtype_enum(g.time_dtype)
            nbytes = lib.cde_rk4_adjoint_mlp_workspace_bytes(n_grid)
            workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            _lib.check(lib.cde_rk4_backprop_mlp_prepare(
                _lib.ptr(self.knots), self.n_intervals, _lib.ptr(g.grid), n_grid, *_weight_args(weights), C, H, f32, tdt,
                _lib.ptr(workspace), nbytes, stream), "cde_rk4_backprop_mlp_prepare")

        def sweeps(chunk, rows):
            head = (_lib.ptr(self.coeffs), _lib.ptr(self.knots), self.n_intervals, self.degree, self.act, _lib.ptr(stages),
                    _lib.ptr(gy), _lib.ptr(g.grid), n_grid)
            tail = (B, C, H, f32, tdt, _lib.ptr(workspace), nbytes, stream)
            k_hi = n_steps
            while k_hi > 0:
                k_lo = max(0, k_hi - chunk)
                for m in range(k_hi - 1, k_lo, -1):                 # stop on the highest node below k_hi that receives a gradient
                    if nodes[m]:
                        k_lo = m
                        break
                if want_control:
                    _lib.check(lib.cde_rk4_backprop_mlp_sweep_dcontrol(*head, k_lo, k_hi, *rows, _lib.ptr(grad_x), *tail),
                               "cde_rk4_backprop_mlp_sweep_dcontrol")
                else:
                    _lib.check(lib.cde_rk4_backprop_mlp_sweep(*head, k_lo, k_hi, *rows, *tail), "cde_rk4_backprop_mlp_sweep")
                yield k_hi - k_lo
                land(k_lo)
                k_hi = k_lo
        grads = self._sweep_and_reduce(weights[0].size(0), n_steps, sweeps)
        return (gy.reshape(*self.batch, H),) + grads + (grad_x,)

    def time_gradients(self, z_saved, grad_out, weights, grad_x, t, want_t=True, want_knots=False):
        return _time_gradients(self, z_saved, grad_out, self._weights(weights), grad_x, t, want_t, want_knots)


def _mlp_upper_half(H, C):
    """32 hidden units x 16 channels (config 5 at hidden size 32: 14 logsignature channels): twice the 16 tiles -- the kernels
    read the upper unit groups straight from the output layer's tensors (csrc/cde_mfma.h: MlpHi)."""
    return 16 < H <= 32 and 8 < C <= 16


# which requests of the 32 x 16 shape the kernels take (the rest of that shape is solved step-wise)
# (the adaptive backward: one GPU's batch -- its shared-controller protocol exchanges one layer-2 image, not two)
_UPPER_HALF_PATHS = {"mlp_rk4_forward", "mlp_dopri5_forward", "mlp_rk4_adjoint", "mlp_rk4_backprop", "mlp_dopri5_adjoint"}


def _mlp_fusable(field, H, C, z0, packed):
    w1, w2 = field.hidden.weight, field.output.weight
    # tiles of the two-layer kernels: 32 hidden units x 8 channels, or 16 x 16 (cde_mi355x.h: cde_rk4_forward_mlp); 32 x 16 with
    # the upper half read from the raw tensors (16-byte rows: width a multiple of 4, an aligned contiguous weight)
    upper = (_mlp_upper_half(H, C) and w1.size(0) % 4 == 0 and w2.is_contiguous() and w2.data_ptr() % 16 == 0
             and field.output.bias.is_contiguous())
    return (z0.dtype == packed.dtype == w1.dtype == w2.dtype == torch.float32
            and ((H <= 32 and C <= 8) or (H <= 16 and C <= 16) or upper)
            and w1.size(0) <= 128 and tuple(w1.shape) == (w1.size(0), H) and tuple(w2.shape) == (H * C, w1.size(0)))


def _mlp3_fusable(field, H, C, z0, packed):
    """The envelope of the three-layer kernels (csrc/rk4_mlp3.hip; cde_mi355x.h: cde_rk4_forward_mlp3): float32, H <= 32,
    C <= 8, both hidden widths <= 128 -- one tile form, no 16-channel layout."""
    w1, wm, w2 = (lin.weight for lin in field.linears)
    return (z0.dtype == packed.dtype == w1.dtype == wm.dtype == w2.dtype == torch.float32 and H <= 32 and C <= 8
            and w1.size(0) <= 128 and wm.size(0) <= 128 and tuple(w1.shape) == (w1.size(0), H)
            and tuple(wm.shape) == (wm.size(0), w1.size(0)) and tuple(w2.shape) == (H * C, wm.size(0)))


class _Mlp3Plan(_MlpPlan):
    """Fused RK4 solves for the three-layer field: forward (K2m3, cde_rk4_forward_mlp3) and continuous-adjoint backward (K3m3
    sweep + three factor reductions, cde_rk4_adjoint_mlp3_*).  One wave per 16 series at every batch size."""

    def _weights(self, saved=None):
        tensors = tuple(p for lin in self.field.linears for p in (lin.weight, lin.bias)) if saved is None else saved
        return tuple(p.detach().contiguous() for p in tensors)

    @staticmethod
    def _weight_args(weights):
        """(W1, b1, width1, Wm, bm, width2, W2, b2) of the C ABI."""
        w1, b1, wm, bm, w2, b2 = weights
        return (_lib.ptr(w1), _lib.ptr(b1), w1.size(0), _lib.ptr(wm), _lib.ptr(bm), wm.size(0), _lib.ptr(w2), _lib.ptr(b2))

    def run(self, z0, stages=False):
        if stages:
            raise NotImplementedError("torchcde_amd: the three-layer field has no reverse-mode (adjoint=False) kernels")
        lib = _lib.load()
        g = self.grids
        out = torch.empty(self.B, g.n_out, self.H, dtype=torch.float32, device=self.device)
        n_steps = max(g.grid.numel() - 1, 0)
        stage_index = torch.empty(max(4 * n_steps, 1), dtype=torch.int64, device=self.device)
        stage_frac = torch.empty(max(4 * n_steps, 1), dtype=torch.float32, device=self.device)
        z0c = z0.detach().reshape(self.B, self.H).contiguous()
        weights = self._weights()
        _lib.check(lib.cde_rk4_forward_mlp3(
            _lib.ptr(self.coeffs), _lib.ptr(self.knots), self.n_intervals, self.degree, *self._weight_args(weights), self.act,
            _lib.ptr(z0c), _lib.ptr(g.grid), g.grid.numel(), _lib.ptr(g.t_out), g.n_out, _lib.ptr(out), self.B, self.C, self.H,
            _lib.dtype_enum(torch.float32), _lib.dtype_enum(g.time_dtype), _lib.ptr(stage_index), _lib.ptr(stage_frac),
            _lib.stream_ptr(self.device)), "cde_rk4_forward_mlp3")
        return out.reshape(*self.batch, g.n_out, self.H)

    def run_adjoint(self, z_saved, grad_out, w1, b1, wm, bm, w2, b2, want_control=False):
        """As _MlpPlan.run_adjoint, with the middle layer's factors: per chunk of steps the sweep streams (U, U1, G2, Gm, G1, Z)
        and three reductions follow -- G2^T U, Gm^T U1 (Gm padded to G2's 256 columns: the reduction's layer-2 form), G1^T Z."""
        if want_control:
            raise NotImplementedError("torchcde_amd: the three-layer sweep has no control gradients")
        lib = _lib.load()
        g = self.grids
        B, H, C = self.B, self.H, self.C
        dev, f32 = self.device, _lib.dtype_enum(torch.float32)
        weights = self._weights((w1, b1, wm, bm, w2, b2))
        width1, width2 = weights[0].size(0), weights[2].size(0)
        nbytes = lib.cde_rk4_adjoint_mlp3_workspace_bytes(g.n_sgrid)
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        stream = _lib.stream_ptr(dev)
        tdt = _lib.dtype_enum(g.time_dtype)
        z_saved = z_saved.detach().reshape(B, self.n_out, H)
        grad_out = grad_out.detach().reshape(B, self.n_out, H)
        # the sweep integrates (y, a) IN PLACE: private copies (see _MlpPlan.run_adjoint)
        y = z_saved[:, -1].clone(memory_format=torch.contiguous_format)
        a = grad_out[:, -1].to(torch.float32).clone(memory_format=torch.contiguous_format)
        acc2 = torch.zeros(256, 132, dtype=torch.float32, device=dev)
        accm = torch.zeros(256, 132, dtype=torch.float32, device=dev)
        acc1 = torch.zeros(128, 36, dtype=torch.float32, device=dev)
        longest = max((g.seg_off_host[p + 1] - 1 - g.seg_off_host[p] for p in range(self.n_out - 1)), default=0)
        if g.n_sgrid > 1 and longest > 0:
            _lib.check(lib.cde_rk4_adjoint_mlp3_prepare(
                _lib.ptr(self.knots), self.n_intervals, _lib.ptr(g.sgrid), g.n_sgrid, *self._weight_args(weights), C, H, f32,
                tdt, _lib.ptr(workspace), nbytes, stream), "cde_rk4_adjoint_mlp3_prepare")
            row_bytes = (132 + 132 + 256 + 256 + 128 + 36) * 4
            chunk = max(1, min(longest, self.scratch_budget // (row_bytes * 4 * B)))
            rows = chunk * 4 * B
            U, U1 = (torch.zeros(rows, 132, dtype=torch.float32, device=dev) for _ in range(2))
            U[:, 128] = 1
            U1[:, 128] = 1
            Z = torch.zeros(rows, 36, dtype=torch.float32, device=dev)
            Z[:, 32] = 1
            G2 = torch.empty(rows, 256, dtype=torch.float32, device=dev)
            Gm = torch.zeros(rows, 256, dtype=torch.float32, device=dev)      # the sweep writes columns 0..127 only
            G1 = torch.empty(rows, 128, dtype=torch.float32, device=dev)
            reduce_ws = torch.empty(lib.cde_mlp_grad_reduce_workspace_bytes(), dtype=torch.uint8, device=dev)
            for p in range(self.n_out - 1):
                k, k_end = g.seg_off_host[p], g.seg_off_host[p + 1] - 1
                while k < k_end:
                    ke = min(k_end, k + chunk)
                    _lib.check(lib.cde_rk4_adjoint_mlp3_sweep(
                        _lib.ptr(self.coeffs), _lib.ptr(self.knots), self.n_intervals, self.degree, self.act, _lib.ptr(y),
                        _lib.ptr(a), _lib.ptr(g.sgrid), g.n_sgrid, k, ke, _lib.ptr(U), _lib.ptr(U1), _lib.ptr(G2), _lib.ptr(Gm),
                        _lib.ptr(G1), _lib.ptr(Z), B, C, H, f32, tdt, _lib.ptr(workspace), nbytes, stream),
                        "cde_rk4_adjoint_mlp3_sweep")
                    n = 4 * (ke - k) * B
                    for G, X, layer, acc in ((G2, U, 2, acc2), (Gm, U1, 2, accm), (G1, Z, 1, acc1)):
                        _lib.check(lib.cde_mlp_grad_reduce(_lib.ptr(G), _lib.ptr(X), n, layer, _lib.ptr(acc), _lib.ptr(reduce_ws),
                                                           reduce_ws.numel(), stream), "cde_mlp_grad_reduce")
                    k = ke
                i_out = self.n_out - 1 - p
                y.copy_(z_saved[:, i_out - 1])                 # torchdiffeq: re-seed z from the stored forward solution
                a.add_(grad_out[:, i_out - 1])                 # and add the incoming gradient at that output time
        # real widths only: with softplus the padded hidden units hold softplus(0) = ln 2 in U and U1
        g_w1, g_b1 = _mlp_gradients(acc1, acc2[None], H, C, width1)[:2]
        g_w2, g_b2 = _mlp_gradients(acc1, acc2[None], H, C, width2)[2:]
        g_wm, g_bm = accm[:width2, :width1].contiguous(), accm[:width2, 128].contiguous()
        return (a.reshape(*self.batch, H), g_w1, g_b1, g_wm, g_bm, g_w2, g_b2, None)

    def run_backprop(self, *args, **kwargs):
        raise NotImplementedError("torchcde_amd: the three-layer field has no reverse-mode (adjoint=False) kernels")


def _mlp_wide_fusable(field, H, C, z0, packed):
    """The envelope of the wide-control kernels (csrc/rk4_mlp_tiled.hip, NV = 2; cde_mi355x.h: cde_rk4_forward_mlp_wide): float32,
    H <= 32, 16 < C <= 64, width <= 128 -- the channel counts beyond every tile form of _mlp_fusable (whose 32 x 16 upper-half
    form keeps the shapes it claims)."""
    w1, w2 = field.hidden.weight, field.output.weight
    return (z0.dtype == packed.dtype == w1.dtype == w2.dtype == torch.float32 and H <= 32 and 16 < C <= 64
            and w1.size(0) <= 128 and tuple(w1.shape) == (w1.size(0), H) and tuple(w2.shape) == (H * C, w1.size(0))
            and not _mlp_fusable(field, H, C, z0, packed))


def _mlp_wide_gradients(acc1, acc2, H, C, width):
    """(dL/dW1, dL/db1, dL/dW2, dL/db2) from the reduced images of the wide-control sweep.  acc1 as _mlp_gradients.  acc2:
    (blocks, 256, >= 129) -- block b holds rows 256 b .. 256 b + 255 of the padded layout (hidden unit h, channel c) ->
    h * CP + c, CP = C rounded up to 4; bias in column 128."""
    CP = (C + 3) // 4 * 4
    rows = acc2.reshape(acc2.size(0) * 256, acc2.size(2))[:H * CP].reshape(H, CP, acc2.size(2))[:, :C]
    return (acc1[:width, :H].contiguous(), acc1[:width, 32].contiguous(), rows[:, :, :width].reshape(H * C, width),
            rows[:, :, 128].reshape(H * C))


class _MlpTiledPlan(_MlpPlan):
    """Fused RK4 solves for the two-layer field with its output layer worked tile by tile (csrc/rk4_mlp_tiled.hip): forward
    (cde_rk4_forward_mlp_<form>) and continuous-adjoint backward (the sweep, cde_rk4_adjoint_mlp_<form>_*, + one factor
    reduction per 256-column block of the output layer's gradient and one per 32-unit half of the state).  One wave per 16
    series at every batch size.  A subclass names the form: the entry points' infix, the number of Z halves, the number of
    128-unit halves of the inner layer (U and G1 come in as many), and what the messages call the shape."""
    form = z_halves = shape_noun = sweep_noun = None
    inner_halves = 1

    def _entry(self, name):
        """(the entry point `name` with the form's infix, its name for messages)"""
        name = name % self.form
        return getattr(_lib.load(), name), name

    def run(self, z0, stages=False):
        if stages:
            raise NotImplementedError("torchcde_amd: %s have no reverse-mode (adjoint=False) kernels" % self.shape_noun)
        g = self.grids
        out = torch.empty(self.B, g.n_out, self.H, dtype=torch.float32, device=self.device)
        n_steps = max(g.grid.numel() - 1, 0)
        stage_index = torch.empty(max(4 * n_steps, 1), dtype=torch.int64, device=self.device)
        stage_frac = torch.empty(max(4 * n_steps, 1), dtype=torch.float32, device=self.device)
        z0c = z0.detach().reshape(self.B, self.H).contiguous()
        weights = self._weights()
        forward, name = self._entry("cde_rk4_forward_mlp_%s")
        _lib.check(forward(
            _lib.ptr(self.coeffs), _lib.ptr(self.knots), self.n_intervals, self.degree, *_weight_args(weights), self.act,
            _lib.ptr(z0c), _lib.ptr(g.grid), g.grid.numel(), _lib.ptr(g.t_out), g.n_out, _lib.ptr(out), self.B, self.C, self.H,
            _lib.dtype_enum(torch.float32), _lib.dtype_enum(g.time_dtype), _lib.ptr(stage_index), _lib.ptr(stage_frac),
            _lib.stream_ptr(self.device)), name)
        return out.reshape(*self.batch, g.n_out, self.H)

    def run_adjoint(self, z_saved, grad_out, w1, b1, w2, b2, want_control=False):
        """As _MlpPlan.run_adjoint, with the output layer's dL/dY2 rows in blocks of 256 columns and the state rows in halves
        of 32 units: per chunk of steps the sweep streams (U halves, G2 blocks, G1 halves, Z halves), each G2 block is reduced
        against every U half into its own image, every G1 half against every Z half."""
        if want_control:
            raise NotImplementedError("torchcde_amd: the %s sweep has no control gradients" % self.sweep_noun)
        lib = _lib.load()
        g = self.grids
        B, H, C = self.B, self.H, self.C
        dev, f32 = self.device, _lib.dtype_enum(torch.float32)
        weights = self._weights((w1, b1, w2, b2))
        width = weights[0].size(0)
        nbytes = self._entry("cde_rk4_adjoint_mlp_%s_workspace_bytes")[0](g.n_sgrid)
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        stream = _lib.stream_ptr(dev)
        tdt = _lib.dtype_enum(g.time_dtype)
        z_saved = z_saved.detach().reshape(B, self.n_out, H)
        grad_out = grad_out.detach().reshape(B, self.n_out, H)
        # the sweep integrates (y, a) IN PLACE: private copies (see _MlpPlan.run_adjoint)
        y = z_saved[:, -1].clone(memory_format=torch.contiguous_format)
        a = grad_out[:, -1].to(torch.float32).clone(memory_format=torch.contiguous_format)
        blocks = (H * ((C + 3) // 4 * 4) + 255) // 256
        inner = self.inner_halves
        acc2 = [torch.zeros(blocks, 256, 132, dtype=torch.float32, device=dev) for _ in range(inner)]
        acc1 = [[torch.zeros(128, 36, dtype=torch.float32, device=dev) for _ in range(self.z_halves)] for _ in range(inner)]
        longest = max((g.seg_off_host[p + 1] - 1 - g.seg_off_host[p] for p in range(self.n_out - 1)), default=0)
        self.steps_per_launch = 0                   # the chunking that ran (tests, tools)
        if g.n_sgrid > 1 and longest > 0:
            prepare, name = self._entry("cde_rk4_adjoint_mlp_%s_prepare")
            _lib.check(prepare(
                _lib.ptr(self.knots), self.n_intervals, _lib.ptr(g.sgrid), g.n_sgrid, *_weight_args(weights), C, H, f32, tdt,
                _lib.ptr(workspace), nbytes, stream), name)
            row_bytes = (inner * 132 + 256 * blocks + inner * 128 + self.z_halves * 36) * 4
            chunk = max(1, min(longest, self.scratch_budget // (row_bytes * 4 * B)))
            self.steps_per_launch = chunk
            rows = chunk * 4 * B
            U = []
            for _ in range(inner):
                U.append(torch.zeros(rows, 132, dtype=torch.float32, device=dev))
                U[-1][:, 128] = 1
            Z = []
            for _ in range(self.z_halves):          # (of the last half the sweep writes the units < H only)
                Z.append(torch.zeros(rows, 36, dtype=torch.float32, device=dev))
                Z[-1][:, 32] = 1
            G2 = torch.zeros(blocks * rows, 256, dtype=torch.float32, device=dev)    # the sweep writes the rows h < H only
            G1 = [torch.empty(rows, 128, dtype=torch.float32, device=dev) for _ in range(inner)]
            reduce_ws = torch.empty(lib.cde_mlp_grad_reduce_workspace_bytes(), dtype=torch.uint8, device=dev)
            sweep, name = self._entry("cde_rk4_adjoint_mlp_%s_sweep")
            for p in range(self.n_out - 1):
                k, k_end = g.seg_off_host[p], g.seg_off_host[p + 1] - 1
                while k < k_end:
                    ke = min(k_end, k + chunk)
                    _lib.check(sweep(
                        _lib.ptr(self.coeffs), _lib.ptr(self.knots), self.n_intervals, self.degree, self.act, _lib.ptr(y),
                        _lib.ptr(a), _lib.ptr(g.sgrid), g.n_sgrid, k, ke, *(_lib.ptr(half) for half in U), _lib.ptr(G2),
                        *(_lib.ptr(half) for half in G1), *(_lib.ptr(half) for half in Z), B, C, H, f32, tdt,
                        _lib.ptr(workspace), nbytes, stream), name)
                    n = 4 * (ke - k) * B
                    for s in range(inner):
                        for b in range(blocks):     # block b starts n rows behind block b - 1
                            _lib.check(lib.cde_mlp_grad_reduce(_lib.ptr(G2[b * n:]), _lib.ptr(U[s]), n, 2, _lib.ptr(acc2[s][b]),
                                                               _lib.ptr(reduce_ws), reduce_ws.numel(), stream),
                                       "cde_mlp_grad_reduce")
                        for half, acc in zip(Z, acc1[s]):
                            _lib.check(lib.cde_mlp_grad_reduce(_lib.ptr(G1[s]), _lib.ptr(half), n, 1, _lib.ptr(acc),
                                                               _lib.ptr(reduce_ws), reduce_ws.numel(), stream),
                                       "cde_mlp_grad_reduce")
                    k = ke
                i_out = self.n_out - 1 - p
                y.copy_(z_saved[:, i_out - 1])                 # torchdiffeq: re-seed z from the stored forward solution
                a.add_(grad_out[:, i_out - 1])                 # and add the incoming gradient at that output time
        if inner == 2:
            gradients = _mlp_broad_gradients(acc1[0][0], acc1[1][0], acc2[0], acc2[1], H, C, width)
        elif self.z_halves == 1:
            gradients = _mlp_wide_gradients(*acc1[0], acc2[0], H, C, width)
        else:
            gradients = _mlp_tall_gradients(*acc1[0], acc2[0], H, C, width)
        return (a.reshape(*self.batch, H),) + gradients + (None,)

    def run_backprop(self, *args, **kwargs):
        raise NotImplementedError("torchcde_amd: %s have no reverse-mode (adjoint=False) kernels" % self.shape_noun)


class _MlpWidePlan(_MlpTiledPlan):
    """The two-layer field on a control of 17 .. 64 channels (NV = 2: K2mc forward, K3mc sweep)."""
    form, z_halves, shape_noun, sweep_noun = "wide", 1, "wide controls", "wide-control"


def _mlp_tall_fusable(field, H, C, z0, packed):
    """The envelope of the tall-state kernels (csrc/rk4_mlp_tiled.hip, NV = 4; cde_mi355x.h: cde_rk4_forward_mlp_tall): float32,
    32 < H <= 64, C <= 64 with H * CP <= 2048 (CP = C rounded up to 4), width <= 128 -- the hidden sizes beyond every tile
    form of _mlp_fusable and _mlp_wide_fusable, which both stop at H = 32."""
    w1, w2 = field.hidden.weight, field.output.weight
    return (z0.dtype == packed.dtype == w1.dtype == w2.dtype == torch.float32 and 32 < H <= 64 and 1 <= C <= 64
            and H * ((C + 3) // 4 * 4) <= 2048 and w1.size(0) <= 128 and tuple(w1.shape) == (w1.size(0), H)
            and tuple(w2.shape) == (H * C, w1.size(0)))


def _mlp_tall_gradients(acc1, acc1_hi, acc2, H, C, width):
    """(dL/dW1, dL/db1, dL/dW2, dL/db2) from the reduced images of the tall-state sweep.  acc1 / acc1_hi: (128, 36) -- columns
    0 .. 31 of the first are dL/dW1[:, 0:32] and column 32 dL/db1, columns 0 .. H - 33 of the second dL/dW1[:, 32:H].  acc2 as
    _mlp_wide_gradients."""
    g_w1 = torch.cat((acc1[:width, :32], acc1_hi[:width, :H - 32]), dim=1).contiguous()
    return (g_w1, acc1[:width, 32].contiguous()) + _mlp_wide_gradients(acc1, acc2, H, C, width)[2:]


class _MlpTallPlan(_MlpTiledPlan):
    """The two-layer field on a hidden state of 33 .. 64 channels (NV = 4: K2mh forward, K3mh sweep; Z and Z_hi)."""
    form, z_halves, shape_noun, sweep_noun = "tall", 2, "tall hidden states", "tall-state"


def _mlp_broad_fusable(field, H, C, z0, packed):
    """The envelope of the broad-inner-layer kernels (csrc/rk4_mlp_broad.hip; cde_mi355x.h: cde_rk4_forward_mlp_broad): float32,
    128 < width <= 256, H <= 32, C <= 64 with H * CP <= 1024 (CP = C rounded up to 4) -- the inner widths beyond _mlp_fusable,
    _mlp_wide_fusable and _mlp_tall_fusable, which all stop at 128."""
    w1, w2 = field.hidden.weight, field.output.weight
    return (z0.dtype == packed.dtype == w1.dtype == w2.dtype == torch.float32 and 128 < w1.size(0) <= 256
            and 1 <= H <= 32 and 1 <= C <= 64 and H * ((C + 3) // 4 * 4) <= 1024
            and tuple(w1.shape) == (w1.size(0), H) and tuple(w2.shape) == (H * C, w1.size(0)))


def _mlp_broad_gradients(acc1_lo, acc1_hi, acc2_lo, acc2_hi, H, C, width):
    """(dL/dW1, dL/db1, dL/dW2, dL/db2) from the reduced images of the broad-inner-layer sweep.  acc1_lo / acc1_hi: (128, 36)
    -- rows 0 .. 127 and 128 .. width - 1 of dL/dW1 | dL/db1 (column 32).  acc2_lo / acc2_hi as _mlp_wide_gradients: columns
    0 .. 127 and 128 .. width - 1 of dL/dW2; dL/db2 in column 128 of the first."""
    lo = _mlp_wide_gradients(acc1_lo, acc2_lo, H, C, 128)
    hi = _mlp_wide_gradients(acc1_hi, acc2_hi, H, C, width - 128)
    return (torch.cat((lo[0], hi[0]), dim=0), torch.cat((lo[1], hi[1]), dim=0), torch.cat((lo[2], hi[2]), dim=1).contiguous(),
            lo[3])


class _MlpBroadPlan(_MlpTiledPlan):
    """The two-layer field with an inner layer of 129 .. 256 units (K2mb forward, K3mb sweep; U and G1 in two halves)."""
    form, z_halves, inner_halves, shape_noun, sweep_noun = "broad", 1, 2, "broad inner layers", "broad-inner-layer"


def _reaches(tensor, leaf):
    """Does the autograd graph of `tensor` reach the leaf `leaf`?  (The coefficient tensor of a control fitted with the same
    knot tensor the spline is evaluated on: test/test_tricks.py:21-49.)"""
    start = getattr(tensor, "grad_fn", None)
    if start is None:
        return False
    target = leaf.grad_fn                       # (a knot tensor that is itself computed: its own node is what the graph reaches)
    seen, stack = set(), [start]
    while stack:
        node = stack.pop()
        if node is None or node in seen:
            continue
        seen.add(node)
        if (target is not None and node is target) or (target is None and getattr(node, "variable", None) is leaf):
            return True
        stack.extend(fn for fn, _ in node.next_functions)
    return False


def _knot_fit_chain(X):
    """The path's buffers whose autograd graph reaches the knot tensor `X._t` (and that tensor), or None.
    torchdiffeq's adjoint differentiates the vector field w.r.t. every entry of adjoint_params with `torch.autograd.grad`
    (its `vjp_params`); for the knot tensor that derivative runs through EVERYTHING the field evaluation reads that was
    computed from it -- the spline's `frac = t - t_j`, and, when the coefficients were fitted with the same tensor
    (`natural_cubic_coeffs(x, t)` then `CubicSpline(coeffs, t)`, as the reference's test does), the fit as well.  The
    fused kernels form the first term; the second is one vector-Jacobian product of the fit with dL/dcoeffs (the block
    integrals are linear in it), added on the host (_with_fit_chain).  With the coefficient tensor in adjoint_params too
    the reference thus counts the fit's chain twice -- once inside the knot block, once when the returned dL/dcoeffs flows
    back through the fit -- and so does this path (the float64 oracle, built on autograd the same way, shows the same)."""
    if not (isinstance(X._t, torch.Tensor) and X._t.requires_grad):
        return None
    buffers = tuple(b for b in X._control_buffers() if _reaches(b, X._t))
    return (buffers, tuple(X._control_buffers()), X._t) if buffers else None


def _control_pieces(plan, grad_x):
    """dL/d(packed coefficients), (B, rows, width), as gradients of the path's buffer views: b, 2c, 3d of a cubic (its `a`
    rows are never read by the derivative), the knot values of a piecewise-linear control."""
    C = plan.C
    gx = grad_x.reshape(*plan.batch, grad_x.size(-2), grad_x.size(-1))
    pieces = (gx[..., C:2 * C], gx[..., 2 * C:3 * C], gx[..., 3 * C:]) if plan.degree == _lib.PATH_CUBIC else (gx,)
    return pieces


def _with_fit_chain(plan, grad_knots, grad_x):
    """dL/d(knot times) plus the fit's chain (see _knot_fit_chain); `grad_x`: dL/d(packed coefficients) of the sweep."""
    chain = getattr(plan, "fit_chain", None)
    if chain is None or grad_knots is None or grad_x is None:
        return grad_knots
    reaching, buffers, knots = chain
    pairs = [(b, g.to(b.dtype)) for b, g in zip(buffers, _control_pieces(plan, grad_x)) if any(b is r for r in reaching)]
    (extra,) = torch.autograd.grad([b for b, _ in pairs], [knots], [g.contiguous() for _, g in pairs], retain_graph=True,
                                   allow_unused=True)
    return grad_knots if extra is None else grad_knots + extra.to(device=grad_knots.device, dtype=grad_knots.dtype)


# ------------------------------------------------------------------------------------------ autograd glue
# Every fused Function takes (z0, *params, plan, wants, t, knots, *control): the field's parameters ((W, b), or the two-layer
# field's (W1, b1, W2, b2)); `wants`: which parameter gradients adjoint_params asks for (None: all); `t` / `knots`: the
# output times / the path's knot times when THEIR gradient is wanted (else None); `control`: the path's differentiable
# buffer views (cubic: b, 2c, 3d; linear: the knot values) when the gradient w.r.t. the coefficients is wanted -- only
# their gradient slots are used.  bench.py and the tests tell the protocols apart by the Functions' class names.
def _keep(ctx, plan, wants, t, knots, control, *saved):
    ctx.plan, ctx.wants, ctx.want_x, ctx.knots = plan, wants, len(control) > 0, knots
    ctx.save_for_backward(*saved, t)


def _gradients(ctx, grads, grad_t, grad_knots, grad_x):
    """The backward result of a fused Function: the sweep's (dL/dz0, *parameter gradients) masked by needs_input_grad and
    `wants`, dL/dt, dL/d knots plus the fit's chain (_with_fit_chain), dL/d the path's buffer views."""
    plan, need, wants = ctx.plan, ctx.needs_input_grad, ctx.wants
    grads = (grads[0].reshape(*plan.batch, plan.H),) + tuple(grads[1:])
    grads = tuple(g if need[i] and (i == 0 or wants is None or wants[i - 1]) else None for i, g in enumerate(grads))
    control = ()
    if ctx.want_x:
        control = tuple(g if n else None for g, n in zip(_control_pieces(plan, grad_x), need[len(grads) + 4:]))
    return grads + (None, None, grad_t, _with_fit_chain(plan, grad_knots, grad_x)) + control


@_once_differentiable
def _adjoint_backward(ctx, grad_out):
    """Fixed-grid solves: the continuous adjoint sweep, and the time gradients from the control-gradient sweep."""
    plan, need = ctx.plan, ctx.needs_input_grad
    z_saved, *weights, t = ctx.saved_tensors
    n = 1 + len(weights)
    want_t, want_knots = need[n + 2], need[n + 3]
    *grads, grad_x = plan.run_adjoint(z_saved, grad_out, *weights, want_control=ctx.want_x)
    grad_t = grad_knots = None
    if want_t or want_knots:
        # The time terms come out of the control-gradient sweep.  It is run IN ADDITION to the sweep above, so that dL/dz0
        # and the parameter gradients are bitwise the same whether or not a time requires grad (the reference's "detach
        # trick" invariance, test/test_tricks.py:111-131); requesting time gradients is rare.  (The two-layer field skips it
        # where the time terms do not read it: dL/dt alone of a piecewise-linear control.)
        if grad_x is None and (isinstance(plan, _Plan) or plan.degree == _lib.PATH_CUBIC or want_knots):
            grad_x = plan.run_adjoint(z_saved, grad_out, *weights, want_control=True)[-1]
        grad_t, grad_knots = plan.time_gradients(z_saved, grad_out, weights, grad_x, t, want_t, want_knots)
    return _gradients(ctx, grads, grad_t, grad_knots, grad_x)


@_once_differentiable
def _backprop_backward(ctx, grad_out):
    """adjoint=False: reverse mode through the stored stages; dL/d(packed coefficients) comes out of the same sweep, the
    knot times follow from it by the chain rule of `frac = t - t_j` / of the widths (plan.time_gradients)."""
    plan, need = ctx.plan, ctx.needs_input_grad
    stages, *weights, _ = ctx.saved_tensors
    want_knots = need[len(weights) + 4]
    *grads, grad_x = plan.run_backprop(stages, grad_out, *weights, want_control=ctx.want_x or want_knots)
    grad_knots = plan.time_gradients(None, None, weights, grad_x, None, False, True)[1] if want_knots else None
    return _gradients(ctx, grads, None, grad_knots, grad_x)


@_once_differentiable
def _dopri5_backward(ctx, grad_out):
    """The adaptive adjoint (K4a / K4am): dL/dt and the control gradients are blocks of its augmented state."""
    plan, need = ctx.plan, ctx.needs_input_grad
    z_saved, *weights, t = ctx.saved_tensors
    n = 1 + len(weights)
    want_t, want_knots = need[n + 2], need[n + 3]
    res = plan.run_adjoint(z_saved, grad_out, *weights, want_t=want_t, want_control=ctx.want_x, want_knots=want_knots)
    # on `t`'s own device: cdeint accepts a CPU `t` next to GPU data
    grad_t = res[n].to(device=t.device, dtype=t.dtype) if want_t else None
    grad_x = grad_knots = None
    if ctx.want_x:
        grad_x, grad_knots = res[-2], res[-1]
        if grad_knots is not None:
            grad_knots = grad_knots.to(device=ctx.knots.device, dtype=ctx.knots.dtype)
    return _gradients(ctx, res[:n], grad_t, grad_knots, grad_x)


class _FusedRK4(torch.autograd.Function):
    """Fixed-grid solve (rk4, midpoint, euler) of the affine field: K2 forward, continuous-adjoint K3 backward."""

    @staticmethod
    def forward(ctx, z0, weight, bias, plan, wants, t, knots, *control):
        out = plan.run_forward(z0, weight, bias)
        _keep(ctx, plan, wants, t, knots, control, out, weight, bias)
        return out.reshape(*plan.batch, plan.n_out, plan.H)

    @staticmethod
    def backward(ctx, grad_out):
        if not ctx.plan.adjoint:
            raise NotImplementedError(
                "torchcde_amd: backpropagating through the solver's internal operations (adjoint=False) is not "
                "implemented on the native path; use adjoint=True (continuous adjoint, the reference's default).")
        return _adjoint_backward(ctx, grad_out)


class _FusedMlpRK4(torch.autograd.Function):
    """The same for the two-layer field: K2m forward, K3m backward."""

    @staticmethod
    def forward(ctx, z0, w1, b1, w2, b2, plan, wants, t, knots, *control):
        out = plan.run(z0)
        _keep(ctx, plan, wants, t, knots, control, out, w1, b1, w2, b2)
        return out

    backward = staticmethod(_adjoint_backward)


class _FusedMlp3RK4(torch.autograd.Function):
    """The same for the three-layer field: K2m3 forward, K3m3 backward (six parameter inputs)."""

    @staticmethod
    def forward(ctx, z0, w1, b1, wm, bm, w2, b2, plan, wants, t, knots, *control):
        out = plan.run(z0)
        _keep(ctx, plan, wants, t, knots, control, out, w1, b1, wm, bm, w2, b2)
        return out

    backward = staticmethod(_adjoint_backward)


class _FusedMlpWideRK4(torch.autograd.Function):
    """The two-layer field on a control of 17 .. 64 channels: K2mc forward, K3mc backward."""

    @staticmethod
    def forward(ctx, z0, w1, b1, w2, b2, plan, wants, t, knots, *control):
        out = plan.run(z0)
        _keep(ctx, plan, wants, t, knots, control, out, w1, b1, w2, b2)
        return out

    backward = staticmethod(_adjoint_backward)


class _FusedMlpTallRK4(_FusedMlpWideRK4):
    """The two-layer field on a hidden state of 33 .. 64 channels: K2mh forward, K3mh backward."""


class _FusedMlpBroadRK4(_FusedMlpWideRK4):
    """The two-layer field with an inner layer of 129 .. 256 units: K2mb forward, K3mb backward."""


class _FusedRK4Backprop(torch.autograd.Function):
    """cdeint(..., method='rk4', adjoint=False) for the affine field: torchdiffeq.odeint under autograd (reference
    solver.py:226-227 with adjoint=False) -- the forward kernel stores the state handed to every field evaluation, the
    backward is reverse-mode differentiation of the 3/8-rule steps themselves (csrc/rk4_backprop.hip), i.e. the gradient
    of the discrete solve, as `loss.backward()` through torchdiffeq's own operations gives it.  (`knots` / `control`: with
    adjoint=False autograd reaches them through X.derivative at every stage.)"""

    @staticmethod
    def forward(ctx, z0, weight, bias, plan, wants, t, knots, *control):
        out, stages = plan.run_forward(z0, weight, bias, stages=True)
        _keep(ctx, plan, wants, t, knots, control, stages, weight, bias)
        return out.reshape(*plan.batch, plan.n_out, plan.H)

    backward = staticmethod(_backprop_backward)


class _FusedMlpRK4Backprop(torch.autograd.Function):
    """cdeint(..., method='rk4', adjoint=False) for the examples' two-layer field: as _FusedRK4Backprop, on K2m / K3m."""

    @staticmethod
    def forward(ctx, z0, w1, b1, w2, b2, plan, wants, t, knots, *control):
        out, stages = plan.run(z0, stages=True)
        _keep(ctx, plan, wants, t, knots, control, stages, w1, b1, w2, b2)
        return out

    backward = staticmethod(_backprop_backward)


# ------------------------------------------------------------------------------------------ dopri5 (K4)
last_dispatch = dispatch.last      # () -> (Choice(path, reason), Request) of this thread's most recent cdeint call
# Module attributes served from the calling thread's _CallState (see the module class at the end of this file):
#   last_dopri5_stats          {"n_accept", "n_reject", "launches"} of the most recent adaptive solve (tests / logging)
#   last_dopri5_adjoint_stats  the same for the most recent fused adaptive backward (summed over the output intervals)
#   record_dopri5_steps        tests: also fetch the accepted (t0, t1, on_jump) steps into last_dopri5_stats["steps"]
#   event_log                  bench.py: a list that receives the HIP events around the rk4 C-ABI calls
_DOPRI_CHUNK = 48          # attempt kernels queued between two looks at the done flag
_WORKSPACE_HEAD = 1 << 20  # bytes at the start of an adaptive workspace that hold the controller blocks and partial sums


def _status(workspace, at):
    """The controller status block at byte `at` of an adaptive workspace (one synchronising copy)."""
    size = ctypes.sizeof(_lib.DopriStatus)
    return _lib.DopriStatus.from_buffer_copy(workspace[at:at + size].cpu().numpy().tobytes())


_STEP_KEYS = ("first_step", "step_t", "min_step", "max_step")


class _StepOptions:
    """first_step / step_t / min_step / max_step of one dopri5 solve as torchdiffeq reads them (floats, 0-d tensors; step_t
    any 1-d tensor or sequence), popped from `options`.  `given` is false when none of them is set: the plans then call the
    entry points without them.  `block()` builds the host struct of the *_options entry points with fresh kernel state."""

    def __init__(self, options, jump_t, device, kept):
        """`kept`: the times a solve keeps (torchdiffeq drops those before its start) -- the check for a time shared by
        step_t and jump_t, or repeated in one of them, runs over these."""
        number = lambda v: float(v.item() if isinstance(v, torch.Tensor) else v)      # noqa: E731
        values = {key: options.pop(key, None) for key in _STEP_KEYS}
        self.given = any(v is not None for v in values.values())
        self.device = device
        self.first_step = float("nan") if values["first_step"] is None else number(values["first_step"])
        self.min_step = 0.0 if values["min_step"] is None else number(values["min_step"])
        self.max_step = float("inf") if values["max_step"] is None else number(values["max_step"])
        self.step_t = self.step_s = None
        self.n_step = 0
        if values["step_t"] is not None:
            # torchdiffeq reads the times as float64 (a list: exactly); a reversed-time solve negates `torch.as_tensor(step_t)`
            # first, which makes a list of floats a float32 tensor -- both are kept, each for the solve that sees it
            st = values["step_t"]
            raw = torch.sort(_to_host(torch.as_tensor(st)).reshape(-1)).values
            st = _to_host(st) if isinstance(st, torch.Tensor) else torch.as_tensor(st, dtype=torch.float64)
            st = torch.sort(st.to(torch.float64).reshape(-1)).values
            both = st if jump_t is None else torch.cat([st, _to_host(torch.as_tensor(jump_t)).to(torch.float64).reshape(-1)])
            if bool((both[kept(both)].unique(return_counts=True)[1] > 1).any()):
                raise ValueError("`step_t` and `jump_t` must not have any repeated elements between them.")
            self.n_step = st.numel()
            self.step_t = st.to(device)
            self.step_s = (-raw).flip(0).to(torch.float64).contiguous().to(device)       # the backward solve runs in s = -t
        if self.given and (not self.min_step >= 0.0 or not self.max_step >= self.min_step):
            raise ValueError("torchcde_amd: dopri5 needs 0 <= min_step <= max_step (got %r, %r)" % (self.min_step, self.max_step))

    def block(self, lib, reverse=False):
        state = torch.zeros(lib.cde_dopri5_step_state_bytes(), dtype=torch.uint8, device=self.device)
        times = self.step_s if reverse else self.step_t
        block = _lib.StepOptions(self.first_step, self.min_step, self.max_step, _lib.ptr(times), self.n_step, _lib.ptr(state))
        block.keep = (state, times)           # the device memory the struct points at lives as long as the struct
        return block


class _Dopri5Plan:
    def __init__(self, path, field, batch, H, C, t, rtol, atol, options, variant=_lib.VARIANT_AUTO,
                 adjoint_rtol=None, adjoint_atol=None, adjoint_options=None):
        self.owner = _state()
        self.record = self.owner.record
        self.variant = variant
        self.adjoint_rtol = float(rtol if adjoint_rtol is None else adjoint_rtol)
        self.adjoint_atol = float(atol if adjoint_atol is None else adjoint_atol)
        from .distributed import step_control
        self.shared = step_control()      # one controller across the shards of a distributed batch (or None)
        options = {} if options is None else dict(options)
        jump_t = options.pop("jump_t", None)
        self.safety = float(options.pop("safety", 0.9))
        self.ifactor = float(options.pop("ifactor", 10.0))
        self.dfactor = float(options.pop("dfactor", 0.2))
        t_first, t_last = float(_to_host(t)[0]), float(_to_host(t)[-1])
        self.steps = _StepOptions(options, jump_t, path._native_inputs()[0].device, lambda times: times >= t_first)
        self.adj_steps = self.steps           # adjoint_options=None: the forward options are the backward's
        if self.steps.given and self.shared is not None:
            raise NotImplementedError("torchcde_amd: first_step / step_t / min_step / max_step have no form under "
                                      "distributed.shared_step_control (one step controller across the shards)")
        for key in ("max_num_steps", "dtype", "norm"):
            if options.get(key, None) is not None:
                raise NotImplementedError("torchcde_amd: dopri5 option %r is not supported natively" % key)
            options.pop(key, None)
        if options:
            raise NotImplementedError("torchcde_amd: unsupported dopri5 options %s" % sorted(options))
        coeffs, knots, _ = path._native_inputs()
        self.coeffs, self.knots = coeffs, knots
        self.path = path
        self.n_intervals, self.degree, self.act = path._n_intervals(), path._degree, _abi_act(field)
        self.hidden = field.hidden if field.kind == "mlp2" else None      # two-layer field: its first Linear
        self.batch, self.B, self.H, self.C = batch, coeffs.size(0), H, C
        self.dtype, self.device = coeffs.dtype, coeffs.device
        self.rtol = float(rtol)
        self.atol = float(atol)
        t_host = _to_host(t).to(torch.float64)
        self.n_out = t_host.numel()
        self.t_host = t_host
        self.t_out = t_host.to(self.device)
        if jump_t is None:
            self.jump_t, self.n_jump, self.jump_s = None, 0, None
        else:
            jt = _to_host(torch.as_tensor(jump_t)).to(torch.float64).reshape(-1)
            jt = torch.sort(jt).values
            self.jump_t, self.n_jump = jt.to(self.device), jt.numel()
            self.jump_s = (-jt).flip(0).contiguous().to(self.device)      # the backward solve runs in s = -t
        self.n_jump_s = self.n_jump
        self.adj_safety, self.adj_ifactor, self.adj_dfactor = self.safety, self.ifactor, self.dfactor
        self.adj_norm_kind = 0      # torchdiffeq's default adjoint norm: mixed over (vjp_t, y, a, parameter gradients)
        if adjoint_options is not None:
            # torchdiffeq: explicit adjoint_options REPLACE the forward options for the backward solve (no jump_t unless
            # it is repeated there); norm: absent (the default mixed norm) or "seminorm" (without the parameter blocks)
            adj = dict(adjoint_options)
            self.adj_norm_kind = 1 if adj.pop("norm", None) == "seminorm" else 0
            jump_b = adj.pop("jump_t", None)
            self.adj_safety = float(adj.pop("safety", 0.9))
            self.adj_ifactor = float(adj.pop("ifactor", 10.0))
            self.adj_dfactor = float(adj.pop("dfactor", 0.2))
            # (every output interval keeps the times after its own start in reversed time: all of them, those up to t[-1])
            self.adj_steps = _StepOptions(adj, jump_b, self.device, lambda times: times <= t_last)
            if self.adj_steps.given and self.shared is not None:
                raise NotImplementedError("torchcde_amd: first_step / step_t / min_step / max_step have no form under "
                                          "distributed.shared_step_control (one step controller across the shards)")
            if jump_b is None:
                self.jump_s, self.n_jump_s = None, 0
            else:
                jb = torch.sort(_to_host(torch.as_tensor(jump_b)).to(torch.float64).reshape(-1)).values
                self.jump_s, self.n_jump_s = (-jb).flip(0).contiguous().to(self.device), jb.numel()

    def run(self, z0, weight, bias):
        """K4: the adaptive forward, `weight` / `bias` of the layer that produces the (H, C) matrix (of a two-layer field
        the second; the first is its `hidden` Linear).  _DOPRI_CHUNK attempts are queued between two looks at the status
        block; under one controller for all shards (torchcde_amd.distributed.shared_step_control) each attempt's pending
        error sums are all-reduced before the launch that consumes them."""
        lib = _lib.load()
        out = torch.empty(self.B, self.n_out, self.H, dtype=self.dtype, device=self.device)
        z0c = z0.detach().reshape(self.B, self.H).contiguous()
        if self.n_out == 1:
            out[:, 0] = z0c
            return out
        mlp = self.hidden is not None
        weights = ((self.hidden.weight, self.hidden.bias) if mlp else ()) + (weight, bias)
        weights = tuple(p.detach().contiguous() for p in weights)
        dt = _lib.dtype_enum(self.dtype)
        nbytes = lib.cde_dopri5_workspace_bytes(self.B, self.C, self.H, dt)
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        workspace[:_WORKSPACE_HEAD].zero_()     # controller blocks + partial sums (a sharded run all-reduces them from launch 0)
        variant = () if mlp else (self.variant,)
        suffix = "_mlp" if mlp else ""
        head = (_lib.ptr(self.coeffs), _lib.ptr(self.knots), self.n_intervals, self.degree, *_weight_args(weights), self.act,
                _lib.ptr(z0c), _lib.ptr(self.t_out), self.n_out, _lib.ptr(self.jump_t), self.n_jump, self.rtol, self.atol,
                self.safety, self.ifactor, self.dfactor, _lib.ptr(out), self.B, self.C, self.H, dt, *variant,
                _lib.ptr(workspace), workspace.numel())
        stream = _lib.stream_ptr(self.device)
        shared = self.shared
        steps = ()
        if shared is None:
            advance = "cde_dopri5_advance" + suffix
            if self.steps.given:
                block = self.steps.block(lib)
                advance, steps = advance + "_options", (ctypes.addressof(block),)
        else:
            reduce, global_batch = shared
            sums = torch.zeros(2, dtype=torch.float64, device=self.device)
            pending = "cde_dopri5_pending_sums" + suffix
            advance = "cde_dopri5_advance" + suffix + "_sharded"
            pending_head = (_lib.ptr(workspace), workspace.numel(), self.B, self.C, self.H, dt, *variant) + (() if mlp else (self.act,))
        launched = 0
        while True:
            if shared is None:
                _lib.check(getattr(lib, advance)(*head, launched, _DOPRI_CHUNK, *steps, stream), advance)
                launched += _DOPRI_CHUNK
            else:
                for _ in range(_DOPRI_CHUNK):
                    _lib.check(getattr(lib, pending)(*pending_head, launched, _lib.ptr(sums), stream), pending)
                    reduce(sums)
                    _lib.check(getattr(lib, advance)(*head, launched, _lib.ptr(sums), global_batch, stream), advance)
                    launched += 1
            status = _status(workspace, (launched & 1) * ctypes.sizeof(_lib.DopriStatus))   # one sync per chunk
            if status.phase == 4:
                break
            if launched > 2_000_000:
                raise RuntimeError("torchcde_amd: dopri5 did not reach t[-1] after %d attempted steps (t = %g, dt = %g)"
                                   % (launched, status.t_hi, status.dt))
        last_dopri5_stats = self.owner.dopri5            # (updated in place: callers may hold the dict itself)
        last_dopri5_stats.clear()
        last_dopri5_stats.update(n_accept=status.n_accept, n_reject=status.n_reject, launches=launched)
        if self.record:
            off = lib.cde_dopri5_trace_offset(self.B, self.C, self.H, dt)
            n = min(status.n_accept, 4096)            # CDE_DOPRI5_TRACE_STEPS
            last_dopri5_stats["steps"] = workspace[off:off + 24 * n].view(torch.float64).view(n, 3).cpu()
        return out

    def run_adjoint(self, z_saved, grad_out, *weights, want_t=False, want_control=False, want_knots=False):
        """torchdiffeq's odeint_adjoint backward for the adaptive solve -- default mixed norm (or "seminorm"), dense output at
        the interval ends -- output intervals from the last to the first.  `weights`: W, b of the affine field (K4a,
        csrc/dopri5_adjoint.hip: one attempt kernel + one reduction kernel per attempted step) or W1, b1, W2, b2 of the
        two-layer one (K4am, csrc/dopri5_mlp_adjoint.hip: per attempted step the attempt kernel, the split-K reduction of
        its gradient factors and the commit / norm kernel, queued by one C-ABI call).  Returns (dL/dz0, *parameter
        gradients[, dL/dt][, dL/dcoeffs, dL/d knots]).
        want_t: the output times require a gradient (torchdiffeq's time_vjps): dL/dt_i = f(t_i, z_i) . dL/dz_i for i >= 1
        (one batched field evaluation, here); vjp_t -- which the kernels integrate and measure in their error norm anyway --
        starts every interval at its carried value minus that term, and is dL/dt_0 after the last one.
        want_control: adjoint_params names the coefficient tensor (self.control_numel elements): dL/dcoeffs, packed layout,
        and (want_knots: the knot times are there too; else None) dL/d knots are appended to the result -- more blocks of
        the mixed norm, accumulated on the device (cde_dopri5_adjoint[_mlp]_advance_dcontrol)."""
        lib = _lib.load()
        B, H, C, dev = self.B, self.H, self.C, self.device
        mlp = len(weights) == 4
        prefix = "cde_dopri5_adjoint_mlp_" if mlp else "cde_dopri5_adjoint_"
        z_saved = z_saved.detach().reshape(B, self.n_out, H)
        grad_out = grad_out.detach().reshape(B, self.n_out, H).to(torch.float32)
        weights = tuple(p.detach().contiguous() for p in weights)
        if not mlp:
            n_w = H * C * H
            flat = torch.zeros(n_w + H * C, dtype=torch.float32, device=dev)       # one buffer: a single all-reduce upstream
            grads = (flat[:n_w].view(H * C, H), flat[n_w:])
        a = grad_out[:, -1].contiguous()
        grad_x = torch.zeros_like(self.coeffs) if want_control else None
        grad_k = torch.zeros_like(self.knots) if (want_control and want_knots) else None
        tail = (grad_x, grad_k) if want_control else ()
        if self.n_out == 1:
            zeros = tuple(torch.zeros_like(p) for p in weights) if mlp else grads
            return (a,) + zeros + ((torch.zeros(1, dtype=torch.float32, device=dev),) if want_t else ()) + tail
        if want_control and self.shared is not None:
            raise NotImplementedError("torchcde_amd: control gradients through the adaptive backward have no shared-controller form")
        nbytes = getattr(lib, prefix + ("dcontrol_workspace_bytes" if want_control else "workspace_bytes"))(B, C, H)
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        workspace[:_WORKSPACE_HEAD].zero_()     # controller blocks + partial sums: defined before the first launch reads them
        stride = lib.cde_dopri5_adjoint_status_stride()
        a_out = torch.empty(B, H, dtype=torch.float32, device=dev)
        shared = self.shared
        with_steps = self.adj_steps.given and shared is None
        reduced = None
        # "seminorm": the parameter blocks are not part of the decision -- only the 8 state sums travel between the shards
        state_only = shared is not None and self.adj_norm_kind == 1
        if shared is not None:
            reduced = torch.zeros(8 if state_only else getattr(lib, prefix + "reduced_count")(), dtype=torch.float64,
                                  device=dev)
        stream = _lib.stream_ptr(dev)
        stats = dict(n_accept=0, n_reject=0, launches=0)
        steps, attempts = [], []
        time_terms = [None] * self.n_out
        carry = None
        if want_t:
            off = getattr(lib, prefix + "carry_offset")(B, C, H)
            workspace[off:off + 256].zero_()                          # the whole carry block (the kernel leaves it alone: bit 1)
            carry = workspace[off:off + 8].view(torch.float64)        # vjp_t, carried across the intervals on the device
            # torchdiffeq: func_eval = func(t[i], y[i]); dLd_cur_t = func_eval . grad_y[i]; aug_state[0] -= dLd_cur_t -- the
            # field at ALL output times in one batched evaluation before the loop
            pre = _field_values(self.act, weights, z_saved[:, 1:])                          # (B, T - 1, H * C)
            dX = self.path.derivative(self.t_out[1:]).reshape(B, self.n_out - 1, C)
            terms = ((pre.view(B, self.n_out - 1, H, C) * dX.unsqueeze(2)).sum(-1) * grad_out[:, 1:]).sum((0, 2))
            if shared is not None:
                # one controller for all shards: vjp_t is a quantity of the WHOLE batch (it is in the error norm), so the
                # terms it starts every interval from are summed over the shards; every rank returns the global dL/dt
                terms64 = terms.to(torch.float64)
                shared[0](terms64)
                terms = terms64.to(torch.float32)
            for i in range(1, self.n_out):
                time_terms[i] = terms[i - 1]
        # the entry points: one attempt-chunk launch per look at the status block; under one controller for all shards
        # one attempt per launch, after which this shard's state sums (and, mixed norm, the S / E gradient images of the
        # attempt) are all-reduced and every shard commits / measures the parameter blocks on the same (global) numbers
        if shared is None:
            advance = prefix + ("advance_dcontrol" if want_control else "advance")
            extra = ((_lib.ptr(grad_x), int(self.control_numel), _lib.ptr(grad_k)) if want_control else
                     () if mlp else (None, 0))
            if with_steps:                     # (the *_options entry points are unsharded: no reduced sums to pass)
                advance += "_options"
                extra = extra if want_control else ()
        else:
            advance = prefix + ("advance_sharded" if mlp else "advance")        # (the affine entry point takes the sums)
            count = () if mlp else (1,)
            gather, apply = ("state_sums", "apply_state_sums") if state_only else ("pending_sums", "apply_reduced")
            gather, apply = prefix + gather, prefix + apply
            tolerances = () if state_only else (self.adjoint_rtol, self.adjoint_atol)
            ws_head = (_lib.ptr(workspace), workspace.numel(), B, C, H)
        if mlp:
            trace_offset = lambda which: lib.cde_dopri5_adjoint_mlp_trace_offset(B, C, H, which)         # noqa: E731
        else:
            trace_offset = lambda which: (lib.cde_dopri5_adjoint_trace_offset,                            # noqa: E731
                                          lib.cde_dopri5_adjoint_attempt_trace_offset)[which](B, C, H)
        w_args = _weight_args(weights)
        step_args = ()
        for i in range(self.n_out - 1, 0, -1):
            y = z_saved[:, i].contiguous()
            s0, s1 = -float(self.t_host[i]), -float(self.t_host[i - 1])
            if want_t:
                carry.copy_((carry.to(torch.float32) - time_terms[i]).to(torch.float64))
            head = (_lib.ptr(self.coeffs), _lib.ptr(self.knots), self.n_intervals, self.degree, *w_args, self.act, _lib.ptr(y),
                    _lib.ptr(a), s0, s1, _lib.ptr(self.jump_s), self.n_jump_s, self.adjoint_rtol, self.adjoint_atol,
                    self.adj_safety, self.adj_ifactor, self.adj_dfactor, self.adj_norm_kind, _lib.ptr(a_out), B, C, H,
                    _lib.dtype_enum(torch.float32), int(i == self.n_out - 1) | (2 if want_t else 0), _lib.ptr(workspace),
                    workspace.numel())
            if with_steps:                     # every output interval is a fresh solve: first_step and the step times restart
                block = self.adj_steps.block(lib, reverse=True)
                step_args = (ctypes.addressof(block),)
            launched = 0
            while True:
                if shared is None:
                    _lib.check(getattr(lib, advance)(*head, launched, _DOPRI_CHUNK, *extra, *step_args, stream), advance)
                    launched += _DOPRI_CHUNK
                else:
                    for _ in range(_DOPRI_CHUNK):
                        _lib.check(getattr(lib, advance)(*head, launched, *count, _lib.ptr(reduced) if launched else None,
                                                         shared[1], stream), advance)
                        launched += 1
                        _lib.check(getattr(lib, gather)(*ws_head, launched, _lib.ptr(reduced), stream), gather)
                        shared[0](reduced)
                        _lib.check(getattr(lib, apply)(*ws_head, *tolerances, launched, _lib.ptr(reduced), stream), apply)
                status = _status(workspace, (launched & 1) * stride)
                if status.phase == 4:
                    break
                if launched > 2_000_000:
                    raise RuntimeError("torchcde_amd: the dopri5 adjoint did not reach t = %g after %d attempted steps"
                                       % (-s1, launched))
            stats["n_accept"] += status.n_accept
            stats["n_reject"] += status.n_reject
            stats["launches"] += launched
            if self.record:
                off = trace_offset(0)
                n = min(status.n_accept, 4096)
                steps.append(workspace[off:off + 24 * n].view(torch.float64).view(n, 3).cpu())
                off = trace_offset(1)
                n = min(status.n_accept + status.n_reject, 16384)
                attempts.append(workspace[off:off + 40 * n].view(torch.float64).view(n, 5).cpu())
            a = a_out + grad_out[:, i - 1]
        if mlp:
            off = lib.cde_dopri5_adjoint_mlp_gradient_offset(B, C, H)
            totals = workspace[off:off + 4 * (256 * 129 + 128 * 33)].view(torch.float32)
            acc2, acc1 = totals[:256 * 129].view(1, 256, 129), totals[256 * 129:].view(128, 33)
            off = lib.cde_dopri5_adjoint_mlp_gradient_upper_offset(B, C, H)
            if off:                                                  # 32 units x 16 channels: hidden units 16..31, a second image
                acc2 = torch.cat([acc2, workspace[off:off + 4 * 256 * 129].view(torch.float32).view(1, 256, 129)])
            grads = _mlp_gradients(acc1, acc2, H, C, weights[0].size(0))
        else:
            _lib.check(lib.cde_dopri5_adjoint_finish(_lib.ptr(workspace), workspace.numel(), _lib.ptr(grads[0]),
                                                     _lib.ptr(grads[1]), B, C, H, int(shared is not None and not state_only),
                                                     stream), "cde_dopri5_adjoint_finish")
        last_dopri5_adjoint_stats = self.owner.dopri5_adjoint
        last_dopri5_adjoint_stats.clear()
        last_dopri5_adjoint_stats.update(stats)
        if self.record:
            last_dopri5_adjoint_stats["steps"] = steps           # one (n, 3) tensor per output interval, last first
            last_dopri5_adjoint_stats["attempts"] = attempts     # (t0, t1, on_jump, accepted, ratio) of EVERY attempt
        if want_t:
            time_terms[0] = carry.to(torch.float32).reshape(())       # time_vjps[0] = the carried vjp_t
            return (a,) + grads + (torch.stack(time_terms),) + tail
        return (a,) + grads + tail

    run_adjoint_mlp = run_adjoint     # (the two-layer field's weights W1, b1, W2, b2: the same driver)


class _FusedDopri5(torch.autograd.Function):
    """dopri5 forward (K4) and torchdiffeq's adaptive adjoint backward (K4a) of the affine field.  (`control` / `knots`:
    K4a then integrates dL/dcoeffs -- and dL/d knots -- as more blocks of the adjoint state.)"""

    @staticmethod
    def forward(ctx, z0, weight, bias, plan, wants, t, knots, *control):
        out = plan.run(z0, weight, bias)
        _keep(ctx, plan, wants, t, knots, control, out, weight, bias)
        return out.reshape(*plan.batch, plan.n_out, plan.H)

    backward = staticmethod(_dopri5_backward)


class _FusedMlpDopri5(torch.autograd.Function):
    """The reference examples' training call with their own model: cdeint(X, CDEFunc, z0, X.interval) -- dopri5 forward
    (K4 with the two-layer field) and torchdiffeq's adaptive adjoint backward (K4am)."""

    @staticmethod
    def forward(ctx, z0, w1, b1, w2, b2, plan, wants, t, knots, *control):
        out = plan.run(z0, w2, b2)
        _keep(ctx, plan, wants, t, knots, control, out, w1, b1, w2, b2)
        return out.reshape(*plan.batch, plan.n_out, plan.H)

    backward = staticmethod(_dopri5_backward)


# ------------------------------------------------------------------------------------------ front end
# ------------------------------------------------------------------------------------------ backend="torchsde"
_TORCHSDE_DT = 1e-3              # torchsde.sdeint's default step (from memory: DESIGN.md section 8 lists it as unchecked)
_TORCHSDE_KEYS = {"method", "dt", "adjoint_method", "adjoint_params", "rtol", "atol", "adjoint_rtol", "adjoint_atol",
                  "adaptive", "adjoint_adaptive", "options", "adjoint_options"}


def _parse_torchsde(kwargs, adjoint):
    """The keywords of cdeint(..., backend="torchsde") (reference solver.py:171-176, :228-230 forwards them to
    torchsde.sdeint[_adjoint]).  Returns (kwargs, revheun): method="reversible_heun" -> revheun = {dt, adjoint_params} for
    this package's reversible Heun solver; method="midpoint" -> revheun None and `kwargs` rewritten as the torchdiffeq
    request with the same step (the reference's own test equates the two, test/test_cdeint.py:49-63).  Anything else --
    Brownian motion, names, logqp, extra solver state, dt_min, adaptive stepping, another method -- raises
    NotImplementedError naming the key or method."""
    method = kwargs.get("method")
    if method not in ("reversible_heun", "midpoint"):
        raise NotImplementedError("torchcde_amd: backend='torchsde' is implemented for method='reversible_heun' and "
                                  "method='midpoint', not for method=%r." % (method,))
    unknown = sorted(set(kwargs) - _TORCHSDE_KEYS)
    if unknown:
        raise NotImplementedError("torchcde_amd: backend='torchsde' does not take the keyword argument(s) %s (accepted: %s)."
                                  % (", ".join(repr(k) for k in unknown), ", ".join(sorted(_TORCHSDE_KEYS))))
    for key in ("adaptive", "adjoint_adaptive"):
        if kwargs.get(key):
            raise NotImplementedError("torchcde_amd: backend='torchsde' takes fixed steps only: %s=%r is not implemented."
                                      % (key, kwargs[key]))
    for key in ("options", "adjoint_options"):
        if kwargs.get(key):
            raise NotImplementedError("torchcde_amd: backend='torchsde' takes no %s (got %r)." % (key, kwargs[key]))
    dt = kwargs.get("dt")
    dt = _TORCHSDE_DT if dt is None else dt
    adjoint_method = kwargs.get("adjoint_method")
    expected = "adjoint_reversible_heun" if method == "reversible_heun" else "midpoint"
    if adjoint_method not in (None, expected):
        raise NotImplementedError("torchcde_amd: backend='torchsde', method=%r is differentiated with adjoint_method=%r, "
                                  "not adjoint_method=%r." % (method, expected, adjoint_method))
    given = kwargs.get("adjoint_params")
    if method == "reversible_heun":
        return kwargs, {"dt": dt, "adjoint_params": None if given is None else tuple(given)}
    out = {k: kwargs[k] for k in ("rtol", "atol", "adjoint_rtol", "adjoint_atol", "adjoint_params") if k in kwargs}
    out.update(method="midpoint", options={"step_size": dt})
    if adjoint:
        out["adjoint_method"] = "midpoint"
    return out, None


def _no_time_gradient(t):
    if torch.is_grad_enabled() and isinstance(t, torch.Tensor) and t.requires_grad:
        raise NotImplementedError("torchcde_amd: method='reversible_heun' does not differentiate with respect to the times t.")


def _revheun_through(X, func, adjoint):
    """adjoint=False asks for the gradient autograd would find through the solver's steps: the reconstructing backward gives
    it for z0 and func's parameters; a control tensor that requires a gradient, or a func that is no module, is
    differentiated by autograd through the host-driven steps themselves."""
    if adjoint or not torch.is_grad_enabled():
        return False
    return not isinstance(func, torch.nn.Module) or any(b.requires_grad for b in X.buffers())


class _ReversibleHeunPlan(_Plan):
    """The fused reversible Heun solve: RHf forward, RHa backward (csrc/revheun.hip)."""

    def __init__(self, path, field, batch, H, C, t, dt, adjoint):
        super().__init__(path, field, batch, H, C, t, dt, None, adjoint, _lib.VARIANT_AUTO)

    def _head(self, weight, bias):
        w, b = weight.detach().contiguous(), bias.detach().contiguous()
        return (w, b), (_lib.ptr(self.coeffs), _lib.ptr(self.knots), self.n_intervals, self.degree, _lib.ptr(w), _lib.ptr(b),
                        self.act)

    def run_forward(self, z0, weight, bias):
        lib = _lib.load()
        n_grid = self.grid.numel()
        out = torch.empty(self.B, self.n_out, self.H, dtype=self.dtype, device=self.device)
        zhat = torch.empty(self.B, self.H, dtype=self.dtype, device=self.device)
        node_index = torch.empty(n_grid, dtype=torch.int64, device=self.device)
        node_frac = torch.empty(n_grid, dtype=self.dtype, device=self.device)
        z0c = z0.detach().reshape(self.B, self.H).contiguous()
        keep, head = self._head(weight, bias)
        begin = self._mark()
        _lib.check(lib.cde_revheun_forward_linear(
            *head, _lib.ptr(z0c), _lib.ptr(self.grid), n_grid, _lib.ptr(self.t_out), self.n_out, _lib.ptr(out), _lib.ptr(zhat),
            self.B, self.C, self.H, _lib.dtype_enum(self.dtype), _lib.dtype_enum(self.time_dtype), _lib.ptr(node_index),
            _lib.ptr(node_frac), _lib.stream_ptr(self.device)), "cde_revheun_forward_linear")
        self._log("forward", begin)
        return out, zhat

    def run_adjoint(self, y_final, zhat_final, grad_out, weight, bias):
        lib = _lib.load()
        _, node_ptr, node_out, node_weight, _ = self.grids.backprop_lists()
        n_grid = self.grid.numel()
        nbytes = lib.cde_revheun_adjoint_workspace_bytes(self.B, n_grid)
        workspace = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=self.device)
        grad_z0 = torch.empty(self.B, self.H, dtype=self.dtype, device=self.device)
        grad_w, grad_b = self._parameter_gradients()
        go = grad_out.detach().reshape(self.B, self.n_out, self.H).contiguous()
        keep, head = self._head(weight, bias)
        begin = self._mark()
        _lib.check(lib.cde_revheun_adjoint_linear(
            *head, _lib.ptr(y_final), _lib.ptr(zhat_final), _lib.ptr(go), _lib.ptr(self.grid), n_grid, _lib.ptr(node_ptr),
            _lib.ptr(node_out), _lib.ptr(node_weight), self.n_out, _lib.ptr(grad_z0), _lib.ptr(grad_w), _lib.ptr(grad_b),
            self.B, self.C, self.H, _lib.dtype_enum(self.dtype), _lib.dtype_enum(self.time_dtype), _lib.ptr(workspace),
            workspace.numel(), _lib.stream_ptr(self.device)), "cde_revheun_adjoint_linear")
        self._log("adjoint", begin)
        return grad_z0, grad_w, grad_b


class _FusedReversibleHeun(torch.autograd.Function):
    """cdeint(..., backend="torchsde", method="reversible_heun") for the affine field: the forward kernel keeps nothing but
    the final (y, zh); the backward kernel rebuilds the trajectory from them and returns the exact gradient of the discrete
    solve -- what adjoint=True (torchsde's adjoint_reversible_heun) and adjoint=False (autograd through the steps) both ask
    for, so both take this sweep."""

    @staticmethod
    def forward(ctx, z0, weight, bias, plan, wants):
        out, zhat = plan.run_forward(z0, weight, bias)
        ctx.plan, ctx.wants = plan, wants
        ctx.save_for_backward(out[:, -1].contiguous(), zhat, weight, bias)
        return out.reshape(*plan.batch, plan.n_out, plan.H)

    @staticmethod
    @_once_differentiable
    def backward(ctx, grad_out):
        plan, need, wants = ctx.plan, ctx.needs_input_grad, ctx.wants
        y_final, zhat, weight, bias = ctx.saved_tensors
        grad_z0, grad_w, grad_b = plan.run_adjoint(y_final, zhat, grad_out, weight, bias)
        return (grad_z0.reshape(*plan.batch, plan.H) if need[0] else None, grad_w if need[1] and wants[0] else None,
                grad_b if need[2] and wants[1] else None, None, None)


def _cdeint_reversible_heun(X, func, z0, t, adjoint, revheun, variant, field, recognised, recognised_kind, batch, H, C):
    """method="reversible_heun" once the compatibility probe has run: the fused plan when the probe found the affine field on
    the kernels' tiles, t is strictly increasing and nothing but z0, W, b wants a gradient; the step-wise solve otherwise."""
    _no_time_gradient(t)
    dt, given = revheun["dt"], revheun["adjoint_params"]
    grad_mode = torch.is_grad_enabled()
    t_is_vector = isinstance(t, torch.Tensor) and t.dim() == 1 and t.is_floating_point() and t.numel() >= 1
    t_host = _to_host(t) if t_is_vector else None
    increasing = t_is_vector and (t_host.numel() == 1 or bool((t_host[1:] > t_host[:-1]).all()))
    if not t_is_vector:
        raise ValueError("t must be a one dimensional floating point tensor.")
    control_wants = grad_mode and not adjoint and any(b.requires_grad for b in X.buffers())
    foreign = []
    if field is not None and adjoint and given is not None:
        foreign = [p for p in given if isinstance(p, torch.Tensor) and p.requires_grad
                   and p is not field.weight and p is not field.bias]
    if adjoint and given is None:
        for buffer in X.buffers():
            if buffer.requires_grad:
                warnings.warn(_GRAD_WARNING)
    reason = ""
    if field is None:
        reason = ("the vector field is not of a recognised form (arbitrary module)" if recognised_kind is None else
                  "reversible Heun is fused for the one-layer fields on the 32 x 8 tiles (float32, H <= 32, C <= 8)")
    elif not _lib.load().cde_revheun_supported(C, H, _lib.dtype_enum(z0.dtype), field.act):
        reason = "reversible Heun is fused for the one-layer fields on the 32 x 8 tiles (float32, H <= 32, C <= 8)"
    elif variant == _lib.VARIANT_GENERIC:
        reason = "variant='generic' was requested (the step-wise reference path)"
    elif not increasing:
        reason = "the output times are not strictly increasing"
    elif foreign:
        reason = "adjoint_params holds tensors other than the field's weight and bias"
    elif control_wants:
        reason = "adjoint=False with control tensors that require a gradient"
    params = given if (adjoint and given is not None) else (tuple(func.parameters()) if isinstance(func, torch.nn.Module) else ())
    wants_grad = grad_mode and (z0.requires_grad or control_wants
                                or any(isinstance(p, torch.Tensor) and p.requires_grad for p in params))
    request = dispatch.Request(
        prod=False, kind=recognised_kind, tiles_ok=field is not None, mfma_shape=field is not None and not reason,
        method="reversible_heun", adjoint=bool(adjoint), wants_grad=bool(wants_grad), wants_t=False,
        wants_control=bool(control_wants or foreign), params="default" if given is None else
        ("foreign" if foreign else "own"), adjoint_method_ok=True, options_ok=True, adjoint_options_ok=True,
        t_ok=bool(increasing), variant_generic=variant == _lib.VARIANT_GENERIC, shared=False, narrow_control=C <= 8,
        backprop_ok=field is not None and not reason, identity=bool(field is not None and field.act == _lib.ACT_NONE),
        control_block=False)
    choice = dispatch.Choice(dispatch.TORCHSDE_PATHS[1] if reason else dispatch.TORCHSDE_PATHS[0], reason)
    dispatch.record(choice, request)
    if reason:
        from . import stepwise
        dispatch.warn_once(func, choice, request)
        return stepwise.solve_reversible_heun(X, func, z0, t, dt, adjoint, given, recognised=recognised,
                                              through=_revheun_through(X, func, adjoint))
    weight, bias = field.weight, field.bias
    plan = _ReversibleHeunPlan(X, field, batch, H, C, t, dt, adjoint)
    if not wants_grad:
        with torch.no_grad():
            return plan.run_forward(z0, weight, bias)[0].reshape(*batch, plan.n_out, H)
    wants = (True, True)
    if adjoint and given is not None:
        wants = (any(p is weight for p in given), any(p is bias for p in given))
    return _FusedReversibleHeun.apply(z0, weight, bias, plan, wants)


def _shape_errors(dX_shape, system_shape, z0):
    # messages of reference solver.py:7-33
    if tuple(dX_shape[:-1]) != tuple(z0.shape[:-1]):
        raise ValueError("X.derivative did not return a tensor with the same number of batch dimensions as z0. "
                         "X.derivative returned shape {} (meaning {} batch dimensions), whilst z0 has shape {} "
                         "(meaning {} batch dimensions)."
                         "".format(tuple(dX_shape), tuple(dX_shape[:-1]), tuple(z0.shape), tuple(z0.shape[:-1])))
    if tuple(system_shape[:-2]) != tuple(z0.shape[:-1]):
        raise ValueError("func did not return a tensor with the same number of batch dimensions as z0. func returned "
                         "shape {} (meaning {} batch dimensions), whilst z0 has shape {} (meaning {} batch"
                         " dimensions)."
                         "".format(tuple(system_shape), tuple(system_shape[:-2]), tuple(z0.shape),
                                   tuple(z0.shape[:-1])))
    if system_shape[-2] != z0.size(-1):
        raise ValueError("func did not return a tensor with the same number of hidden channels as z0. func returned "
                         "shape {} (meaning {} channels), whilst z0 has shape {} (meaning {} channels)."
                         "".format(tuple(system_shape), system_shape[-2], tuple(z0.shape), z0.size(-1)))
    if system_shape[-1] != dX_shape[-1]:
        raise ValueError("func did not return a tensor with the same number of input channels as X.derivative "
                         "returned. func returned shape {} (meaning {} channels), whilst X.derivative returned shape "
                         "{} (meaning {} channels)."
                         "".format(tuple(system_shape), system_shape[-1], tuple(dX_shape), dX_shape[-1]))


def _cdeint_tuple(X, func, z0, t, adjoint, backend, kwargs):
    """Tuple-valued state (reference solver.py:68-95): checks and messages as the reference, then the step-wise solver
    on the concatenated state (what torchdiffeq does with tuples); returns a tuple of (..., len(t), H_i) tensors."""
    revheun = None
    if backend == "torchsde":
        kwargs, revheun = _parse_torchsde(kwargs, adjoint)
    elif backend != "torchdiffeq":
        raise ValueError(f"Unrecognised backend={backend}")
    for part in z0:
        if not isinstance(part, torch.Tensor):
            raise ValueError("z0 must either a tensor or a tuple/list of tensors.")
        _lib.require_gpu(part, "z0")
    probe_t = t[0].to(z0[0].device) if isinstance(t, torch.Tensor) else t
    with torch.no_grad():
        dX = X.derivative(probe_t)
        if not isinstance(dX, (tuple, list)):
            raise ValueError("z0 is a tuple/list and so X.derivative must return a tuple/list as well.")
        if len(z0) != len(dX):
            raise ValueError("z0 and X.derivative(t) must be tuples of the same length.")
        is_prod = hasattr(func, "prod")
        system = func.prod(probe_t, z0, dX) if is_prod else func(probe_t, z0)
    name = "func.prod" if is_prod else "func"
    if not isinstance(system, (tuple, list)):
        raise ValueError("z0 is a tuple/list and so %s must return a tuple/list as well." % name)
    if len(z0) != len(system):
        raise ValueError("z0 and %s must be tuples of the same length."
                         % ("func.prod(t, z, dXdt)" if is_prod else "func(t, z)"))
    for dX_i, system_i, z_i in zip(dX, system, z0):
        if not isinstance(dX_i, torch.Tensor):
            raise ValueError("X.derivative must return a tensor or tuple of tensors.")
        if not isinstance(system_i, torch.Tensor):
            raise ValueError("%s must return a tensor or tuple/list of tensors." % name)
        if is_prod:
            if tuple(dX_i.shape[:-1]) != tuple(z_i.shape[:-1]):
                _shape_errors(tuple(dX_i.shape), tuple(z_i.shape) + (dX_i.size(-1),), z_i)
            if system_i.shape != z_i.shape:
                raise ValueError("func.prod did not return a tensor with the same shape as z0. func.prod returned shape "
                                 "{} whilst z0 has shape {}.".format(tuple(system_i.shape), tuple(z_i.shape)))
        else:
            _shape_errors(tuple(dX_i.shape), tuple(system_i.shape), z_i)
    from . import stepwise
    kw = dict(kwargs)
    kw.pop("variant", None)
    kw.setdefault("atol", 1e-6)
    kw.setdefault("rtol", 1e-4)
    if adjoint:
        kw.setdefault("adjoint_atol", kw["atol"])
        kw.setdefault("adjoint_rtol", kw["rtol"])
    sizes = [part.size(-1) for part in z0]
    field = stepwise.TupleField(X, func, sizes)
    if revheun is not None:
        _no_time_gradient(t)
        dispatch.record(dispatch.Choice(dispatch.TORCHSDE_PATHS[1], "tuple-valued state"), None)
        out = stepwise.solve_reversible_heun(X, func, torch.cat(z0, dim=-1), t, revheun["dt"], adjoint,
                                             revheun["adjoint_params"], field=field,
                                             through=not adjoint and torch.is_grad_enabled())
        return tuple(out.split(sizes, dim=-1))
    out = stepwise.solve(X, func, torch.cat(z0, dim=-1), t, adjoint, kw.get("method") or "dopri5", kw.get("options"),
                         kw["rtol"], kw["atol"], kw.get("adjoint_method"), kw.get("adjoint_options"),
                         kw.get("adjoint_rtol"), kw.get("adjoint_atol"), kw.get("adjoint_params"), field=field)
    return tuple(out.split(sizes, dim=-1))


def _cdeint_foreign_control(X, func, z0, t, adjoint, kwargs, revheun=None):
    """A control that is not one of this package's paths (reference solver.py:45-46: anything with a `derivative` method,
    typically an nn.Module of the user's): the reference's compatibility checks and messages (solver.py:44-67), then the
    step-wise solver -- X.derivative(t) is called as it is (under autograd when its parameters or the times need a
    gradient), the vector field times dX/dt runs in cde_contract."""
    _lib.require_gpu(z0, "z0")
    probe_t = t[0].to(z0.device) if isinstance(t, torch.Tensor) else t
    is_prod = hasattr(func, "prod")
    with torch.no_grad():
        dX = X.derivative(probe_t.detach() if isinstance(probe_t, torch.Tensor) else probe_t)
        system = func.prod(probe_t, z0, dX) if is_prod else func(probe_t, z0)
    if not isinstance(dX, torch.Tensor):
        raise ValueError("z0 is a tensor and so X.derivative must return a tensor as well.")
    if is_prod:
        if not isinstance(system, torch.Tensor):
            raise ValueError("z0 is a tensor and so func.prod must return a tensor as well.")
        if tuple(dX.shape[:-1]) != tuple(z0.shape[:-1]):
            _shape_errors(tuple(dX.shape), tuple(z0.shape) + (dX.size(-1),), z0)
        if system.shape != z0.shape:
            raise ValueError("func.prod did not return a tensor with the same shape as z0. func.prod returned shape {} "
                             "whilst z0 has shape {}.".format(tuple(system.shape), tuple(z0.shape)))
    else:
        if not isinstance(system, torch.Tensor):
            raise ValueError("z0 is a tensor and so func must return a tensor as well.")
        _shape_errors(tuple(dX.shape), tuple(system.shape), z0)
    _lib.require_gpu(dX, "X.derivative(t)")
    buffers = tuple(X.buffers()) if isinstance(X, torch.nn.Module) else ()
    if adjoint and "adjoint_params" not in kwargs:
        for buffer in buffers:
            if buffer.requires_grad:
                warnings.warn(_GRAD_WARNING)
    from . import stepwise
    field = stepwise.ForeignControlField(X, func)
    if revheun is not None:
        _no_time_gradient(t)
        dispatch.record(dispatch.Choice(dispatch.TORCHSDE_PATHS[1], "the control is not one of this package's paths: "
                                                                    "X.derivative is called at every evaluation"), None)
        return stepwise.solve_reversible_heun(X, func, z0, t, revheun["dt"], adjoint, revheun["adjoint_params"], field=field,
                                              through=not adjoint and torch.is_grad_enabled())
    dispatch.record(dispatch.Choice(dispatch.STEPWISE, "the control is not one of this package's paths: X.derivative is "
                                                       "called at every evaluation"), None)
    kw = dict(kwargs)
    return stepwise.solve(X, func, z0, t, adjoint, kw.pop("method", None) or "dopri5", kw.pop("options", None),
                          kw["rtol"], kw["atol"], kw.get("adjoint_method"), kw.get("adjoint_options"),
                          kw.get("adjoint_rtol"), kw.get("adjoint_atol"), kw.get("adjoint_params"), field=field)


def cdeint(X, func, z0, t, adjoint=True, backend="torchdiffeq", **kwargs):
    r"""Solve  z_t = z_{t_0} + \int_{t_0}^t f(s, z_s) dX_s  on the MI355X.

    Arguments, return value (shape ``(..., len(t), hidden_channels)``) and errors as reference
    ``torchcde.cdeint`` (solver.py:144-194).  ``variant=`` (extra keyword, one of
    "auto" | "generic" | "mfma" | "split" | "bf16x3") selects the kernel family: "bf16x3" runs the rk4 solve's weight
    GEMMs on the bf16 matrix pipe at float32 accuracy (csrc/rk4_bf16x3.hip), the others exist for testing."""
    variant = {"auto": _lib.VARIANT_AUTO, "generic": _lib.VARIANT_GENERIC, "mfma": _lib.VARIANT_MFMA,
               "split": _lib.VARIANT_SPLIT, "bf16x3": _lib.VARIANT_BF16X3}[kwargs.pop("variant", "auto")]
    # tolerance defaults of solver.py:195-203 (only adaptive methods read them)
    kwargs.setdefault("atol", 1e-6)
    kwargs.setdefault("rtol", 1e-4)
    if adjoint:
        kwargs.setdefault("adjoint_atol", kwargs["atol"])
        kwargs.setdefault("adjoint_rtol", kwargs["rtol"])

    if not hasattr(X, "derivative"):
        raise ValueError("X must have a 'derivative' method.")
    if isinstance(z0, (tuple, list)):
        return _cdeint_tuple(X, func, tuple(z0), t, adjoint, backend, kwargs)
    if not isinstance(z0, torch.Tensor):
        raise ValueError("z0 must either a tensor or a tuple/list of tensors.")
    revheun = None
    if backend == "torchsde":
        # method="reversible_heun": this package's own solver (csrc/revheun.hip, stepwise.solve_reversible_heun);
        # method="midpoint": the torchdiffeq request with the same step, which the code below then serves
        kwargs, revheun = _parse_torchsde(kwargs, adjoint)
    elif backend != "torchdiffeq":
        raise ValueError(f"Unrecognised backend={backend}")
    if not isinstance(X, _NativePath):
        # solver.py:45-46 asks X for nothing but a `derivative` method: a user-defined control is solved step by step on the
        # GPU with X.derivative(t) itself under every evaluation (cde_contract for the matrix-vector product)
        return _cdeint_foreign_control(X, func, z0, t, adjoint, kwargs, revheun)
    stepwise_kwargs = dict(kwargs)      # what the step-wise path would receive (the reference forwards these verbatim)
    _lib.require_gpu(z0, "z0")
    packed = X._packed()
    _lib.require_gpu(packed, "the control path")
    batch = tuple(packed.shape[:-2])
    C = X._channels()
    H = z0.size(-1)
    if hasattr(func, "prod"):
        # solver.py:48-53, :35-41, :121-123: the module computes f(t, z) dX itself; solved step by step with the native
        # control derivative under every evaluation
        if batch != tuple(z0.shape[:-1]):
            _shape_errors(batch + (C,), tuple(z0.shape) + (C,), z0)
        with torch.no_grad():
            probe_t = t[0].to(z0.device) if isinstance(t, torch.Tensor) else t
            first = func.prod(probe_t, z0, X.derivative(probe_t))
        if not isinstance(first, torch.Tensor):
            raise ValueError("z0 is a tensor and so func.prod must return a tensor as well.")
        if first.shape != z0.shape:
            raise ValueError("func.prod did not return a tensor with the same shape as z0. func.prod returned shape {} "
                             "whilst z0 has shape {}.".format(tuple(first.shape), tuple(z0.shape)))
        from . import stepwise
        if revheun is not None:
            _no_time_gradient(t)
            dispatch.record(dispatch.Choice(dispatch.TORCHSDE_PATHS[1], "func.prod multiplies by the control derivative "
                                                                        "itself"), None)
            return stepwise.solve_reversible_heun(X, func, z0, t, revheun["dt"], adjoint, revheun["adjoint_params"],
                                                  through=_revheun_through(X, func, adjoint))
        dispatch.record(dispatch.Choice(dispatch.STEPWISE, "func.prod multiplies by the control derivative itself"), None)
        kw = stepwise_kwargs
        return stepwise.solve(X, func, z0, t, adjoint, kw.pop("method", None) or "dopri5", kw.pop("options", None),
                              kw["rtol"], kw["atol"], kw.get("adjoint_method"), kw.get("adjoint_options"),
                              kw.get("adjoint_rtol"), kw.get("adjoint_atol"), kw.get("adjoint_params"))

    # compatibility probe of solver.py:44-67: one evaluation of func at t[0], shapes checked against z0;
    # the same evaluation establishes (bitwise) whether func belongs to the fused affine family.
    field, system = probe(func, t[0].to(z0.device) if isinstance(t, torch.Tensor) else t, z0)
    if not isinstance(system, torch.Tensor):
        raise ValueError("z0 is a tensor and so func must return a tensor as well.")
    _shape_errors(batch + (C,), tuple(system.shape), z0)
    # func's formula, when the probe identified it: lets the step-wise adjoint write its dynamics in closed form
    # (`variant="generic"` keeps autograd: the independent cross-check the tests compare against)
    recognised = field if variant == _lib.VARIANT_AUTO else None
    recognised_kind = None if field is None else field.kind
    mlp = mlp_wide = mlp_tall = mlp_broad = None
    if field is not None and field.kind == "mlp2":
        if _mlp_broad_fusable(field, H, C, z0, packed):     # 129 .. 256 inner units: its own kernels, rk4 only (kind "mlp2b")
            mlp_broad, field = field, None
        elif _mlp_wide_fusable(field, H, C, z0, packed):      # 17 .. 64 channels: its own kernels, rk4 only (kind "mlp2w")
            mlp_wide, field = field, None
        elif _mlp_tall_fusable(field, H, C, z0, packed):    # 33 .. 64 hidden channels: its own kernels, rk4 only (kind "mlp2h")
            mlp_tall, field = field, None
        else:
            mlp, field = (field if _mlp_fusable(field, H, C, z0, packed) else None), None
    mlp3 = None
    if field is not None and field.kind == "mlp3":
        mlp3, field = (field if _mlp3_fusable(field, H, C, z0, packed) else None), None
    if field is not None:
        weight, bias = field.weight, field.bias
        if tuple(weight.shape) != (H * C, H) or not (z0.dtype == packed.dtype == weight.dtype):
            field = None              # not a shape / dtype the fused kernels take: solve it step by step instead
        elif not _lib.load().cde_rk4_supported(C, H, _lib.dtype_enum(z0.dtype), field.act, int(bool(adjoint)), variant):
            field = None              # beyond the fused kernels' tiles (LDS / lane limits): step-wise, not a late error

    if revheun is not None:
        return _cdeint_reversible_heun(X, func, z0, t, adjoint, revheun, variant, field, recognised, recognised_kind,
                                       batch, H, C)
    if variant == _lib.VARIANT_BF16X3 and (field is None or field.act != _lib.ACT_NONE or kwargs.get("method") != "rk4"
                                           or z0.dtype != torch.float32 or H > 32 or C > 8):
        # an explicit request for a specific kernel family is never redirected
        raise NotImplementedError("torchcde_amd: variant='bf16x3' covers method='rk4' with the one-layer identity-activation "
                                  "field Linear(H, H*C), float32, H <= 32, C <= 8.")
    if adjoint and "adjoint_params" not in kwargs:
        for buffer in X.buffers():
            if buffer.requires_grad:
                warnings.warn(_GRAD_WARNING)

    # solver configuration (what the reference forwards verbatim to torchdiffeq, solver.py:175-176,227)
    method = kwargs.pop("method", None)
    options = kwargs.pop("options", None)
    if method is None:
        method = "dopri5"
    grad_mode = torch.is_grad_enabled()
    given_params = kwargs.get("adjoint_params")
    if given_params is not None:
        given_params = tuple(given_params)
    # what must be differentiated: z0, the field's parameters (or the caller's adjoint_params -- which may name the
    # control's coefficient / knot tensors, README.md:251-270), the output times
    param_source = given_params if (adjoint and given_params is not None) else (
        tuple(func.parameters()) if isinstance(func, torch.nn.Module) else ())
    wants_grad = grad_mode and (z0.requires_grad or any(isinstance(p, torch.Tensor) and p.requires_grad
                                                        for p in param_source))
    if not adjoint and grad_mode and any(b.requires_grad for b in X.buffers()):
        wants_grad = True            # backprop through the solver reaches the control: the step-wise path differentiates it
    wants_t = grad_mode and isinstance(t, torch.Tensor) and t.requires_grad
    wants_grad = wants_grad or wants_t
    # gradients w.r.t. the control's tensors or the times come out of the pre-activation MFMA adjoint kernel only
    control_ids = {b.untyped_storage().data_ptr() for b in X._control_buffers()} | {X._t.untyped_storage().data_ptr()}
    control_wants = grad_mode and adjoint and given_params is not None and any(
        isinstance(p, torch.Tensor) and p.requires_grad and p.untyped_storage().data_ptr() in control_ids
        for p in given_params)
    if not adjoint:
        # autograd through the solver's own operations reaches every control tensor that requires a gradient
        control_wants = grad_mode and any(b.requires_grad for b in X.buffers())
    mfma_shape = (field is not None and z0.dtype == torch.float32 and H <= 32 and C <= 8
                  and variant != _lib.VARIANT_GENERIC)
    adj_opts = kwargs.get("adjoint_options")
    adjoint_method = kwargs.get("adjoint_method")
    t_is_vector = isinstance(t, torch.Tensor) and t.dim() == 1 and t.is_floating_point() and t.numel() >= 1
    t_host = _to_host(t) if t_is_vector else None
    increasing = t_is_vector and (t_host.numel() == 1 or bool((t_host[1:] > t_host[:-1]).all()))

    # ---- how the caller's adjoint_params relate to the field's own parameters and the control's tensors
    known = (field if field is not None else mlp if mlp is not None else mlp3 if mlp3 is not None else
             mlp_wide if mlp_wide is not None else mlp_tall if mlp_tall is not None else mlp_broad)
    own = () if known is None else (
        (field.weight, field.bias) if field is not None else
        tuple(p for lin in known.linears for p in (lin.weight, lin.bias)))     # two / three layers: all four / all six
    params_kind = "default"
    if given_params is not None and known is not None:
        extra = [p for p in given_params if not any(p is o for o in own)]
        extra_ok = all(isinstance(p, torch.Tensor) and p.untyped_storage().data_ptr() in control_ids for p in extra)
        complete = field is not None or all(any(p is o for p in given_params) for o in own)    # K3m / K4am: all four or none; K3m3: all six
        params_kind = "own" if (extra_ok and complete) else "foreign"
        if field is None and any(p is X._t for p in extra) and method not in ("rk4", "dopri5"):
            params_kind = "foreign"             # knot-time gradients of a two-layer solve: under rk4 and (with the coefficient
                                                # tensor: control_block) dopri5, else step-wise

    # the adaptive backward measures every entry of adjoint_params as a block of its error norm: control gradients are fused
    # there when the ONE extra entry is the packed coefficient tensor the path reads (its buffers are views of it)
    control_block = None
    if given_params is not None and known is not None and params_kind == "own":
        extra = [p for p in given_params if not any(p is o for o in own)]
        tensors = [p for p in extra if p is not X._t]
        if (len(tensors) == 1 and len(extra) <= 2 and tensors[0].requires_grad and tensors[0].is_contiguous()
                and tensors[0].numel() == packed.numel() and tensors[0].dtype == packed.dtype
                and tensors[0].untyped_storage().data_ptr() == packed.untyped_storage().data_ptr()):
            control_block = tensors[0]          # (+ optionally the knot times X._t: a fourth block)

    fixed_keys, adaptive_keys = {"step_size"}, {"jump_t", "safety", "ifactor", "dfactor", *_STEP_KEYS}
    # ONE normalised view of the options for the fused paths (the step-wise path gets them verbatim, like torchdiffeq):
    # None values and torchdiffeq's own defaults spelled out are the same request as leaving the key away
    fused_options = _strip_noops(options, fixed=method != "dopri5")
    fused_adj_opts = _strip_noops(adj_opts, fixed=method != "dopri5")

    def within(opts, allowed):
        return opts is None or (isinstance(opts, dict) and set(opts) <= allowed)

    if method == "dopri5":
        options_ok = within(fused_options, adaptive_keys)
        adjoint_options_ok = fused_adj_opts is None or (within(fused_adj_opts, adaptive_keys | {"norm"})
                                                        and fused_adj_opts.get("norm", "seminorm") == "seminorm")
    else:
        options_ok = within(fused_options, fixed_keys)
        adjoint_options_ok = within(fused_adj_opts, fixed_keys)
    from .distributed import step_control
    request = dispatch.Request(
        prod=False, kind=(None if known is None else "mlp2w" if mlp_wide is not None else "mlp2h" if mlp_tall is not None
                          else "mlp2b" if mlp_broad is not None else known.kind),
        tiles_ok=known is not None, mfma_shape=mfma_shape,
        method=method, adjoint=bool(adjoint), wants_grad=bool(wants_grad), wants_t=bool(wants_t),
        wants_control=bool(control_wants), params=params_kind,
        adjoint_method_ok=adjoint_method in (None, method), options_ok=options_ok,
        adjoint_options_ok=adjoint_options_ok, t_ok=bool(increasing) or not t_is_vector,
        variant_generic=variant == _lib.VARIANT_GENERIC, shared=step_control() is not None, narrow_control=C <= 8,
        backprop_ok=bool((mfma_shape and variant in (_lib.VARIANT_AUTO, _lib.VARIANT_MFMA))
                         or (mlp is not None and variant == _lib.VARIANT_AUTO)),
        identity=bool(field is not None and field.act == _lib.ACT_NONE),
        control_block=control_block is not None)
    if recognised_kind is not None and known is None:
        # the probe recognised the formula but the shape / dtype is beyond the tiles: say so in the record and the warning
        request = request._replace(kind=recognised_kind, tiles_ok=False)
    choice = dispatch.select_path(request)
    if (mlp is not None and _mlp_upper_half(H, C) and choice.path != dispatch.STEPWISE
            and (choice.path not in _UPPER_HALF_PATHS or (choice.path == "mlp_dopri5_adjoint" and request.shared))):
        # 32 units x 16 channels: fused where the kernels read the upper half (see _UPPER_HALF_PATHS)
        request = request._replace(tiles_ok=False)
        choice = dispatch.select_path(request)
    if choice.path == "rk4" and field is not None and field.kind == "affine":
        B_total = z0.numel() // H
        if _lib.load().cde_rk4_bf16x3_form(B_total, C, H, _lib.dtype_enum(z0.dtype), field.act, variant):
            form = "bf16x3_forward" if (control_wants and variant == _lib.VARIANT_AUTO) else "bf16x3"
        else:
            form = "exact"
        tiled = (variant == _lib.VARIANT_AUTO and not control_wants and not wants_t
                 and _lib.load().cde_rk4_affine_tiled_supported(C, H, _lib.dtype_enum(z0.dtype), field.act))
        choice = choice.with_form(form, "tiled" if tiled else "")
    dispatch.record(choice, request)

    if choice.path == dispatch.STEPWISE:
        # Arbitrary vector fields / methods / differentiation modes: host-driven stepping with the native control
        # derivative and contraction kernels under every evaluation (torchcde_amd/stepwise.py).
        from . import stepwise
        dispatch.warn_once(func, choice, request)
        if step_control() is not None and (method == "dopri5" or adjoint_method == "dopri5"):
            warnings.warn("torchcde_amd: shared_step_control() is active but this adaptive solve runs step-wise, which "
                          "does not share its step controller across ranks: every rank takes its own step sequence.")
        kw = stepwise_kwargs
        return stepwise.solve(X, func, z0, t, adjoint, method, options, kw["rtol"], kw["atol"],
                              kw.get("adjoint_method"), kw.get("adjoint_options"), kw.get("adjoint_rtol"),
                              kw.get("adjoint_atol"), kw.get("adjoint_params"), recognised=recognised)
    if not t_is_vector:
        raise ValueError("t must be a one dimensional floating point tensor.")

    unknown = set(kwargs) - {"rtol", "atol", "adjoint_rtol", "adjoint_atol", "adjoint_method", "adjoint_options",
                             "adjoint_params"}
    if unknown:
        raise NotImplementedError("torchcde_amd: unsupported cdeint keyword arguments {}".format(sorted(unknown)))

    # ---- three-layer fields (rk4 only: forward, and the continuous adjoint for z0 and the six parameters)
    if mlp3 is not None:
        step = _parse_fixed_options(fused_options, "solver")
        if choice.path == "mlp_rk4_forward":
            with torch.no_grad():
                return _Mlp3Plan(X, mlp3, batch, H, C, t, step).run(z0)
        adj_step = step if fused_adj_opts is None else _parse_fixed_options(fused_adj_opts, "adjoint")
        plan = _Mlp3Plan(X, mlp3, batch, H, C, t, step, adj_step)
        return _FusedMlp3RK4.apply(z0, *(p for lin in mlp3.linears for p in (lin.weight, lin.bias)), plan, None, None, None)

    # ---- two-layer fields on 17 .. 64 channels (rk4 only: forward, and the continuous adjoint for z0 and the four parameters)
    if mlp_wide is not None:
        step = _parse_fixed_options(fused_options, "solver")
        if choice.path == "mlp_rk4_forward":
            with torch.no_grad():
                return _MlpWidePlan(X, mlp_wide, batch, H, C, t, step).run(z0)
        adj_step = step if fused_adj_opts is None else _parse_fixed_options(fused_adj_opts, "adjoint")
        plan = _MlpWidePlan(X, mlp_wide, batch, H, C, t, step, adj_step)
        return _FusedMlpWideRK4.apply(z0, mlp_wide.hidden.weight, mlp_wide.hidden.bias, mlp_wide.output.weight,
                                      mlp_wide.output.bias, plan, None, None, None)

    # ---- two-layer fields on 33 .. 64 hidden channels (rk4 only: forward, and the continuous adjoint for z0 and the four parameters)
    if mlp_tall is not None:
        step = _parse_fixed_options(fused_options, "solver")
        if choice.path == "mlp_rk4_forward":
            with torch.no_grad():
                return _MlpTallPlan(X, mlp_tall, batch, H, C, t, step).run(z0)
        adj_step = step if fused_adj_opts is None else _parse_fixed_options(fused_adj_opts, "adjoint")
        plan = _MlpTallPlan(X, mlp_tall, batch, H, C, t, step, adj_step)
        return _FusedMlpTallRK4.apply(z0, mlp_tall.hidden.weight, mlp_tall.hidden.bias, mlp_tall.output.weight,
                                      mlp_tall.output.bias, plan, None, None, None)

    # ---- two-layer fields with 129 .. 256 inner units (rk4 only: forward, and the continuous adjoint for z0 and the four parameters)
    if mlp_broad is not None:
        step = _parse_fixed_options(fused_options, "solver")
        if choice.path == "mlp_rk4_forward":
            with torch.no_grad():
                return _MlpBroadPlan(X, mlp_broad, batch, H, C, t, step).run(z0)
        adj_step = step if fused_adj_opts is None else _parse_fixed_options(fused_adj_opts, "adjoint")
        plan = _MlpBroadPlan(X, mlp_broad, batch, H, C, t, step, adj_step)
        return _FusedMlpBroadRK4.apply(z0, mlp_broad.hidden.weight, mlp_broad.hidden.bias, mlp_broad.output.weight,
                                       mlp_broad.output.bias, plan, None, None, None)

    # ---- two-layer fields
    if choice.path == "mlp_rk4_adjoint":
        step = _parse_fixed_options(fused_options, "solver")
        adj_step = step if fused_adj_opts is None else _parse_fixed_options(fused_adj_opts, "adjoint")
        plan = _MlpPlan(X, mlp, batch, H, C, t, step, adj_step)
        want_knots = bool(grad_mode and given_params is not None and any(p is X._t and p.requires_grad for p in given_params))
        # (the coefficient tensor the path was built from: dL/dcoeffs flows back through the path's buffer views)
        want_x = bool(grad_mode and given_params is not None and any(
            isinstance(p, torch.Tensor) and p.requires_grad and p is not X._t
            and p.untyped_storage().data_ptr() in control_ids for p in given_params))
        control_inputs = X._control_buffers() if want_x else ()
        plan.fit_chain = _knot_fit_chain(X) if want_knots else None
        return _FusedMlpRK4.apply(z0, mlp.hidden.weight, mlp.hidden.bias, mlp.output.weight, mlp.output.bias, plan,
                                  None, t if wants_t else None, X._t if want_knots else None, *control_inputs)
    if choice.path in ("rk4_backprop", "mlp_rk4_backprop"):
        # adjoint=False: the control tensors autograd must reach (their gradients come out of the same reverse-mode sweep)
        want_x = bool(grad_mode and any(b.requires_grad for b in X._control_buffers()))
        knots_in = X._t if (grad_mode and X._t.requires_grad) else None
        control_inputs = X._control_buffers() if want_x else ()
    if choice.path == "mlp_rk4_backprop":
        plan = _MlpPlan(X, mlp, batch, H, C, t, _parse_fixed_options(fused_options, "solver"))
        return _FusedMlpRK4Backprop.apply(z0, mlp.hidden.weight, mlp.hidden.bias, mlp.output.weight, mlp.output.bias, plan,
                                          None, None, knots_in, *control_inputs)
    if choice.path == "mlp_rk4_forward":
        with torch.no_grad():
            return _MlpPlan(X, mlp, batch, H, C, t, _parse_fixed_options(fused_options, "solver")).run(z0)
    if choice.path in ("mlp_dopri5_forward", "mlp_dopri5_adjoint"):
        plan = _Dopri5Plan(X, mlp, batch, H, C, t, kwargs["rtol"], kwargs["atol"], fused_options, variant,
                           kwargs.get("adjoint_rtol"), kwargs.get("adjoint_atol"), fused_adj_opts)
        if choice.path == "mlp_dopri5_forward":
            with torch.no_grad():
                return plan.run(z0, mlp.weight, mlp.bias).reshape(*batch, plan.n_out, H)
        # the reference examples' own training call (no method: dopri5 + adjoint): K4 forward, K4am backward
        want_x = bool(control_wants and control_block is not None)
        control_inputs = X._control_buffers() if want_x else ()
        plan.control_numel = control_block.numel() if want_x else 0
        knots_in = X._t if (want_x and any(p is X._t and p.requires_grad for p in given_params)) else None
        plan.fit_chain = _knot_fit_chain(X) if knots_in is not None else None
        return _FusedMlpDopri5.apply(z0, mlp.hidden.weight, mlp.hidden.bias, mlp.output.weight, mlp.output.bias, plan,
                                     None, t if wants_t else None, knots_in, *control_inputs)

    # ---- one-layer fields
    weight, bias = field.weight, field.bias
    if choice.path == "rk4_backprop":
        plan = _Plan(X, field, batch, H, C, t, _parse_fixed_options(fused_options, "solver"), None, False, variant)
        return _FusedRK4Backprop.apply(z0, weight, bias, plan, None, None, knots_in, *control_inputs)
    if choice.path in ("dopri5_forward", "dopri5_adjoint"):
        plan = _Dopri5Plan(X, field, batch, H, C, t, kwargs["rtol"], kwargs["atol"], fused_options, variant,
                           kwargs.get("adjoint_rtol"), kwargs.get("adjoint_atol"), fused_adj_opts)
        if choice.path == "dopri5_forward":
            # nothing is to be differentiated (`adjoint_params=()` with weights that still require grad, no_grad ...): no
            # autograd node -- one here would reach K4a without its eligibility checks
            with torch.no_grad():
                return plan.run(z0, weight, bias).reshape(*batch, plan.n_out, H)
        wants = (True, True) if given_params is None else (any(p is weight for p in given_params),
                                                           any(p is bias for p in given_params))
        # control gradients: dL/dcoeffs flows back to the caller's tensor through the path's buffer views
        want_x = bool(control_wants and control_block is not None)
        control_inputs = X._control_buffers() if want_x else ()
        plan.control_numel = control_block.numel() if want_x else 0
        knots_in = X._t if (want_x and any(p is X._t and p.requires_grad for p in given_params)) else None
        plan.fit_chain = _knot_fit_chain(X) if knots_in is not None else None
        return _FusedDopri5.apply(z0, weight, bias, plan, wants, t if wants_t else None, knots_in, *control_inputs)
    step_size = _parse_fixed_options(fused_options, "solver")
    adjoint_step = step_size if fused_adj_opts is None else _parse_fixed_options(fused_adj_opts, "adjoint")
    want_w = want_b = True
    want_x = want_knots = False
    if given_params is not None and adjoint:
        for p in given_params:
            if p is weight or p is bias:
                continue
            if p is X._t:
                # the knot times of the control (reference test/test_tricks.py:21-49 passes them): the chain through
                # `frac = t - t_j` of the spline evaluation
                want_knots = want_knots or (p.requires_grad and grad_mode)
            else:
                # the coefficient tensor the path was built from (README.md:251-270): dL/dcoeffs flows back to it
                # through the path's buffer views
                want_x = want_x or (p.requires_grad and grad_mode)
        want_w = any(p is weight for p in given_params)
        want_b = any(p is bias for p in given_params)
    plan = _Plan(X, field, batch, H, C, t, step_size, adjoint_step, adjoint, variant,
                 _lib.FIXED_METHODS[method] if choice.path == "fixed_grid" else _lib.METHOD_RK4)
    control_inputs = X._control_buffers() if want_x else ()
    plan.fit_chain = _knot_fit_chain(X) if want_knots else None
    return _FusedRK4.apply(z0, weight, bias, plan, (want_w, want_b), t if wants_t else None,
                           X._t if want_knots else None, *control_inputs)


# ------------------------------------------------------------------------------------------ per-thread module attributes
class _Module(types.ModuleType):
    """`torchcde_amd.cdeint.last_dopri5_stats` etc. read and write the CALLING THREAD's state (_CallState): two threads
    solving at once do not see each other's statistics, and one thread recording step traces does not switch it on for
    the other."""
    last_dopri5_stats = property(lambda self: _state().dopri5)
    last_dopri5_adjoint_stats = property(lambda self: _state().dopri5_adjoint)
    record_dopri5_steps = property(lambda self: _state().record, lambda self, value: setattr(_state(), "record", bool(value)))
    event_log = property(lambda self: _state().event_log, lambda self, value: setattr(_state(), "event_log", value))


sys.modules[__name__].__class__ = _Module
