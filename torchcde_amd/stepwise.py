"""Step-wise solve for vector fields the fused kernels do not recognise.

``func`` is arbitrary user PyTorch code, so it cannot be fused; what the reference owns around it still runs
natively on every vector-field evaluation:

    dX/dt        K1b  ``cde_path_eval``     (replaces CubicSpline.derivative, interpolation_cubic.py:331-336)
    f(t,z) @ dX  ``cde_contract``           (replaces the batched mat-vec of _VectorField.forward, solver.py:130)

and the time stepping that the reference delegates to torchdiffeq (solver.py:226-227) is driven from the host with
the same semantics as the fused kernels / SURVEY appendix A: fixed-grid ``rk4`` (3/8 rule), ``midpoint``, ``euler``;
adaptive ``dopri5`` with the batch-global controller; linear / dense output interpolation; continuous adjoint
(augmented state integrated backwards with the forward method) or plain autograd through the steps
(``adjoint=False``).  Everything stays on the GPU; there is no CPU fallback here either.
"""
import bisect

import torch

from . import _lib


# ------------------------------------------------------------------------------------------ native pieces
class _Contract(torch.autograd.Function):
    """out[..., h] = sum_c F[..., h, c] * dX[..., c]  (native forward; the backward is an outer product)."""

    @staticmethod
    def forward(ctx, F, dX):
        lib = _lib.load()
        _lib.require_gpu(F, "func(t, z)")
        H, C = F.size(-2), F.size(-1)
        Fc = F.detach().contiguous()
        dXc = dX.detach().to(F.dtype).contiguous()
        B = Fc.numel() // (H * C)
        out = torch.empty(F.shape[:-1], dtype=F.dtype, device=F.device)
        _lib.check(lib.cde_contract(_lib.ptr(Fc), _lib.ptr(dXc), _lib.ptr(out), B, H, C, _lib.dtype_enum(F.dtype),
                                    _lib.stream_ptr(F.device)), "cde_contract")
        ctx.save_for_backward(dXc, Fc if dX.requires_grad else None)
        ctx.f_shape, ctx.dx_shape = F.shape, dX.shape
        return out

    @staticmethod
    def backward(ctx, grad):
        dX, F = ctx.saved_tensors
        grad_F = grad.unsqueeze(-1) * dX.reshape(ctx.f_shape[:-2] + (1, ctx.f_shape[-1]))
        grad_dX = None
        if F is not None and ctx.needs_input_grad[1]:          # the control derivative carries gradient to the coefficients
            grad_dX = (grad.unsqueeze(-1) * F.reshape(ctx.f_shape)).sum(-2).reshape(ctx.dx_shape)
        return grad_F, grad_dX


class ControlledField:
    """t, z -> f(t, z) dX/dt with the reference's shape contract (solver.py:117-135)."""

    def __init__(self, X, func):
        self.X, self.func = X, func
        self.through_time = False      # backprop through the solver: dX/dt(t) itself is differentiated w.r.t. t
        self.recognised = None         # fields.AffineField / MLPField when the probe identified func's formula

    def __call__(self, t, z):
        dX = self.X.derivative(t if self.through_time else t.detach())
        if hasattr(self.func, "prod"):                       # solver.py:121-123: the user supplies f(t, z) dX directly
            return self.func.prod(t, z, dX)
        return _Contract.apply(self.func(t, z), dX)

    def time_partial(self, t, z):
        """The part of d f(t, z)/dt that autograd cannot see here: f depends on t through dX/dt(t), which is a native
        kernel call on detached times -- f(t, z) with dX/dt replaced by d2X/dt2 (f is linear in the control slope)."""
        with torch.no_grad():
            d2X = self.X._second_derivative(t.detach())
            if hasattr(self.func, "prod"):
                return self.func.prod(t, z, d2X)
            return _Contract.apply(self.func(t, z), d2X)


class ForeignControlField(ControlledField):
    """The same for a control that is not one of this package's paths (reference solver.py:45-46, :117-135): X.derivative is
    the user's code, so it is called under the ambient autograd mode with the time it is given -- gradients reach X's own
    parameters when they are among `adjoint_params`, and the time through X when the control depends on it smoothly."""

    def __call__(self, t, z):
        dX = self.X.derivative(t)
        if hasattr(self.func, "prod"):
            return self.func.prod(t, z, dX)
        return _Contract.apply(self.func(t, z), dX)

    def time_partial(self, t, z):
        # nothing to add: X.derivative ran on the very time tensor the adjoint differentiates, so autograd has already
        # seen the dependence of f on t through the control (ControlledField adds it by hand because the native
        # derivative kernel is opaque to autograd)
        return torch.zeros_like(z)


def _explicit_dynamics(field, params):
    """The augmented dynamics of the continuous adjoint in closed form for a RECOGNISED vector field (fields.py: the
    probe established bitwise that func is act(Linear(z)), act(Linear(hid(Linear(z)))) or act(Linear(hid(Linear(hid(Linear(z))))))
    with hid = relu | softplus, viewed (..., H, C)):
    (t, y, a) -> (f, -a^T df/dy, [-a^T df/dp for p in params]) with a dozen matrix / elementwise launches instead of an
    autograd graph of about forty per evaluation -- the step-wise adaptive backward of the reference's example models
    (two-layer field, default dopri5 + adjoint call) is bound by launches, not by arithmetic.  Returns None when a
    parameter is not one of the field's weights / biases (autograd then differentiates func as usual)."""
    rec = getattr(field, "recognised", None)
    if rec is None or not isinstance(field, ControlledField) or hasattr(field.func, "prod"):
        return None
    layers = rec.linears
    slots = []
    def same(own, p):            # backward() sees the parameters as saved tensors: identity, or the same memory
        return own is not None and (own is p or (own.shape == p.shape and own.dtype == p.dtype and
                                                 own.data_ptr() == p.data_ptr()))
    for p in params:
        where = [(i, name) for i, lin in enumerate(layers) for name in ("weight", "bias") if same(getattr(lin, name), p)]
        if not where:
            return None
        slots.append(where[0])
    tanh = rec.act == _lib.ACT_TANH
    hidden_layers = layers[:-1]                  # none (affine), one (two-layer field) or two (three-layer field)
    softplus = bool(hidden_layers) and rec.hidden_act == _lib.HIDDEN_SOFTPLUS
    out_layer = layers[-1]
    last = len(layers) - 1

    def run(tt, yy, aa):
        H = yy.size(-1)
        z, a = yy.reshape(-1, H), aa.reshape(-1, H)
        dX = field.X.derivative(tt)
        C = dX.size(-1)
        dX = dX.reshape(-1, C)
        r = z
        inputs, pres = [], []                    # per hidden layer: what it was applied to, its pre-activation
        for lin in hidden_layers:
            w1, b1 = lin.weight, lin.bias
            h1 = r @ w1.t() if b1 is None else torch.addmm(b1, r, w1.t())
            inputs.append(r)
            pres.append(h1)
            r = torch.nn.functional.softplus(h1) if softplus else h1.relu()
        w, b = out_layer.weight, out_layer.bias
        u = r @ w.t() if b is None else torch.addmm(b, r, w.t())
        th = u.tanh() if tanh else u
        fe = _Contract.apply(th.view(-1, H, C), dX)
        gu = (a.neg().unsqueeze(-1) * dX.unsqueeze(-2)).reshape(-1, H * C)            # cotangent -a on f = F dX
        if tanh:
            gu = torch.addcmul(gu, gu * th, th, value=-1)                             # * (1 - tanh^2)
        grads = {}
        need = set(slots)
        if (last, "weight") in need:
            grads[(last, "weight")] = gu.t() @ r
        if (last, "bias") in need:
            grads[(last, "bias")] = gu.sum(0)
        vy = gu @ w
        for i in range(len(hidden_layers) - 1, -1, -1):                               # back through the hidden layers
            h1 = pres[i]
            gh1 = vy * (torch.sigmoid(h1).masked_fill(h1 > 20, 1.0) if softplus else (h1 > 0))   # softplus' = sigmoid; torch: 1 above its threshold
            if (i, "weight") in need:
                grads[(i, "weight")] = gh1.t() @ inputs[i]
            if (i, "bias") in need:
                grads[(i, "bias")] = gh1.sum(0)
            vy = gh1 @ hidden_layers[i].weight
        return fe.reshape(yy.shape), vy.reshape(yy.shape), [grads[slot].reshape(p.shape) for slot, p in zip(slots, params)]

    return run


# ------------------------------------------------------------------------------------------ helpers
_NONE, _PREV, _NEXT = 0, 1, 2


def _rms(x):
    return x.abs().pow(2).mean().sqrt()


def _nudge(t, direction):
    with torch.no_grad():
        delta = torch.nextafter(t, t + direction) - t
    return t + delta


def _flatten(parts):
    return torch.cat([p.reshape(-1) for p in parts])


def _unflatten(flat, lead, shapes):
    out, offset = [], 0
    for shape in shapes:
        n = 1
        for s in shape:
            n *= s
        out.append(flat[..., offset:offset + n].reshape(tuple(lead) + tuple(shape)))
        offset += n
    return tuple(out)


class _Wrapped:
    """torchdiffeq's function wrappers in one place: tuple flattening, time reversal, time cast, ulp nudges."""

    def __init__(self, func, shapes=None, reverse=False):
        self.func, self.shapes, self.reverse = func, shapes, reverse

    def __call__(self, t, y, perturb=_NONE):
        t = t.to(y.dtype)
        if perturb == _NEXT:
            t = _nudge(t, 1)
        elif perturb == _PREV:
            t = _nudge(t, -1)
        if self.reverse:
            t = -t
        if self.shapes is None:
            out = self.func(t, y)
        else:
            out = _flatten(self.func(t, _unflatten(y, (), self.shapes)))
        return -1.0 * out if self.reverse else out


# ------------------------------------------------------------------------------------------ fixed grid
def _grid(t, step_size):
    if step_size is None:
        return t
    n = torch.ceil((t[-1] - t[0]) / step_size + 1).item()
    grid = torch.arange(0, n, dtype=t.dtype, device=t.device) * step_size + t[0]
    grid[-1] = t[-1]
    return grid


def _inc_rk4(f, t0, dt, t1, y0):
    third, two_thirds = 1 / 3, 2 / 3
    k1 = f(t0, y0)
    k2 = f(t0 + dt * third, y0 + dt * k1 * third)
    k3 = f(t0 + dt * two_thirds, y0 + dt * (k2 - k1 * third))
    k4 = f(t1, y0 + dt * (k1 - k2 + k3))
    return (k1 + 3 * (k2 + k3) + k4) * dt * 0.125


def _inc_midpoint(f, t0, dt, t1, y0):
    half = 0.5 * dt
    return dt * f(t0 + half, y0 + f(t0, y0) * half)


def _inc_euler(f, t0, dt, t1, y0):
    return dt * f(t0, y0)


_FIXED = {"rk4": _inc_rk4, "midpoint": _inc_midpoint, "euler": _inc_euler}


def _solve_fixed(increment, f, y0, t, step_size):
    t_host = t.detach().cpu()                       # the grid and the output bookkeeping live on the host
    grid = _grid(t_host, step_size)
    # backprop through the solver w.r.t. the times: the device copy of the grid stays a function of `t`, built as
    # torchdiffeq builds it (the output times themselves, or t[0] + i * step_size with the last point replaced by t[-1])
    through = torch.is_grad_enabled() and t.requires_grad
    if through:
        t_dev = t.to(y0.device)
        if step_size is None:
            grid_dev = t_dev
        else:
            steps = torch.arange(0, len(grid), dtype=t_dev.dtype, device=t_dev.device) * step_size + t_dev[0]
            grid_dev = torch.cat([steps[:-1], t_dev[-1:]])
    out = [y0]
    j = 1
    on_device = lambda v: v.to(y0.device)
    for i, (t0h, t1h) in enumerate(zip(grid[:-1], grid[1:])):
        t0, t1 = (grid_dev[i], grid_dev[i + 1]) if through else (on_device(t0h), on_device(t1h))
        dt = t1 - t0
        y1 = y0 + increment(f, t0, dt, t1, y0)
        while j < len(t_host) and bool(t1h >= t_host[j]):
            tj = t_host[j]
            if bool(tj == t0h):
                out.append(y0)
            elif bool(tj == t1h):
                out.append(y1)
            else:
                slope = ((t_dev[j] - t0) / (t1 - t0) if through else on_device((tj - t0h) / (t1h - t0h))).to(y0.dtype)
                out.append(y0 + slope * (y1 - y0))
            j += 1
        y0 = y1
    return torch.stack(out)


# ------------------------------------------------------------------------------------------ dopri5
_ALPHA = [1 / 5, 3 / 10, 4 / 5, 8 / 9, 1., 1.]
_BETA = [[1 / 5], [3 / 40, 9 / 40], [44 / 45, -56 / 15, 32 / 9], [19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729],
         [9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656],
         [35 / 384, 0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84]]
_C_ERR = [35 / 384 - 1951 / 21600, 0, 500 / 1113 - 22642 / 50085, 125 / 192 - 451 / 720,
          -2187 / 6784 - -12231 / 42400, 11 / 84 - 649 / 6300, -1. / 60.]
_C_MID = [6025192743 / 30085553152 / 2, 0, 51252292925 / 65400821598 / 2, -2691868925 / 45128329728 / 2,
          187940372067 / 1594534317056 / 2, -1776094331 / 19743644256 / 2, 11237099 / 235043384 / 2]


_DOPRI5_OPTIONS = ("jump_t", "safety", "ifactor", "dfactor", "max_num_steps", "first_step", "step_t", "min_step", "max_step")


def _solve_dopri5(f, y0, t, rtol, atol, norm, jump_t=None, safety=0.9, ifactor=10.0, dfactor=0.2,
                  max_num_steps=2 ** 31 - 1, first_step=None, step_t=None, min_step=0, max_step=float("inf"), record=None):
    """Host-driven Dormand-Prince with torchdiffeq's controller (float64 time, batch-global RMS error norm).
    first_step / step_t / min_step / max_step as torchdiffeq's adaptive solvers read them (oracle/odeint.py: _Dopri5):
    every attempt's step size is clamped to [min_step, max_step], clipped onto the next step time, and an attempt longer
    than max_step is rejected, one no longer than min_step accepted, whatever its error ratio.  `record`: a list that
    receives (t0, t1, on_jump, accepted) of every attempt."""
    dev, ydt = y0.device, y0.dtype
    td = torch.float64
    as_t = lambda v: torch.as_tensor(v, dtype=td, device=dev)
    rtol, atol, safety, ifactor, dfactor = as_t(rtol), as_t(atol), as_t(safety), as_t(ifactor), as_t(dfactor)
    min_step = as_t(0 if min_step is None else min_step)
    max_step = as_t(float("inf") if max_step is None else max_step)
    beta = [torch.tensor(b, dtype=ydt, device=dev) for b in _BETA]
    alpha = torch.tensor(_ALPHA, dtype=ydt, device=dev)
    c_err = torch.tensor(_C_ERR, dtype=ydt, device=dev)
    c_mid = torch.tensor(_C_MID, dtype=ydt, device=dev)
    t = t.to(td)
    out = [y0]
    f0 = f(t[0], y0)
    if first_step is not None:
        dt = as_t(first_step)
    else:
        # Hairer's initial step (order 4 -> exponent 1/5)
        scale = atol + torch.abs(y0) * rtol
        d0, d1 = norm(y0 / scale).abs(), norm(f0 / scale).abs()
        h0 = torch.tensor(1e-6, dtype=ydt, device=dev) if (d0 < 1e-5 or d1 < 1e-5) else 0.01 * d0 / d1
        h0 = h0.abs()
        f1 = f(t[0] + h0, y0 + h0 * f0)
        d2 = torch.abs(norm((f1 - f0) / scale) / h0)
        if d1 <= 1e-15 and d2 <= 1e-15:
            h1 = torch.max(torch.tensor(1e-6, dtype=ydt, device=dev), h0 * 1e-3)
        else:
            h1 = (0.01 / max(d1, d2)) ** (1. / 5.)
        dt = torch.min(100 * h0, h1.abs()).to(td)

    def kept(times):                            # torchdiffeq keeps the times >= t[0], sorted
        if times is None:
            return []
        tt = torch.as_tensor(times, dtype=td, device=dev).detach().reshape(-1)      # (a list of floats: read as float64)
        return torch.sort(tt[tt >= t[0]]).values.tolist()
    jumps, steps = kept(jump_t), kept(step_t)
    both = sorted(steps + jumps)
    if any(a == b for a, b in zip(both[:-1], both[1:])):
        raise ValueError("`step_t` and `jump_t` must not have any repeated elements between them.")
    i_jump = min(bisect.bisect(jumps, t[0].item()), len(jumps) - 1)
    i_step = min(bisect.bisect(steps, t[0].item()), len(steps) - 1)
    y, fy, t_lo, t_hi, dense = y0, f0, t[0], t[0], None
    for i in range(1, len(t)):
        target = t[i]
        n = 0                                   # torchdiffeq counts max_num_steps per output interval
        while target > t_hi:
            assert n < max_num_steps, "max_num_steps exceeded"
            n += 1
            t0 = t_hi
            if not torch.isfinite(dt):
                dt = min_step
            dt = dt.clamp(min_step, max_step)
            t1 = t0 + dt
            on_step = on_jump = False
            if steps:
                nxt = steps[i_step]
                if t0.item() < nxt < (t0 + dt).item():
                    on_step, t1 = True, as_t(nxt)
                    dt = t1 - t0
            if jumps:
                nxt = jumps[i_jump]
                if t0.item() < nxt < (t0 + dt).item():
                    on_jump, on_step, t1 = True, False, as_t(nxt)
                    dt = t1 - t0
            t0y, dty, t1y = t0.to(ydt), dt.to(ydt), t1.to(ydt)
            ks = [fy]
            yi = y
            for s, (a, b) in enumerate(zip(alpha, beta)):
                ti, perturb = (t1y, _PREV) if s >= 4 else (t0y + a * dty, _NONE)
                yi = y + torch.stack(ks, dim=-1).matmul(b * dty).view_as(fy)
                ks.append(f(ti, yi, perturb=perturb))
            k = torch.stack(ks, dim=-1)
            y1, f1 = yi, ks[-1]
            tol = atol + rtol * torch.max(y.abs(), y1.abs())
            ratio = norm(k.matmul(dty * c_err) / tol).abs()
            accept = bool(ratio <= 1)
            if bool(dt > max_step):
                accept = False
            if bool(dt <= min_step):
                accept = True
            if record is not None:
                record.append((t0.item(), t1.item(), float(on_jump), float(accept)))
            if accept:
                dense = (y, fy, y1, f1, k, dty)          # the interpolant's coefficients are formed only if it is evaluated
                if on_step and i_step != len(steps) - 1:
                    i_step += 1
                if on_jump:
                    if i_jump != len(jumps) - 1:
                        i_jump += 1
                    f1 = f(t1, y1, perturb=_NEXT)
                y, fy, t_lo, t_hi = y1, f1, t0, t1
            else:
                t_lo, t_hi = t0, t0
            if ratio == 0:
                dt = dt * ifactor
            else:
                df = torch.ones((), dtype=td, device=dev) if ratio < 1 else dfactor
                dt = dt * torch.min(ifactor, torch.max(safety / ratio.to(td) ** 0.2, df))
            dt = dt.clamp(min_step, max_step)
        ya, fa, yb, fb, k, dty = dense                  # the step that reached the output time: quartic dense output
        ymid = ya + k.matmul(dty * c_mid).view_as(ya)
        coeffs = (ya, dty * fa, dty * (fb - 4 * fa) - 11 * ya - 5 * yb + 16 * ymid,
                  dty * (5 * fa - 3 * fb) + 18 * ya + 14 * yb - 32 * ymid,
                  2 * dty * (fb - fa) - 8 * (yb + ya) + 16 * ymid)
        x = ((target - t_lo) / (t_hi - t_lo)).to(ydt)
        total, xp = coeffs[0] + x * coeffs[1], x
        for coeff in coeffs[2:]:
            xp = xp * x
            total = total + xp * coeff
        out.append(total)
    return torch.stack(out)


# ------------------------------------------------------------------------------------------ front end
def odeint(func, y0, t, *, method, options, rtol, atol):
    """(len(t), *y0.shape) solution, tensor or tuple state, increasing or decreasing ``t``."""
    options = {} if options is None else dict(options)
    shapes = None
    if not isinstance(y0, torch.Tensor):
        shapes = [tuple(p.shape) for p in y0]
        y0 = _flatten(y0)
    reverse = len(t) > 1 and bool(t[0] > t[1])
    if reverse:
        t = -t
        for key in ("jump_t", "step_t"):
            if options.get(key) is not None:
                options[key] = -torch.as_tensor(options[key]).flip(0)
    f = _Wrapped(func, shapes, reverse)
    norm = options.pop("norm", None)
    if norm is None:
        norm = _rms if shapes is None else (lambda flat: max(_rms(p) for p in _unflatten(flat, (), shapes)))
    elif shapes is not None:
        user_norm = norm
        norm = lambda flat: user_norm(_unflatten(flat, (), shapes))
    if method in _FIXED:
        step_size = options.pop("step_size", None)
        for key in ("grid_constructor", "perturb"):
            if options.pop(key, None):
                raise NotImplementedError("torchcde_amd: option %r is not supported on the step-wise path" % key)
        if options.pop("interp", "linear") != "linear" or options:
            raise NotImplementedError("torchcde_amd: unsupported fixed-grid options %s" % sorted(options))
        sol = _solve_fixed(_FIXED[method], f, y0, t, step_size)
    elif method == "dopri5":
        allowed = {k: options.pop(k) for k in _DOPRI5_OPTIONS if k in options}
        if any(v is not None for v in options.values()):
            raise NotImplementedError("torchcde_amd: unsupported dopri5 options %s" % sorted(options))
        sol = _solve_dopri5(f, y0, t, rtol, atol, norm, **allowed)
    else:
        raise NotImplementedError("torchcde_amd: method %r is not implemented (rk4, midpoint, euler, dopri5 are)" % method)
    if shapes is not None:
        sol = _unflatten(sol, (len(t),), shapes)
    return sol


class _Adjoint(torch.autograd.Function):
    """Continuous adjoint, torchdiffeq's scheme: augmented state (vjp_t, y, a_y, a_params...)
    integrated backwards per output interval; y re-seeded from the stored solution, a_y bumped by the incoming
    gradient at every output time."""

    @staticmethod
    def forward(ctx, cfg, y0, t, *params):
        ctx.cfg = cfg
        with torch.no_grad():
            ans = odeint(cfg["func"], y0, t, method=cfg["method"], options=cfg["options"], rtol=cfg["rtol"],
                         atol=cfg["atol"])
        ctx.save_for_backward(t, ans, *params)
        return ans

    @staticmethod
    def backward(ctx, grad_y):
        cfg = ctx.cfg
        func = cfg["func"]
        t, y, *params = ctx.saved_tensors
        params = tuple(params)
        with torch.no_grad():
            need_t = cfg["t_requires_grad"]
            aug = [torch.zeros((), dtype=y.dtype, device=y.device), y[-1], grad_y[-1]]
            aug.extend(torch.zeros_like(p) for p in params)

            explicit = _explicit_dynamics(func, params)

            def dynamics(time, state):
                yy, aa = state[1], state[2]
                if explicit is not None:
                    tt = time.detach().to(yy.dtype)
                    fe, vy, vp = explicit(tt, yy, aa)
                    vt = torch.zeros_like(state[0])            # a recognised field does not read t itself
                    if need_t:
                        vt = vt - (aa * func.time_partial(tt, yy)).sum().to(vt.dtype)
                    return (vt, fe, vy, *vp)
                with torch.enable_grad():
                    # the "detach trick" (reference test/test_tricks.py:111-131): t joins the graph only when its
                    # gradient is wanted, so parameter gradients are bitwise the same either way
                    tt = time.detach().to(yy.dtype)
                    if need_t:
                        tt = tt.requires_grad_(True)
                    yy = yy.detach().requires_grad_(True)
                    fe = func(tt, yy)
                    if need_t:
                        vt, vy, *vp = torch.autograd.grad(fe, (tt, yy) + params, -aa, allow_unused=True,
                                                          retain_graph=True)
                    else:
                        vt = None
                        # retain_graph as torchdiffeq: an adjoint_param may itself be the output of a differentiable
                        # construction (the reference's own test passes `coeffs = natural_cubic_coeffs(path, t)`), whose
                        # graph every evaluation then walks
                        vy, *vp = torch.autograd.grad(fe, (yy,) + params, -aa, allow_unused=True, retain_graph=True)
                vt = torch.zeros_like(state[0]) if vt is None else vt.to(state[0].dtype)
                if need_t and hasattr(func, "time_partial"):           # d f/dt through the control slope dX/dt(t)
                    vt = vt - (aa * func.time_partial(tt.detach(), yy.detach())).sum().to(vt.dtype)
                vy = torch.zeros_like(yy) if vy is None else vy
                vp = [torch.zeros_like(p) if g is None else g for p, g in zip(params, vp)]
                return (vt, fe, vy, *vp)

            adj_options = dict(cfg["adjoint_options"])
            if adj_options.get("norm") == "seminorm":        # torchdiffeq: the parameter blocks stay out of the error norm
                adj_options["norm"] = lambda parts: max(parts[0].abs(), _rms(parts[1]), _rms(parts[2]))
            if cfg["adjoint_method"] == "dopri5" and "norm" not in adj_options:
                def adjoint_norm(parts):
                    tt, yy, aa, *pp = parts
                    extra = max([_rms(p) for p in pp]) if pp else 0.0
                    return max(tt.abs(), _rms(yy), _rms(aa), extra)
                adj_options["norm"] = adjoint_norm
            time_vjps = [None] * len(t)
            for i in range(len(t) - 1, 0, -1):
                if need_t:                       # the effect of moving this output time: dL/dt_i = f(t_i, y_i) . dL/dy_i
                    dldt = (func(t[i].to(y.dtype), y[i]) * grad_y[i]).sum()
                    aug[0] = aug[0] - dldt
                    time_vjps[i] = dldt
                sol = odeint(dynamics, tuple(aug), t[i - 1:i + 1].flip(0), method=cfg["adjoint_method"],
                             options=adj_options, rtol=cfg["adjoint_rtol"], atol=cfg["adjoint_atol"])
                aug = [s[1] for s in sol]
                aug[1] = y[i - 1]
                aug[2] = aug[2] + grad_y[i - 1]
            grad_t = None
            if need_t:
                time_vjps[0] = aug[0]
                grad_t = torch.stack([v.to(t.dtype) for v in time_vjps]) if len(t) > 1 else torch.zeros_like(t)
        return (None, aug[2], grad_t, *aug[3:])


# ------------------------------------------------------------------------------------------ reversible Heun
# backend="torchsde", method="reversible_heun" (arXiv 2105.13493, Algorithms 1 and 2; semantics: DESIGN.md section 8) for
# everything the fused kernels (csrc/revheun.hip) do not take.  State (y, zh, f), zh_0 = y_0, f_0 = F(t_0, y_0); per step
#     zh' = 2 y - zh + f dt;   f' = F(t', zh');   y' = y + (f + f') dt/2
# with dt = grid[k+1] - grid[k] rounded once to the state's dtype and used identically in both directions.
def _revheun_outputs(grid, t_host):
    """Per output time (node k, slope): y_k itself (slope None) or y_k + slope (y_{k+1} - y_k) -- the walk over
    (grid, t) that _solve_fixed and the fused kernels make."""
    outs, j = [(0, None)], 1
    for k, (t0, t1) in enumerate(zip(grid[:-1], grid[1:])):
        while j < len(t_host) and bool(t1 >= t_host[j]):
            tj = t_host[j]
            if bool(tj == t0):
                outs.append((k, None))
            elif bool(tj == t1):
                outs.append((k + 1, None))
            else:
                outs.append((k, (tj - t0) / (t1 - t0)))
            j += 1
    if len(outs) != len(t_host):
        raise NotImplementedError("torchcde_amd: method='reversible_heun' needs non-decreasing output times")
    return outs


def _revheun_forward(f, y0, times, dts, outs):
    """The forward recurrences; returns (outputs stacked over the output times, y_N, zh_N)."""
    on_node, in_step = {}, {}
    for j, (k, slope) in enumerate(outs):
        (on_node if slope is None else in_step).setdefault(k, []).append((j, slope))
    result = [None] * len(outs)
    y = zh = y0
    for j, _ in on_node.get(0, ()):
        result[j] = y
    if dts:
        fk = f(times[0], zh)
    for k, dt in enumerate(dts):
        zh = 2 * y - zh + fk * dt
        f1 = f(times[k + 1], zh)
        y1 = y + (fk + f1) * (0.5 * dt)
        for j, slope in in_step.get(k, ()):
            result[j] = y + float(slope.to(y0.dtype)) * (y1 - y)
        for j, _ in on_node.get(k + 1, ()):
            result[j] = y1
        y, fk = y1, f1
    return torch.stack(result), y, zh


class _ReversibleHeun(torch.autograd.Function):
    """The exact gradient of the discrete reversible Heun solve from (y_N, zh_N) alone: the backward pass walks the nodes
    N .. 0, rebuilds the state by inverting the steps and differentiates them -- one field evaluation and one
    vector-Jacobian product per node (closed form for a recognised field, autograd otherwise).  With dt = dt_{k-1}:
        a = fbar_k + ybar_k dt/2;   f_k, v, dtheta = F, (dF/dz)^T a, (dF/dtheta)^T a  at (t_k, zh_k)
        y_k = y_{k+1} - (f_k + f_{k+1}) dt_k/2   (y lags one node: it needs f_k)
        zt = zbar_k + v;   fbar_{k-1} = ybar_k dt/2 + zt dt;   ybar_{k-1} = ybar_k + 2 zt + (outputs on node k-1)
        zbar_{k-1} = -zt;  zh_{k-1} = 2 y_k - zh_k - f_k dt
    and node 0 is evaluated at zh_0 (= y_0) with cotangent fbar_0: dL/dy_0 = ybar_0 + zbar_0 + v."""

    @staticmethod
    def forward(ctx, cfg, y0, *params):
        with torch.no_grad():
            out, y_last, zh_last = _revheun_forward(cfg["func"], y0, cfg["times"], cfg["dts"], cfg["outs"])
        ctx.cfg = cfg
        ctx.save_for_backward(y_last, zh_last, *params)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        cfg = ctx.cfg
        func, times, dts = cfg["func"], cfg["times"], cfg["dts"]
        y, zh, *params = ctx.saved_tensors
        params = tuple(params)
        n = len(dts)
        landing = [[] for _ in range(n + 1)]          # the transpose of the output interpolation
        for j, (k, slope) in enumerate(cfg["outs"]):
            if slope is None:
                landing[k].append((j, None))
            else:
                s = float(slope.to(y.dtype))
                landing[k].append((j, float(torch.ones((), dtype=y.dtype) - slope.to(y.dtype))))
                landing[k + 1].append((j, s))

        def outputs_on(k, g):
            for j, w in landing[k]:
                g = g + (grad_out[j] if w is None else w * grad_out[j])
            return g

        with torch.no_grad():
            explicit = _explicit_dynamics(func, params)

            def node(tt, z, cot):
                if explicit is not None:
                    return explicit(tt, z, -cot)                # (written for the cotangent -a of the continuous adjoint)
                with torch.enable_grad():
                    zz = z.detach().requires_grad_(True)
                    fe = func(tt, zz)
                    vz, *vp = torch.autograd.grad(fe, (zz,) + params, cot, allow_unused=True, retain_graph=True)
                vz = torch.zeros_like(z) if vz is None else vz
                return fe.detach(), vz, [torch.zeros_like(p) if g is None else g for p, g in zip(params, vp)]

            grads = [torch.zeros_like(p) for p in params]
            ybar = outputs_on(n, torch.zeros_like(y))
            zbar, fbar = torch.zeros_like(y), torch.zeros_like(y)
            f_next = None
            for k in range(n, 0, -1):
                dt = dts[k - 1]
                fk, v, dp = node(times[k], zh, fbar + ybar * (0.5 * dt))
                grads = [g + d for g, d in zip(grads, dp)]
                if f_next is not None:
                    y = y - (fk + f_next) * (0.5 * dts[k])
                zt = zbar + v
                fbar = ybar * (0.5 * dt) + zt * dt
                ybar = outputs_on(k - 1, ybar + 2 * zt)
                zbar = -zt
                zh = 2 * y - zh - fk * dt
                f_next = fk
            _, v, dp = node(times[0], zh, fbar)
            grads = [g + d for g, d in zip(grads, dp)]
        return (None, ybar + zbar + v, *grads)


def solve_reversible_heun(X, func, z0, t, dt, adjoint, adjoint_params, field=None, recognised=None, through=False):
    """Step-wise cdeint(..., backend="torchsde", method="reversible_heun", dt=dt): returns (..., len(t), H).  Gradients of z0
    and the parameters (`adjoint_params`, or func's own) come from the reconstructing backward pass; `through`: plain
    autograd through the host-driven steps instead (adjoint=False with control tensors -- or anything else outside func's
    parameters -- that requires a gradient)."""
    if field is None:
        field = ControlledField(X, func)
        field.recognised = recognised
    t_host = t.detach().cpu()
    grid = _grid(t_host, dt)
    outs = _revheun_outputs(grid, t_host)
    times = grid.to(z0.device).to(z0.dtype)
    dts = [float(d) for d in (grid[1:] - grid[:-1]).to(z0.dtype)]
    if through or not torch.is_grad_enabled():
        out = _revheun_forward(field, z0, times, dts, outs)[0]
    else:
        if adjoint_params is None:
            if not isinstance(func, torch.nn.Module):
                if adjoint:
                    raise ValueError("func must be an instance of nn.Module to specify the adjoint parameters; alternatively "
                                     "they can be specified explicitly via the `adjoint_params` argument. If there are no "
                                     "parameters then it is allowable to set `adjoint_params=()`.")
                adjoint_params = ()
            else:
                adjoint_params = tuple(func.parameters())
        params = tuple(p for p in adjoint_params if isinstance(p, torch.Tensor) and p.requires_grad)
        cfg = dict(func=field, times=times, dts=dts, outs=outs)
        out = _ReversibleHeun.apply(cfg, z0, *params)
    lead = range(1, out.dim() - 1)
    return out.permute(*lead, 0, -1)


class TupleField:
    """Tuple state (reference solver.py:68-95, :131-133): z = (z_1, .., z_k), X.derivative(t) = (dX_1, .., dX_k), func
    returns one (.., H_i, C_i) matrix per component (or func.prod the products).  torchdiffeq solves such systems on
    the concatenated state; so does this wrapper (components are concatenated along the hidden axis)."""

    def __init__(self, X, func, sizes):
        self.X, self.func, self.sizes = X, func, tuple(sizes)

    def __call__(self, t, z):
        parts = z.split(self.sizes, dim=-1)
        dX = self.X.derivative(t.detach())
        if hasattr(self.func, "prod"):
            out = self.func.prod(t, parts, dX)
        else:
            out = tuple(_Contract.apply(f, d) for f, d in zip(self.func(t, parts), dX))
        return torch.cat(tuple(out), dim=-1)

    def time_partial(self, t, z):
        with torch.no_grad():
            parts = z.split(self.sizes, dim=-1)
            d2X = self.X._second_derivative(t.detach())
            if hasattr(self.func, "prod"):
                out = self.func.prod(t, parts, d2X)
            else:
                out = tuple(_Contract.apply(f, d) for f, d in zip(self.func(t, parts), d2X))
            return torch.cat(tuple(out), dim=-1)


def solve(X, func, z0, t, adjoint, method, options, rtol, atol, adjoint_method, adjoint_options, adjoint_rtol,
          adjoint_atol, adjoint_params, field=None, recognised=None):
    """Step-wise cdeint: returns (..., len(t), H) like the fused path.  `recognised`: the probe's verdict on func
    (fields.AffineField / MLPField) when its formula is known -- the adjoint then evaluates its dynamics in closed
    form (`_explicit_dynamics`)."""
    if field is None:
        field = ControlledField(X, func)
        field.recognised = recognised
    t = t.to(z0.device)
    if adjoint:
        if adjoint_params is None:
            if not isinstance(func, torch.nn.Module):
                raise ValueError("func must be an instance of nn.Module to specify the adjoint parameters; alternatively "
                                 "they can be specified explicitly via the `adjoint_params` argument. If there are no "
                                 "parameters then it is allowable to set `adjoint_params=()`.")
            adjoint_params = tuple(func.parameters())
        params = tuple(p for p in adjoint_params if p.requires_grad)
        fixed_opts = {k: v for k, v in (options or {}).items() if k != "norm"}
        cfg = dict(func=field, method=method, options=options, rtol=rtol, atol=atol,
                   adjoint_method=adjoint_method or method,
                   adjoint_options=fixed_opts if adjoint_options is None else dict(adjoint_options),
                   adjoint_rtol=adjoint_rtol, adjoint_atol=adjoint_atol,
                   t_requires_grad=bool(t.requires_grad and torch.is_grad_enabled()))
        out = _Adjoint.apply(cfg, z0, t, *params)
    else:
        if isinstance(field, ControlledField):
            field.through_time = bool(torch.is_grad_enabled() and t.requires_grad)
        out = odeint(field, z0, t, method=method, options=options, rtol=rtol, atol=atol)
    lead = range(1, out.dim() - 1)
    return out.permute(*lead, 0, -1)
