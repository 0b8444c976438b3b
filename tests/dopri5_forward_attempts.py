"""The attempt table of one adaptive FORWARD solve (csrc/dopri5.hip), read off the controller's status blocks.

The forward kernels trace their accepted steps only.  Everything else the controller does -- rejected attempts, the
step-size update, the clipping onto jump times, Hairer's first step -- is in the status block (`DopriStatus`,
include/cde_mi355x.h: cde_dopri5_status) that `_Dopri5Plan.run` (torchcde_amd/cdeint.py) reads back after every
`_DOPRI_CHUNK` launches.  With `_DOPRI_CHUNK = 1` the sequence of those blocks is the complete list of attempts; `run`
below patches the chunk (through `monkeypatch`, so it is per test) and wraps the module's `_status` to keep every block.

Launch <-> status <-> attempt (line numbers: torchcde_amd/csrc/dopri5.hip unless a file is named)
  * launch k runs on parity k & 1 (cde_launch.h:126-128): it reads controller block k & 1 and writes the other
    (:236-237 and :357-363 generic; :396, :407 the MFMA kernels), and leaves its workgroups' partial sums in the
    partial buffer of the block it writes (:245, :356).  `statuses[k]` is the block launch k wrote, `sums[k]` the two
    sums launch k left (cde_dopri5_pending_sums with total_launches = k + 1, :1251).
  * launch 0 (phase 0 -> 1, :118-129, :358): f(t0, y0); sums[0] = (sum (y0 / scale)^2, sum (f0 / scale)^2).
    launch 1 (phase 1 -> 2, :130-139): Hairer's h0 from those sums into `h0`; f(t0 + h0, y0 + h0 f0);
    sums[1][0] = sum ((f1 - f0) / scale)^2.
    launch 2 (phase 2 -> 3, :140-156): `dt` = Hairer's first step; the FIRST attempt [t_hi, t1_try] is planned
    (:204-216: `t1_try`, `dt_try`, `on_jump`) and made.
  * attempt j is made by launch 2 + j and decided by launch 3 + j (:157-192): statuses[2 + j] holds its plan,
    sums[2 + j][0] its error sum, statuses[3 + j] the decision (`n_accept` / `n_reject`, `t_lo`, `t_hi`, `i_out`, `i_jump`)
    and the next step size `dt` = dt_try * factor(ratio).
  * the launch that decides the last attempt finds every output written (:200-201), makes no new attempt and writes
    phase 4 (:361): a solve of N attempts is N + 3 launches, statuses[N + 2].phase == 4.

A row of the table: (t0, t1, on_jump, accepted, factor) =
  (statuses[2 + j].t_hi, statuses[2 + j].t1_try, statuses[2 + j].on_jump,
   statuses[3 + j].n_accept - statuses[2 + j].n_accept, statuses[3 + j].dt / statuses[2 + j].dt_try).

The pending sums are what the next launch adds up itself only where the kernel's grid is dopri_grid(form, n) (:1094-1096,
:1252).  The small-batch split forms (the eight waves of a workgroup share one 16-series tile: :1200-1201, :1214-1219,
:1236-1239) launch one workgroup per TILE, so cde_dopri5_pending_sums sees the first ceil(B / 128) tiles only: `run` takes
`read_sums=False` for them unless the batch is a single tile, and the ratio is recovered from `factor` instead
(`ratio_bounds`).
"""
import ctypes
import math

import torch

SAFETY, IFACTOR, DFACTOR = 0.9, 10.0, 0.2        # torchdiffeq's defaults (the calls of the tests pass none of them)
_CLAMP = 1e-12                                   # dt / dt_try is one float64 division away from the factor itself


class ForwardAttempts:
    """statuses, sums (None where not readable), rows (N, 5) float64, out, stats (last_dopri5_stats of the call)."""

    def __init__(self, statuses, sums, out, stats, n_elems, dtype):
        self.statuses, self.sums, self.out, self.stats, self.n_elems, self.dtype = statuses, sums, out, stats, n_elems, dtype
        n = len(statuses) - 3
        assert n >= 1, "no attempt was made (%d status blocks)" % len(statuses)
        rows = []
        for j in range(n):
            plan, done = statuses[2 + j], statuses[3 + j]
            rows.append((plan.t_hi, plan.t1_try, float(plan.on_jump), float(done.n_accept - plan.n_accept),
                         done.dt / plan.dt_try))
        self.rows = torch.tensor(rows, dtype=torch.float64)

    def __len__(self):
        return self.rows.size(0)

    def replay(self):
        """What the oracle's `replay_attempts` takes: (t0, t1, on_jump, accepted)."""
        return self.rows[:, :4].clone()

    def ratio(self, j):
        """The error ratio launch 3 + j decided attempt j on, as the kernel forms it (:159): sqrt(sum0 / (B H)) rounded to
        the state dtype.  Only where the sums are readable."""
        value = torch.tensor(math.sqrt(self.sums[2 + j][0] / self.n_elems), dtype=torch.float64)
        return float(value.to(self.dtype))

    def ratio_bounds(self, j):
        """[lo, hi] the kernel's ratio of attempt j lies in, from the step-size update alone (:181-190):
        factor = min(ifactor, max(safety / ratio^(1/5), ratio < 1 ? 1 : dfactor))."""
        factor = float(self.rows[j, 4])
        if abs(factor - 1.0) <= _CLAMP:
            return (SAFETY / 1.0) ** 5, 1.0
        if abs(factor - DFACTOR) <= _CLAMP * DFACTOR:
            return (SAFETY / DFACTOR) ** 5, math.inf
        if abs(factor - IFACTOR) <= _CLAMP * IFACTOR:
            return 0.0, (SAFETY / IFACTOR) ** 5
        r = (SAFETY / factor) ** 5
        return r, r


def next_factor(ratio):
    """torchdiffeq's _optimal_step_size (oracle/odeint.py: _next_dt) on a float64 ratio."""
    if ratio == 0:
        return IFACTOR
    return min(IFACTOR, max(SAFETY / ratio ** 0.2, 1.0 if ratio < 1 else DFACTOR))


def run(native, monkeypatch, front, X, func, z0, t_out, *, read_sums, mlp, tanh=False, variant="auto", chunk=1,
        record=True, path=None, **call):
    """One forward `native.cdeint` under no_grad with `_DOPRI_CHUNK = chunk`; returns its ForwardAttempts (chunk 1) or
    (out, stats) (any other chunk: the blocks in between are never read back).  `path`: the dispatch path the call must take."""
    from torchcde_amd import _lib
    lib = _lib.load()
    (B, H), C = z0.shape, func.C
    dtype = z0.dtype
    statuses, sums = [], []
    original = front._status
    size = ctypes.sizeof(_lib.DopriStatus)

    def status(workspace, at):
        block = original(workspace, at)
        statuses.append(block)
        launched = len(statuses)
        assert at == (launched & 1) * size                   # the block the last launch wrote
        if read_sums:
            pair = torch.zeros(2, dtype=torch.float64, device=workspace.device)
            head = (_lib.ptr(workspace), workspace.numel(), B, C, H, _lib.dtype_enum(dtype))
            stream = _lib.stream_ptr(workspace.device)
            if mlp:
                _lib.check(lib.cde_dopri5_pending_sums_mlp(*head, launched, _lib.ptr(pair), stream), "pending_sums_mlp")
            else:
                enum = {"auto": _lib.VARIANT_AUTO, "generic": _lib.VARIANT_GENERIC, "mfma": _lib.VARIANT_MFMA}[variant]
                act = _lib.ACT_TANH if tanh else _lib.ACT_NONE
                _lib.check(lib.cde_dopri5_pending_sums(*head, enum, act, launched, _lib.ptr(pair), stream), "pending_sums")
            sums.append(tuple(pair.cpu().tolist()))
        return block

    kw = dict(call)
    if variant != "auto":
        kw["variant"] = variant
    with monkeypatch.context() as patch:
        patch.setattr(front, "_DOPRI_CHUNK", chunk)
        if chunk == 1:
            patch.setattr(front, "_status", status)
        patch.setattr(front, "record_dopri5_steps", record)
        with torch.no_grad():
            out = native.cdeint(X, func, z0, t_out, **kw)
        stats = dict(front.last_dopri5_stats)
    if path is not None:
        choice = front.last_dispatch()[0]
        assert choice.path == path, "took %r (%s), not %r" % (choice.path, choice.reason, path)
    if chunk != 1:
        return out, stats
    return ForwardAttempts(statuses, sums if read_sums else None, out, stats, B * H, dtype)
