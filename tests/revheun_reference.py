"""The reversible Heun method (arXiv 2105.13493, Algorithm 1) restated in plain torch: what every number of
cdeint(..., backend="torchsde", method="reversible_heun") is compared against (torchsde itself is not a dependency).

    grid    t[0] + k dt, the last point replaced by t[-1] (the fixed-step grid of both back ends)
    state   (y, zh, f):  zh_0 = y_0 = z0,  f_0 = F(t_0, z0),  F(t, z) = func(t, z) . dX/dt(t)
    step    zh' = 2 y - zh + f dt;   f' = F(t', zh');   y' = y + (f + f') dt/2        (dt = grid[k+1] - grid[k])
    output  y at the output times, linear between grid points

The recurrences are ordinary differentiable torch operations, so autograd through them is the gradient of the discrete solve
-- the quantity the reconstructing backward passes return."""
import math

import torch


def grid_of(t, dt):
    """Python floats: t[0] + k dt for k < n - 1, then t[-1], with n = ceil((t[-1] - t[0]) / dt + 1)."""
    t0, t1 = float(t[0]), float(t[-1])
    n = int(math.ceil((t1 - t0) / dt + 1))
    return [t0 + k * dt for k in range(n - 1)] + [t1]


def controlled(X, func):
    """(t, z) -> func(t, z) . dX/dt(t) over an oracle path (oracle.interp.CubicPath / LinearPath) or anything with `derivative`."""
    def field(t, z):
        return (func(t, z) @ X.derivative(t).unsqueeze(-1)).squeeze(-1)
    return field


def nodes(field, z0, grid):
    """y at every grid node (a list of tensors shaped like z0) and zh at the last one."""
    at = lambda v: torch.tensor(v, dtype=z0.dtype)
    y, zh = z0, z0
    f = field(at(grid[0]), zh)
    ys = [y]
    for a, b in zip(grid[:-1], grid[1:]):
        dt = float(torch.tensor(b - a, dtype=z0.dtype))
        zh = 2 * y - zh + f * dt
        f1 = field(at(b), zh)
        y = y + (f + f1) * (0.5 * dt)
        f = f1
        ys.append(y)
    return ys, zh


def solve(X, func, z0, t, dt):
    """(..., len(t), H): the solution at the (increasing) output times `t`."""
    grid = grid_of(t, dt)
    ys, _ = nodes(controlled(X, func), z0, grid)
    out, k = [], 0
    for tj in (float(v) for v in t):
        while k + 1 < len(grid) - 1 and grid[k + 1] <= tj:
            k += 1
        if tj == grid[k] or len(grid) == 1:
            out.append(ys[k])
        elif tj == grid[k + 1]:
            out.append(ys[k + 1])
        else:
            slope = float(torch.tensor((tj - grid[k]) / (grid[k + 1] - grid[k]), dtype=z0.dtype))
            out.append(ys[k] + slope * (ys[k + 1] - ys[k]))
    return torch.stack(out, dim=-2)
