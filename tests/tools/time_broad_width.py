"""Times cdeint(method="rk4") of the examples' two-layer field at twice its inner width (256) on controls of 8 and 32 channels:
forward, and forward + backward (adjoint=True).  Public API only, so the same file runs on a commit that solves these shapes
step-wise and on one that fuses them; the dispatch verdict is printed with every row.

    python tests/tools/time_broad_width.py [--rows 8:4096 8:32768 32:4096] [--repeats 5] [--budget SECONDS] [--as-parent]

H = 32, width 256, L = 65 knots, cubic control, step_size = 1 (64 steps), final tanh, hidden relu.  Each figure is the median
of `repeats` timed calls after one warm-up call, every call ended by a device synchronise; the fastest and slowest call are
printed beside it.  `--budget`: stop timing a row after that many seconds (at least the warm-up and one timed call are made;
the count is printed).  `--as-parent`: take the broad-inner-layer predicate out of the dispatch, which leaves the call exactly
where a commit without these kernels has it -- kind "mlp2" beyond the tiles, step-wise with the closed-form adjoint.  One JSON
line per row.
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torchcde_amd                                                            # noqa: E402
front = importlib.import_module("torchcde_amd.cdeint")                         # (the package attribute is the function)

H, WIDTH, L = 32, 256, 65


class Field(torch.nn.Module):
    def __init__(self, C):
        super().__init__()
        self.C = C
        self.linear1 = torch.nn.Linear(H, WIDTH)
        self.linear2 = torch.nn.Linear(WIDTH, H * C)

    def forward(self, t, z):
        return self.linear2(self.linear1(z).relu()).tanh().view(*z.shape[:-1], H, self.C)


def timed(call, repeats, budget):
    call()                                                                      # warm-up: code objects, allocator, plans
    torch.cuda.synchronize()
    times, begin = [], time.perf_counter()
    while len(times) < repeats and (not times or time.perf_counter() - begin < budget):
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return dict(median=statistics.median(times), fastest=min(times), slowest=max(times), calls=len(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", nargs="+", default=["8:4096", "8:32768", "32:4096"], help="C:B pairs")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--budget", type=float, default=60.0)
    ap.add_argument("--as-parent", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    torchcde_amd.load()
    warnings.simplefilter("ignore")
    if args.as_parent and hasattr(front, "_mlp_broad_fusable"):
        front._mlp_broad_fusable = lambda *a, **k: False
    for C, B in (map(int, row.split(":")) for row in args.rows):
        torch.manual_seed(C)
        x = torch.randn(B, L, C, device="cuda").cumsum(1) * 0.1
        X = torchcde_amd.CubicSpline(torchcde_amd.hermite_cubic_coefficients_with_backward_differences(x))
        func = Field(C).cuda()
        z0 = torch.randn(B, H, device="cuda")
        kw = dict(method="rk4", options=dict(step_size=1.0))

        def forward():
            with torch.no_grad():
                return torchcde_amd.cdeint(X, func, z0, X.interval, **kw)

        def train():
            z = z0.clone().requires_grad_(True)
            func.zero_grad()
            out = torchcde_amd.cdeint(X, func, z, X.interval, **kw)
            train.plan = getattr(out.grad_fn, "plan", None)
            out[:, -1].square().sum().backward()

        row = dict(C=C, B=B, H=H, width=WIDTH, steps=L - 1, as_parent=args.as_parent)
        row["forward"] = timed(forward, args.repeats, args.budget)
        choice, request = front.last_dispatch()
        row["forward_path"], row["kind"] = choice.path, request.kind
        row["train"] = timed(train, args.repeats, args.budget)
        row["train_path"] = front.last_dispatch()[0].path
        row["steps_per_sweep_launch"] = getattr(train.plan, "steps_per_launch", None)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
