"""Fused time of the two-layer field with a softplus hidden layer against the relu field: the example model's shape
(C=8, H=32, width 128, cubic control of length 7 -> tests' `example_model`) at 4096 series, rk4 forward + adjoint.

    python scripts/bench_softplus.py [--batch 4096] [--length 7] [--reps 20]
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import torchcde_amd as native  # noqa: E402
from helpers import make_series  # noqa: E402


class TwoLayer(torch.nn.Module):
    def __init__(self, H, C, width, hidden):
        super().__init__()
        self.H, self.C, self.hidden = H, C, hidden
        self.linear1, self.linear2 = torch.nn.Linear(H, width), torch.nn.Linear(width, H * C)

    def forward(self, t, z):
        return self.linear2(self.hidden(self.linear1(z))).tanh().view(*z.shape[:-1], self.H, self.C)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--length", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, L, C, H, width = args.batch, args.length, 8, 32, 128
    X = native.CubicSpline(native.hermite_cubic_coefficients_with_backward_differences(make_series(B, L, C).to(dev)))
    z0 = torch.randn(B, H, device=dev)
    for name, hidden in (("relu", torch.relu), ("softplus", torch.nn.functional.softplus), ("relu", torch.relu),
                         ("softplus", torch.nn.functional.softplus)):
        torch.manual_seed(0)
        func = TwoLayer(H, C, width, hidden).to(dev)

        def step():
            z = z0.clone().requires_grad_(True)
            out = native.cdeint(X, func, z, X.interval, method="rk4", options=dict(step_size=1.0))
            out[:, -1].sum().backward()
        for _ in range(3):
            step()
        assert sys.modules["torchcde_amd.cdeint"].last_dispatch()[0].path == "mlp_rk4_adjoint"       # fused, not step-wise
        torch.cuda.synchronize()
        times = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            step()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        times.sort()
        print("%-8s rk4 fwd+adjoint, %d series x %d steps: median %.3f ms, min %.3f ms" % (
            name, B, L - 1, times[len(times) // 2], times[0]), flush=True)


if __name__ == "__main__":
    main()
