"""Timing and backward-pass memory of the reversible Heun solve (backend="torchsde", method="reversible_heun") on the full-size
workload (B=32768, L=128, C=8, H=32, dt = 1), next to the fixed-grid solves of the same build: midpoint (identity field:
the only field it is fused for) and rk4 with adjoint=True / adjoint=False.  Forward only, forward + backward, and the peak
memory of forward + backward over what is allocated before the solve (torch.cuda.max_memory_allocated).

    python scripts/bench_reversible_heun.py [--batch 32768] [--length 128] [--reps 5]
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import torchcde_amd as native  # noqa: E402
from helpers import LinearField, make_series  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32768)
    ap.add_argument("--length", type=int, default=128)
    ap.add_argument("--channels", type=int, default=8)
    ap.add_argument("--hidden", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, L, C, H = args.batch, args.length, args.channels, args.hidden
    x = make_series(B, L, C).to(dev)
    X = native.CubicSpline(native.hermite_cubic_coefficients_with_backward_differences(x))
    z0 = torch.randn(B, H, device=dev)
    fields = {"tanh": LinearField(H, C, scale=1.0, tanh=True, seed=0).to(dev),
              "identity": LinearField(H, C, scale=0.5, seed=0).to(dev)}
    rk4 = dict(method="rk4", options=dict(step_size=1.0))
    rows = [
        ("reversible_heun", "tanh", dict(backend="torchsde", method="reversible_heun", dt=1.0)),
        ("reversible_heun", "identity", dict(backend="torchsde", method="reversible_heun", dt=1.0)),
        ("midpoint", "identity", dict(method="midpoint", options=dict(step_size=1.0))),
        ("rk4 adjoint=True", "tanh", dict(adjoint=True, **rk4)),
        ("rk4 adjoint=False", "tanh", dict(adjoint=False, **rk4)),
        ("rk4 adjoint=True", "identity", dict(adjoint=True, **rk4)),
        ("rk4 adjoint=False", "identity", dict(adjoint=False, **rk4)),
    ]
    for name, field, kw in rows:
        func = fields[field]

        def forward():
            with torch.no_grad():
                native.cdeint(X, func, z0, X.interval, **kw)

        def both():
            z = z0.clone().requires_grad_(True)
            out = native.cdeint(X, func, z, X.interval, **kw)
            out[:, -1].sum().backward()

        def timed(step):
            step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.reps):
                step()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / args.reps * 1e3

        fwd, fb = timed(forward), timed(both)
        path = sys.modules["torchcde_amd.cdeint"].last_dispatch()[0].path
        for p in func.parameters():
            p.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        both()
        torch.cuda.synchronize()
        peak = (torch.cuda.max_memory_allocated() - before) / 2 ** 20
        print(f"{name:18s} {field:8s} path={path:16s} forward {fwd:7.2f} ms   forward+backward {fb:7.2f} ms   "
              f"peak memory of forward+backward {peak:8.1f} MiB", flush=True)


if __name__ == "__main__":
    main()
