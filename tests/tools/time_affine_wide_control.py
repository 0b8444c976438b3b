"""Times cdeint(method="rk4") of the one-layer field Linear(H, H C) (+ tanh) on controls of 21 and 64 channels: forward, and
forward + backward (adjoint=True), at 4096 and 32768 series -- the default kernels (variant "auto": K2c / K3c of
csrc/rk4_affine_tiled.hip inside their envelope) against variant="generic", the VALU kernels, in the same process.

    python tests/tools/time_affine_wide_control.py [--batches 4096 32768] [--channels 21 64] [--repeats 3] [--limit SECONDS]

H = 32, L = 65 knots, cubic control, step_size = 1 (64 steps).  Every timed step -- one (C, B, activation, variant, direction)
-- runs in a child process of its own under `timeout`, so a step that takes too long ends alone and is printed as "timeout";
a child that ends in any other way than with a figure ends the run.  Each figure is the median of `repeats` timed calls after
one warm-up call, every call ended by a device synchronise.  One table at the end, milliseconds.
"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
H, L = 32, 65


def measure(C, B, tanh, variant, train, repeats):
    import torch
    sys.path.insert(0, ROOT)
    import torchcde_amd
    front = importlib.import_module("torchcde_amd.cdeint")
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    torchcde_amd.load()
    warnings.simplefilter("ignore")

    class Field(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.linear = torch.nn.Linear(H, H * C)

        def forward(self, t, z):
            y = self.linear(z)
            return (y.tanh() if tanh else y).view(*z.shape[:-1], H, C)

    torch.manual_seed(C)
    x = torch.randn(B, L, C, device="cuda").cumsum(1) * 0.1
    X = torchcde_amd.CubicSpline(torchcde_amd.hermite_cubic_coefficients_with_backward_differences(x))
    func = Field().cuda()
    with torch.no_grad():                                                       # pre-activations of order 1 over the solve
        func.linear.weight.mul_(0.4 / C ** 0.5)
        func.linear.bias.mul_(0.4 / C ** 0.5)
    z0 = torch.randn(B, H, device="cuda")
    kw = dict(method="rk4", options=dict(step_size=1.0), variant=variant)

    def forward():
        with torch.no_grad():
            return torchcde_amd.cdeint(X, func, z0, X.interval, **kw)

    def backward():
        z = z0.clone().requires_grad_(True)
        func.zero_grad()
        torchcde_amd.cdeint(X, func, z, X.interval, **kw)[:, -1].square().sum().backward()

    call = backward if train else forward
    call()                                                                      # warm-up: code objects, allocator, plans
    torch.cuda.synchronize()
    choice = front.last_dispatch()[0]
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    print(json.dumps(dict(seconds=statistics.median(times), path=choice.path, family=getattr(choice, "family", ""))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[4096, 32768])
    ap.add_argument("--channels", type=int, nargs="+", default=[21, 64])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--limit", type=int, default=120, help="seconds per timed step")
    ap.add_argument("--child", nargs=5, metavar=("C", "B", "TANH", "VARIANT", "TRAIN"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        C, B, tanh, variant, train = args.child
        return measure(int(C), int(B), tanh == "1", variant, train == "1", args.repeats)
    rows = []
    for C in args.channels:
        for B in args.batches:
            for tanh in (False, True):
                row = dict(C=C, B=B, act="tanh" if tanh else "identity")
                for train in (False, True):
                    for variant in ("auto", "generic"):
                        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--repeats",
                               str(args.repeats), "--child", str(C), str(B), "1" if tanh else "0", variant, "1" if train else "0"]
                        proc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
                        key = ("train_" if train else "forward_") + variant
                        if proc.returncode == 124:
                            row[key] = "timeout"
                        elif proc.returncode != 0:
                            print(proc.stdout[-4000:])
                            sys.exit("the step %s ended with status %d: nothing more is started" % (cmd[-5:], proc.returncode))
                        else:
                            got = json.loads(proc.stdout.strip().splitlines()[-1])
                            row[key] = "%.2f" % (1e3 * got["seconds"])
                            if variant == "auto":
                                row["family"] = got["family"] or "-"
                        print(json.dumps(row), flush=True)
                rows.append(row)
    cols = ["C", "B", "act", "family", "forward_auto", "forward_generic", "train_auto", "train_generic"]
    print("\n" + " | ".join("%15s" % c for c in cols))
    for row in rows:
        print(" | ".join("%15s" % row.get(c, "") for c in cols))


if __name__ == "__main__":
    main()
