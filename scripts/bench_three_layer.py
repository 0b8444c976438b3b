"""One rk4 training step (forward + adjoint=True backward, step_size 1) of the three-layer field
Linear(32, w) -> relu -> Linear(w, w) -> relu -> Linear(w, 256) -> tanh at 4096 series x 128 knots x 8 channels: fused, step-wise
as `variant="generic"` runs it, the two-layer field of the same width for comparison, the identity-activation field, and the
three factor reductions of one sweep chunk on their own (profiles/NOTES.md, the three-layer section).

    python scripts/bench_three_layer.py [--batch 4096] [--length 128] [--width 128] [--reps 5]
    python scripts/bench_three_layer.py --plain-call-only [--library PATH]

--plain-call-only times nothing but `cdeint(X, func, z0, t, method="rk4", options=dict(step_size=1.0))` of the three-layer
module and prints the path it took: run from a checkout of an EARLIER commit (this file copied next to it), that is the time
the module took there -- step-wise, before the field was recognised.  --library names a built libcde_mi355x.so to load when
that checkout has none of its own (the step-wise path uses the control-derivative and contraction kernels only)."""
import argparse
import os
import sys
import time
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))


class Field(torch.nn.Module):
    """`widths` = (w,): the examples' two-layer field; (w1, w2): one layer deeper."""

    def __init__(self, H, C, widths, final_tanh=True):
        super().__init__()
        self.H, self.C, self.final_tanh = H, C, final_tanh
        sizes = (H,) + tuple(widths) + (H * C,)
        self.layers = torch.nn.ModuleList(torch.nn.Linear(a, b) for a, b in zip(sizes[:-1], sizes[1:]))

    def forward(self, t, z):
        for lin in self.layers[:-1]:
            z = lin(z).relu()
        y = self.layers[-1](z)
        return (y.tanh() if self.final_tanh else y).view(*z.shape[:-1], self.H, self.C)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--length", type=int, default=128)
    ap.add_argument("--width", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--plain-call-only", action="store_true")
    ap.add_argument("--library", default=None)
    args = ap.parse_args()
    import torchcde_amd as native
    from torchcde_amd import _lib
    from helpers import make_series
    if args.library:
        _lib.SO_PATH = os.path.abspath(args.library)
    front = sys.modules["torchcde_amd.cdeint"]
    dev = torch.device("cuda:0")
    B, L, C, H, w = args.batch, args.length, 8, 32, args.width
    X = native.CubicSpline(native.hermite_cubic_coefficients_with_backward_differences(make_series(B, L, C, seed=1).to(dev)))
    z0 = torch.randn(B, H, generator=torch.Generator().manual_seed(2)).to(dev)

    def timed(label, func, reps, grad=True, **kw):
        def step():
            func.zero_grad()
            z = z0.clone().requires_grad_(grad)
            with torch.set_grad_enabled(grad):
                out = native.cdeint(X, func, z, X.interval, method="rk4", options=dict(step_size=1.0), **kw)
            path = front.last_dispatch()[0].path
            if grad:
                out[:, -1].sum().backward()
            return path
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            step()                                                # untimed
            torch.cuda.synchronize()
            times = []
            for _ in range(reps):
                t0 = time.perf_counter()
                path = step()
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t0) * 1e3)
        print("%-46s %-16s %s ms" % (label, path, " ".join("%.2f" % t for t in times)), flush=True)

    torch.manual_seed(5)
    three = Field(H, C, (w, w)).to(dev)
    if args.plain_call_only:
        timed("three-layer, the plain call of this checkout", three, max(1, min(args.reps, 3)))
        return
    two = Field(H, C, (w,)).to(dev)
    three_id = Field(H, C, (w, w), final_tanh=False).to(dev)
    timed("three-layer, training step", three, args.reps)
    timed("three-layer, forward solve (no_grad)", three, args.reps, grad=False)
    timed("three-layer identity activation, training step", three_id, args.reps)
    timed("two-layer, training step", two, args.reps)
    timed("two-layer, forward solve (no_grad)", two, args.reps, grad=False)
    timed("three-layer, variant='generic' training step", three, min(args.reps, 3), variant="generic")

    # the three reductions behind one sweep chunk at the default scratch budget, each on its own
    lib = _lib.load()
    row_bytes = (132 + 132 + 256 + 256 + 128 + 36) * 4
    chunk = max(1, min(L - 1, front._MlpPlan.scratch_budget // (row_bytes * 4 * B)))
    rows = chunk * 4 * B
    ws = torch.empty(lib.cde_mlp_grad_reduce_workspace_bytes(), dtype=torch.uint8, device=dev)
    stream = _lib.stream_ptr(dev)
    print("one sweep chunk: %d steps = %d factor rows (%d chunks per solve)" % (chunk, rows, -(-(L - 1) // chunk)))
    for label, g_cols, x_cols, layer, acc_shape in (("G2^T U   (256 x 132)", 256, 132, 2, (256, 132)),
                                                    ("Gm^T U1  (Gm padded to 256 columns)", 256, 132, 2, (256, 132)),
                                                    ("G1^T Z   (128 x 36)", 128, 36, 1, (128, 36))):
        G = torch.randn(rows, g_cols, device=dev)
        Xf = torch.randn(rows, x_cols, device=dev)
        acc = torch.zeros(acc_shape, device=dev)
        times = []
        for i in range(4):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            _lib.check(lib.cde_mlp_grad_reduce(_lib.ptr(G), _lib.ptr(Xf), rows, layer, _lib.ptr(acc), _lib.ptr(ws), ws.numel(),
                                               stream), "cde_mlp_grad_reduce")
            b.record()
            torch.cuda.synchronize()
            if i:
                times.append(a.elapsed_time(b))
        print("reduction %-40s %s ms per chunk" % (label, " ".join("%.3f" % t for t in times)), flush=True)
        del G, Xf


if __name__ == "__main__":
    main()
