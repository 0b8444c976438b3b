"""The inputs of tests/test_gpu_24_irregular_knots.py, judged without a GPU (tests/irregular_controls.py): for every case of the
table

  * the inputs are fair: the oracle run in float32 on the CPU stays within 1e-5 of the largest entry of the float64 result on
    the trajectory and on every gradient -- no relu unit sits on its kink, float32 is a meaningful yardstick, and on gradients
    the 1e-3 term of the GPU test's bar decides.  A condition on the draw, not a tolerance: a case that misses it gets another
    series seed (irregular_controls.SEEDS), never a wider cap;
  * the inputs have teeth: a solve that pairs every linear slope with the next interval's width, and one that reads the same
    coefficients on uniform knots, each differ from the true float64 solve by at least 10 x the GPU test's bar at its widest
    (atol + rtol max|want|), on the trajectory and on dL/dz0.

Each case prints its float32 deviation (as a fraction of the largest entry) and each mutant's distance as a multiple of the bar.
"""
import pytest

import irregular_controls as ic

FAIR = 1e-5
TEETH = 10.0


@pytest.mark.parametrize("case", ic.ALL_CASES, ids=ic.case_id)
def test_inputs_are_fair_and_have_teeth(case):
    ref = ic.reference(case)
    want, cpu32 = ref["f64"], ref["f32"]
    worst = {name: ic.cpu32_error(ref, name) / want[name].abs().max().item() for name in cpu32}
    print("%s: max|z| %.3g; float32 oracle / largest entry: %s" % (
        ic.case_id(case), want["out"].abs().max().item(), ", ".join("%s %.2g" % kv for kv in worst.items())))
    multiples = {}
    for which, run in ic.mutants(case).items():
        for name, bar in (("out", ic.out_bar(case, ref)), ("z", ic.grad_bar(case, ref, "z"))):
            multiples[which, name] = (run[name] - want[name]).abs().max().item() / ic.widest(bar, want[name])
    print("    mutants / bar: %s" % ", ".join("%s %s %.3g" % (k + (v,)) for k, v in multiples.items()))
    assert set(cpu32) == (set(want) if case.family != "revheun" else {"out"})
    for name, share in worst.items():
        assert share <= FAIR, "float32 oracle off by %.3g of the largest entry on %s: move this case's series seed" % (share, name)
    assert set(multiples) == {(w, n) for w in (("uniform_knots", "shifted_widths") if case.degree == 1 else ("uniform_knots",))
                              for n in ("out", "z")}
    for key, multiple in multiples.items():
        assert multiple >= TEETH, "%s on %s is only %.3g x the bar away from the true solve" % (key + (multiple,))
    if case.family == "mlp2":
        # the row that also runs with adjoint=False: autograd through the oracle's steps is its reference
        ref = ic.reference(case, adjoint=False)
        worst = {name: ic.cpu32_error(ref, name) / ref["f64"][name].abs().max().item() for name in ref["f32"]}
        print("    adjoint=False, float32 oracle / largest entry: %s" % ", ".join("%s %.2g" % kv for kv in worst.items()))
        assert set(worst) == set(want) and max(worst.values()) <= FAIR, worst
