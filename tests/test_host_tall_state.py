"""The two-layer field on hidden states of 33 to 64 channels as far as it goes without a GPU: the dispatch rows of kind "mlp2h",
the envelope (host and library, and that at most one of the three two-layer envelopes claims a shape), the argument checks of
the new entry points, and a restatement of the index maps of csrc/cde_mlp_tiled.h -- layer 1 over K = 64, the four tiles of
va = W1^T g1, the state halves Z | Z_hi and the host's gather of dW1 | db1 -- against plain einsum at ragged shapes."""
import itertools

import numpy as np
import torch

import torchcde_amd
from torchcde_amd import _lib
from torchcde_amd import dispatch as D
from torchcde_amd.fields import probe
from rejected_calls import build_args
from helpers import TwoLayerField


# ------------------------------------------------------------------------------------------------ dispatch
def _ask(**kw):
    base = dict(prod=False, kind="mlp2h", tiles_ok=True, mfma_shape=False, method="rk4", adjoint=True, wants_grad=True,
                wants_t=False, wants_control=False, params="default", adjoint_method_ok=True, options_ok=True,
                adjoint_options_ok=True, t_ok=True, variant_generic=False, shared=False, narrow_control=False,
                backprop_ok=False, identity=False, control_block=False)
    base.update(kw)
    return D.select_path(D.Request(**base))


def test_dispatch_rows_of_the_tall_state_field():
    """select_path for kind "mlp2h" over every flag, three methods and the three parameter kinds (pruned as
    tests/test_host_wide_control.py prunes them).  Fused exactly under rk4 with step_size options, not generic, and either no
    gradient or adjoint=True with its method / options in range, own parameters, no time or control gradient; a reason with
    every step-wise verdict."""
    flags = ["prod", "tiles_ok", "adjoint", "wants_grad", "wants_t", "wants_control", "adjoint_method_ok", "options_ok",
             "adjoint_options_ok", "t_ok", "variant_generic", "shared", "narrow_control", "control_block"]
    seen = {}
    n = 0
    for method in ("rk4", "dopri5", "midpoint"):
        for params in ("default", "own", "foreign"):
            for bits in itertools.product((False, True), repeat=len(flags)):
                f = dict(zip(flags, bits))
                if (f["wants_t"] or f["wants_control"]) and not f["wants_grad"]:
                    continue
                if f["control_block"] and not (f["wants_control"] and f["adjoint"] and params == "own"):
                    continue
                q = D.Request(kind="mlp2h", method=method, params=params, mfma_shape=False, backprop_ok=False, identity=False, **f)
                c = D.select_path(q)
                n += 1
                seen[c.path] = seen.get(c.path, 0) + 1
                base = (not f["prod"] and f["tiles_ok"] and f["t_ok"] and method == "rk4" and f["options_ok"]
                        and not f["variant_generic"])
                want = D.STEPWISE
                if base and not f["wants_grad"]:
                    want = "mlp_rk4_forward"
                elif (base and f["adjoint"] and f["adjoint_method_ok"] and f["adjoint_options_ok"] and params != "foreign"
                      and not f["wants_t"] and not f["wants_control"]):
                    want = "mlp_rk4_adjoint"
                assert c.path == want, (q, c)
                assert (c.path == D.STEPWISE) == bool(c.reason)
                # row for row the verdict of the wide-control block
                assert c.path == D.select_path(q._replace(kind="mlp2w")).path
    assert n > 10000 and set(seen) == {"mlp_rk4_forward", "mlp_rk4_adjoint", D.STEPWISE}
    assert set(seen) - {D.STEPWISE} <= set(D.FUSED_PATHS)                     # no new path name
    assert len(D.FUSED_PATHS) == 10 and len(D.Request._fields) == 20          # nor a new field of the request

    assert _ask().path == "mlp_rk4_adjoint" and _ask(params="own").path == "mlp_rk4_adjoint"
    assert _ask(wants_grad=False).path == _ask(wants_grad=False, adjoint=False).path == "mlp_rk4_forward"
    # the default method first: its reason names the hidden-state size and what is fused for it
    default = _ask(method="dopri5")
    assert default.path == D.STEPWISE and "33 to 64" in default.reason and "rk4" in default.reason
    for kw in (dict(method="dopri5", wants_grad=False), dict(method="dopri5", shared=True), dict(method="midpoint"),
               dict(method="euler", wants_grad=False), dict(adjoint=False), dict(wants_t=True),
               dict(wants_control=True, params="own"), dict(params="foreign"), dict(adjoint_method_ok=False),
               dict(adjoint_options_ok=False), dict(options_ok=False)):
        verdict = _ask(**kw)
        assert verdict.path == D.STEPWISE and "33 to 64" in verdict.reason and "rk4" in verdict.reason, (kw, verdict)
    assert "generic" in _ask(variant_generic=True).reason
    assert "tiles" in _ask(tiles_ok=False).reason and "increasing" in _ask(t_ok=False).reason
    # nothing moved for the other kinds
    assert _ask(kind="mlp2", backprop_ok=True).path == "mlp_rk4_adjoint"
    assert _ask(kind="mlp2", backprop_ok=True, adjoint=False).path == "mlp_rk4_backprop"
    assert _ask(kind="mlp2", method="dopri5").path == "mlp_dopri5_adjoint"
    assert _ask(kind="mlp2", tiles_ok=False).path == D.STEPWISE
    assert _ask(kind="mlp2w").path == "mlp_rk4_adjoint" and "wide control" in _ask(kind="mlp2w", method="dopri5").reason
    assert _ask(kind="mlp3").path == "mlp_rk4_adjoint" and "three-layer" in _ask(kind="mlp3", method="dopri5").reason


# ------------------------------------------------------------------------------------------------ the envelope
def _fusable(H, C, width, dtype=torch.float32):
    from torchcde_amd.cdeint import _mlp_tall_fusable, _mlp_wide_fusable, _mlp_fusable
    func = TwoLayerField(H, C, width, dtype=dtype)
    z0 = torch.zeros(3, H, dtype=dtype)
    field = probe(func, torch.tensor(0.25, dtype=dtype), torch.randn(3, H, generator=torch.Generator().manual_seed(1)).to(dtype))[0]
    assert field is not None and field.kind == "mlp2"
    packed = torch.zeros(3, 4, C, dtype=dtype)
    claims = [fn(field, H, C, z0, packed) for fn in (_mlp_tall_fusable, _mlp_wide_fusable, _mlp_fusable)]
    assert sum(map(bool, claims)) <= 1, (H, C, width, claims)                 # one set of kernels claims a shape, or none
    return claims[0]


INSIDE = [(33, 3, 9), (64, 8, 128), (64, 32, 128), (40, 48, 20), (33, 60, 16), (48, 1, 1)]                  # (H, C, width)
OUTSIDE = [(32, 8, 16), (32, 21, 16), (65, 8, 16), (64, 33, 16), (44, 48, 16), (64, 8, 129)]


def test_tall_state_envelope_host_and_library_agree():
    lib = torchcde_amd.load()
    relu_tanh, softplus_id = _lib.field_act(_lib.ACT_TANH, _lib.HIDDEN_RELU), _lib.field_act(_lib.ACT_NONE, _lib.HIDDEN_SOFTPLUS)
    f32, f64 = _lib.dtype_enum(torch.float32), _lib.dtype_enum(torch.float64)
    for H, C, width in INSIDE:
        assert _fusable(H, C, width), (H, C, width)
        for act in (relu_tanh, softplus_id):
            assert lib.cde_rk4_mlp_tall_supported(C, H, width, f32, act) == 1, (H, C, width, act)
        assert lib.cde_rk4_mlp_wide_supported(C, H, width, f32, relu_tanh) == 0                # the other kernels keep refusing it
    for H, C, width in OUTSIDE:
        assert not _fusable(H, C, width), (H, C, width)
        assert lib.cde_rk4_mlp_tall_supported(C, H, width, f32, relu_tanh) == 0, (H, C, width)
    assert not _fusable(64, 8, 16, torch.float64)
    assert lib.cde_rk4_mlp_tall_supported(8, 64, 16, f64, relu_tanh) == 0
    assert lib.cde_rk4_mlp_tall_supported(8, 64, 16, f32, _lib.field_act(_lib.ACT_TANH, 2)) == 0      # an unknown hidden code
    assert lib.cde_rk4_mlp_tall_supported(8, 64, 16, f32, 5) == 0 and lib.cde_rk4_mlp_tall_supported(8, 64, 16, 7, relu_tanh) == 0
    assert lib.cde_rk4_mlp_tall_supported(0, 64, 16, f32, relu_tanh) == 0 and lib.cde_rk4_mlp_tall_supported(8, 0, 16, f32, 0) == 0
    assert lib.cde_rk4_mlp_tall_supported(8, 64, 0, f32, relu_tanh) == 0
    # every (H, C) of the square: the library's envelope is the stated formula
    for H in range(30, 68):
        for C in range(1, 67):
            want = 32 < H <= 64 and C <= 64 and H * ((C + 3) // 4 * 4) <= 2048
            assert lib.cde_rk4_mlp_tall_supported(C, H, 128, f32, relu_tanh) == int(want), (H, C)


# ------------------------------------------------------------------------------------------------ the C ABI
CALLSH = {
    "cde_rk4_forward_mlp_tall": "coeffs knots n_intervals=4 degree=3 W1 bias1 width=32 W2 bias2 act=1 z0 grid n_grid=5 t_out "
                                "n_out=2 z_out B=64 C=21 H=64 dtype=0 time_dtype=0 stage_index stage_frac stream=0",
    "cde_rk4_adjoint_mlp_tall_workspace_bytes": "n_sgrid=5",
    "cde_rk4_adjoint_mlp_tall_prepare": "knots n_intervals=4 sgrid n_sgrid=5 W1 bias1 width=32 W2 bias2 C=21 H=64 dtype=0 "
                                        "time_dtype=0 workspace workspace_bytes=1073741824 stream=0",
    "cde_rk4_adjoint_mlp_tall_sweep": "coeffs knots n_intervals=4 degree=3 act=1 y_state a_state sgrid n_sgrid=5 k_begin=0 "
                                      "k_end=4 U G2 G1 Z Z_hi B=64 C=21 H=64 dtype=0 time_dtype=0 workspace "
                                      "workspace_bytes=1073741824 stream=0",
}
# entry point -> {code: overrides of the valid call above that must return it}: the ORDER of the checks -- sizes (-3), unknown
# dtype (-2), the forward solve's empty batch (0), the envelope (-4), pointers (-1), the workspace one byte short (-5)
REJECTEDH = {
    "cde_rk4_forward_mlp_tall": {
        -3: ["C=0", "H=0", "n_intervals=0", "B=-1", "width=0", "n_out=0", "n_grid=0", "C=0 dtype=7", "H=0 coeffs=0"],
        -2: ["dtype=7", "time_dtype=7", "dtype=7 H=32", "dtype=7 B=0"],
        0: ["B=0", "B=0 H=32", "B=0 coeffs=0", "B=0 dtype=1"],
        -4: ["dtype=1", "H=32", "H=65", "C=65", "C=33", "H=44 C=48", "width=129", "act=5", "act=33", "act=256", "H=32 coeffs=0",
             "dtype=1 W2=0", "C=16 H=16"],
        -1: ["coeffs=0", "knots=0", "W1=0", "bias1=0", "W2=0", "bias2=0", "z0=0", "grid=0", "t_out=0", "z_out=0", "stage_index=0",
             "stage_frac=0"],
    },
    "cde_rk4_adjoint_mlp_tall_prepare": {
        -3: ["C=0", "H=0", "n_intervals=0", "width=0", "n_sgrid=-1", "C=0 dtype=7"],
        -2: ["dtype=7", "dtype=7 H=32"],
        -4: ["dtype=1", "H=32", "H=65", "C=65", "C=33", "width=129", "H=32 knots=0", "C=16 H=16"],
        -1: ["knots=0", "sgrid=0", "W1=0", "bias1=0", "W2=0", "bias2=0", "workspace=0", "workspace=0 workspace_bytes=0"],
        -5: ["workspace_bytes=SHORT"],
    },
    "cde_rk4_adjoint_mlp_tall_sweep": {
        -3: ["C=0", "H=0", "n_intervals=0", "B=0", "B=-1", "k_begin=-1", "k_begin=3 k_end=2", "k_end=5", "B=0 dtype=7"],
        -2: ["dtype=7", "dtype=7 act=5"],
        -4: ["dtype=1", "H=32", "H=65", "C=65", "C=33", "act=5", "act=33", "act=256", "act=5 coeffs=0", "C=16 H=16"],
        -1: ["coeffs=0", "knots=0", "y_state=0", "a_state=0", "sgrid=0", "U=0", "G2=0", "G1=0", "Z=0", "Z_hi=0", "workspace=0",
             "workspace=0 workspace_bytes=0"],
        -5: ["workspace_bytes=SHORT"],
    },
}


def test_tall_state_entry_points_reject_bad_calls_without_a_gpu():
    """Dummy pointers, no device: every row fails a check that comes before the first HIP call (tests/rejected_calls.py)."""
    lib = torchcde_amd.load()
    need = lib.cde_rk4_adjoint_mlp_tall_workspace_bytes(5)
    # [stage_index: 16 int64][stage_frac: 16 f32][layer-1 image (128 x 64) | b1 | W1^T image | b2 [2240] | two padded copies
    # [2240][128]]; 2240 = 2048 + 3 * 64 rows: the last unit group's tiles run up to three units past H
    images = (8192 + 128) + 4 * 8 * 64 * 4 + 2240 + 2 * 2240 * 128
    assert need == 256 + 256 + 4 * images and need % 256 == 0
    assert lib.cde_rk4_adjoint_mlp_tall_workspace_bytes(1) == lib.cde_rk4_adjoint_mlp_tall_workspace_bytes(0) == 4 * images
    assert set(REJECTEDH) | {"cde_rk4_adjoint_mlp_tall_workspace_bytes"} == set(CALLSH) <= set(_lib.EXPORTED_SYMBOLS)
    assert "cde_rk4_mlp_tall_supported" in _lib.EXPORTED_SYMBOLS
    wrong = []
    for name, by_code in REJECTEDH.items():
        call = getattr(lib, name)
        assert call(*build_args(CALLSH[name], "coeffs=0" if "coeffs" in CALLSH[name] else "knots=0")) == -1   # valid but for one pointer
        for code, cases in by_code.items():
            for overrides in cases:
                got = call(*build_args(CALLSH[name], overrides.replace("SHORT", str(need - 1))))
                if got != code:
                    wrong.append("%s(%s): %d, expected %d" % (name, overrides, got, code))
    assert not wrong, "\n".join(wrong)
    assert lib.cde_abi_version() == 3 == _lib.ABI_VERSION                     # the change is additive


# ------------------------------------------------------------------------------------------------ the index maps
LANES = [(l & 15, l >> 4) for l in range(64)]                                 # lane -> (n, q)


def _mfma(A, Bm):
    """one 16x16x4 f32 MFMA over a wave: lane (i, k) supplies A[i][k], lane (n, k) supplies B[k][n]"""
    return A @ Bm


def test_layer_one_image_over_64_state_units_and_the_four_tiles_of_va():
    """th_l1_image / th_layer1: image [tile T1][K group sg][lane][4], K step s = 4 sg + j feeds state unit 4 s + kq, which is
    register s of lane (n, kq) -- against W1 z + b1.  th_w1t_image: tile T, K step (T1, r); row i is state unit
    4 (4 T + (i & 3)) + (i >> 2), so register r of lane (n, q) is unit 16 T + 4 r + q -- against W1^T g1."""
    rng = np.random.default_rng(3)
    for H, width in ((64, 128), (33, 9), (47, 50)):
        W1, b1 = rng.standard_normal((width, H)), rng.standard_normal(width)
        z = rng.standard_normal((16, H))                                      # 16 series
        zs = np.zeros((64, 16))                                               # lane registers: zs[lane][s] = unit 4 s + q
        for lane, (n, q) in enumerate(LANES):
            for s in range(16):
                zs[lane, s] = z[n, 4 * s + q] if 4 * s + q < H else 0.0
        image = np.zeros((8, 4, 64, 4))
        for T1, sg, lane, j in itertools.product(range(8), range(4), range(64), range(4)):
            row, k = 16 * T1 + (lane & 15), 4 * (4 * sg + j) + (lane >> 4)
            image[T1, sg, lane, j] = W1[row, k] if row < width and k < H else 0.0
        pre = np.zeros((128, 16))
        for T1 in range(8):
            acc = np.zeros((16, 16))
            for s in range(16):
                A = np.array([[image[T1, s >> 2, 16 * kq + i, s & 3] for kq in range(4)] for i in range(16)])
                Bm = np.array([[zs[16 * kq + n, s] for n in range(16)] for kq in range(4)])
                acc += _mfma(A, Bm)
            pre[16 * T1:16 * T1 + 16] = acc
        want = W1 @ z.T
        np.testing.assert_allclose(pre[:width], want, rtol=1e-12, atol=1e-12)
        assert not pre[width:].any()
        # va = W1^T g1: lane (n, q) holds g1 of units 16 T1 + 4 q + r in register 4 T1 + r
        g1 = np.zeros((128, 16))
        g1[:width] = rng.standard_normal((width, 16))
        va = np.zeros((64, 16))                                               # [state unit][series]
        for T in range(4):
            acc = np.zeros((16, 16))
            for T1, r in itertools.product(range(8), range(4)):
                A = np.zeros((16, 4))
                for i, kq in itertools.product(range(16), range(4)):
                    unit, k = 16 * T1 + 4 * kq + r, 4 * (4 * T + (i & 3)) + (i >> 2)
                    A[i, kq] = W1[unit, k] if unit < width and k < H else 0.0
                Bm = np.array([[g1[16 * T1 + 4 * kq + r, n] for n in range(16)] for kq in range(4)])
                acc += _mfma(A, Bm)
            for q, r in itertools.product(range(4), range(4)):               # D row 4 q + r of lane quarter q, register r
                va[16 * T + 4 * r + q] = acc[4 * q + r]
        np.testing.assert_allclose(va[:H], W1.T @ g1[:width], rtol=1e-12, atol=1e-12)
        assert not va[H:].any()


def test_state_halves_and_the_gather_of_the_first_layer_gradient():
    """The sweep writes unit u < 32 to Z[:, u] and unit u >= 32 to Z_hi[:, u - 32]; the host writes the "1" columns; G1^T Z and
    G1^T Z_hi (the layer-1 form of cde_mlp_grad_reduce, restated as a matrix product) gathered by cdeint._mlp_tall_gradients
    are dL/dW1 | dL/db1 of einsum."""
    from torchcde_amd.cdeint import _mlp_tall_gradients
    gen = torch.Generator().manual_seed(4)
    for H, C, width in ((64, 8, 128), (33, 3, 9), (40, 48, 20)):
        rows = 24
        z = torch.randn(rows, H, generator=gen, dtype=torch.float64)
        g1 = torch.zeros(rows, 128, dtype=torch.float64)
        g1[:, :width] = torch.randn(rows, width, generator=gen, dtype=torch.float64)
        Z, Z_hi = torch.zeros(rows, 36, dtype=torch.float64), torch.zeros(rows, 36, dtype=torch.float64)
        Z[:, 32] = 1
        Z_hi[:, 32] = 1
        for m in range(16):
            for q in range(4):
                unit = 4 * m + q
                if unit < H:
                    (Z if m < 8 else Z_hi)[:, (unit & 31)] = z[:, unit]
        acc1, acc1_hi = g1.t() @ Z, g1.t() @ Z_hi
        CP = (C + 3) // 4 * 4
        blocks = (H * CP + 255) // 256
        acc2 = torch.zeros(blocks, 256, 132, dtype=torch.float64)
        dW1, db1, dW2, db2 = _mlp_tall_gradients(acc1, acc1_hi, acc2, H, C, width)
        assert dW1.shape == (width, H) and db1.shape == (width,) and dW2.shape == (H * C, width) and db2.shape == (H * C,)
        torch.testing.assert_close(dW1, torch.einsum("rw,rh->wh", g1[:, :width], z), rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(db1, g1[:, :width].sum(0), rtol=1e-12, atol=1e-12)


def test_padded_rows_cover_the_last_unit_group():
    """The sweep's tiles of unit group P run over rows (4 P + 0 .. 3) CP + c: at most 4 ceil(H / 4) CP <= 2240 rows inside the
    envelope (cde_mlp_tiled.h: MlpTiled<4>::ROWS), and more than 2048 at some shapes -- the padded copies must be that long."""
    worst = 0
    for H in range(33, 65):
        for C in range(1, 65):
            CP = (C + 3) // 4 * 4
            if H * CP <= 2048:
                worst = max(worst, (H + 3) // 4 * 4 * CP)
    assert 2048 < worst <= 2240
