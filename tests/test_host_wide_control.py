"""The two-layer field on controls of 17 to 64 channels as far as it goes without a GPU: the dispatch rows of kind "mlp2w", the
envelope (host and library), the argument checks of the new entry points, and a lane-level restatement of the index maps of
csrc/rk4_mlp_tiled.hip / cde_mlp_tiled.h -- the output layer's tiles, the dX slab, the padded copies of the sweep, the G2 blocks
and the host's gather of dW2 | db2 from the reduced block images -- against plain einsum at ragged shapes."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import torchcde_amd
from torchcde_amd import _lib
from torchcde_amd import dispatch as D
from torchcde_amd.fields import probe
from rejected_calls import build_args
from helpers import TwoLayerField

SHAPES = [(32, 64, 128), (5, 17, 9), (32, 21, 50), (1, 64, 1)]          # (H, C, width)


# ------------------------------------------------------------------------------------------------ dispatch
def _ask(**kw):
    base = dict(prod=False, kind="mlp2w", tiles_ok=True, mfma_shape=False, method="rk4", adjoint=True, wants_grad=True,
                wants_t=False, wants_control=False, params="default", adjoint_method_ok=True, options_ok=True,
                adjoint_options_ok=True, t_ok=True, variant_generic=False, shared=False, narrow_control=False,
                backprop_ok=False, identity=False, control_block=False)
    base.update(kw)
    return D.select_path(D.Request(**base))


def test_dispatch_rows_of_the_wide_control_field():
    """select_path for kind "mlp2w" over every flag, three methods and the three parameter kinds (pruned as
    tests/test_host_three_layer.py prunes them).  Fused exactly under rk4 with step_size options, not generic, and either no
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
                q = D.Request(kind="mlp2w", method=method, params=params, mfma_shape=False, backprop_ok=False, identity=False, **f)
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
    assert n > 10000 and set(seen) == {"mlp_rk4_forward", "mlp_rk4_adjoint", D.STEPWISE}
    assert set(seen) - {D.STEPWISE} <= set(D.FUSED_PATHS)                     # no new path name

    assert _ask().path == "mlp_rk4_adjoint" and _ask(params="own").path == "mlp_rk4_adjoint"
    assert _ask(wants_grad=False).path == _ask(wants_grad=False, adjoint=False).path == "mlp_rk4_forward"
    # the default method first: its reason names the wide control and what is fused for it
    default = _ask(method="dopri5")
    assert default.path == D.STEPWISE and "wide control" in default.reason and "rk4" in default.reason
    for kw in (dict(method="dopri5", wants_grad=False), dict(method="dopri5", shared=True), dict(method="midpoint"),
               dict(method="euler", wants_grad=False), dict(adjoint=False), dict(wants_t=True),
               dict(wants_control=True, params="own"), dict(params="foreign"), dict(adjoint_method_ok=False),
               dict(adjoint_options_ok=False), dict(options_ok=False)):
        verdict = _ask(**kw)
        assert verdict.path == D.STEPWISE and "wide control" in verdict.reason and "rk4" in verdict.reason, (kw, verdict)
    assert "generic" in _ask(variant_generic=True).reason
    assert "tiles" in _ask(tiles_ok=False).reason and "increasing" in _ask(t_ok=False).reason
    # nothing moved for the other kinds
    assert _ask(kind="mlp2", backprop_ok=True).path == "mlp_rk4_adjoint"
    assert _ask(kind="mlp2", backprop_ok=True, adjoint=False).path == "mlp_rk4_backprop"
    assert _ask(kind="mlp2", method="dopri5").path == "mlp_dopri5_adjoint"
    assert _ask(kind="mlp2", tiles_ok=False).path == D.STEPWISE
    assert _ask(kind="mlp3").path == "mlp_rk4_adjoint"


# ------------------------------------------------------------------------------------------------ the envelope
def _fusable(H, C, width, dtype=torch.float32):
    from torchcde_amd.cdeint import _mlp_wide_fusable, _mlp_fusable
    func = TwoLayerField(H, C, width, dtype=dtype)
    z0 = torch.zeros(3, H, dtype=dtype)
    field = probe(func, torch.tensor(0.25, dtype=dtype), torch.randn(3, H, generator=torch.Generator().manual_seed(1)).to(dtype))[0]
    assert field is not None and field.kind == "mlp2"
    packed = torch.zeros(3, 4, C, dtype=dtype)
    wide, narrow = _mlp_wide_fusable(field, H, C, z0, packed), _mlp_fusable(field, H, C, z0, packed)
    assert not (wide and narrow)                                              # one set of kernels claims a shape, or none
    return wide


def test_wide_control_envelope_host_and_library_agree():
    lib = torchcde_amd.load()
    relu_tanh, softplus_id = _lib.field_act(_lib.ACT_TANH, _lib.HIDDEN_RELU), _lib.field_act(_lib.ACT_NONE, _lib.HIDDEN_SOFTPLUS)
    f32, f64 = _lib.dtype_enum(torch.float32), _lib.dtype_enum(torch.float64)
    inside = [(8, 17, 16), (8, 21, 16), (8, 64, 16), (1, 21, 16), (32, 21, 16), (8, 21, 1), (8, 21, 128), (32, 64, 128), (1, 64, 1)]
    outside = [(8, 16, 16), (8, 65, 16), (33, 21, 16), (8, 21, 129), (32, 16, 128), (16, 16, 64)]
    for H, C, width in inside:
        assert _fusable(H, C, width), (H, C, width)
        for act in (relu_tanh, softplus_id):
            assert lib.cde_rk4_mlp_wide_supported(C, H, width, f32, act) == 1, (H, C, width, act)
    for H, C, width in outside:
        assert not _fusable(H, C, width), (H, C, width)
        assert lib.cde_rk4_mlp_wide_supported(C, H, width, f32, relu_tanh) == 0, (H, C, width)
    assert not _fusable(8, 21, 16, torch.float64)
    assert lib.cde_rk4_mlp_wide_supported(21, 8, 16, f64, relu_tanh) == 0
    assert lib.cde_rk4_mlp_wide_supported(21, 8, 16, f32, _lib.field_act(_lib.ACT_TANH, 2)) == 0      # an unknown hidden code
    assert lib.cde_rk4_mlp_wide_supported(21, 8, 16, f32, 5) == 0 and lib.cde_rk4_mlp_wide_supported(21, 8, 16, 7, relu_tanh) == 0
    assert lib.cde_rk4_mlp_wide_supported(0, 8, 16, f32, relu_tanh) == 0 and lib.cde_rk4_mlp_wide_supported(21, 0, 16, f32, 0) == 0


# ------------------------------------------------------------------------------------------------ the C ABI
CALLSW = {
    "cde_rk4_forward_mlp_wide": "coeffs knots n_intervals=4 degree=3 W1 bias1 width=32 W2 bias2 act=1 z0 grid n_grid=5 t_out "
                                "n_out=2 z_out B=64 C=21 H=32 dtype=0 time_dtype=0 stage_index stage_frac stream=0",
    "cde_rk4_adjoint_mlp_wide_workspace_bytes": "n_sgrid=5",
    "cde_rk4_adjoint_mlp_wide_prepare": "knots n_intervals=4 sgrid n_sgrid=5 W1 bias1 width=32 W2 bias2 C=21 H=32 dtype=0 "
                                        "time_dtype=0 workspace workspace_bytes=1073741824 stream=0",
    "cde_rk4_adjoint_mlp_wide_sweep": "coeffs knots n_intervals=4 degree=3 act=1 y_state a_state sgrid n_sgrid=5 k_begin=0 "
                                      "k_end=4 U G2 G1 Z B=64 C=21 H=32 dtype=0 time_dtype=0 workspace "
                                      "workspace_bytes=1073741824 stream=0",
}
# entry point -> {code: overrides of the valid call above that must return it}: the ORDER of the checks -- sizes (-3), unknown
# dtype (-2), the forward solve's empty batch (0), the envelope (-4), pointers (-1), the workspace one byte short (-5)
REJECTEDW = {
    "cde_rk4_forward_mlp_wide": {
        -3: ["C=0", "H=0", "n_intervals=0", "B=-1", "width=0", "n_out=0", "n_grid=0", "C=0 dtype=7", "H=0 coeffs=0"],
        -2: ["dtype=7", "time_dtype=7", "dtype=7 H=33", "dtype=7 B=0"],
        0: ["B=0", "B=0 H=33", "B=0 coeffs=0", "B=0 dtype=1"],
        -4: ["dtype=1", "H=33", "C=16", "C=65", "C=8", "width=129", "act=5", "act=33", "act=256", "H=33 coeffs=0", "dtype=1 W2=0",
             "C=16 H=16"],
        -1: ["coeffs=0", "knots=0", "W1=0", "bias1=0", "W2=0", "bias2=0", "z0=0", "grid=0", "t_out=0", "z_out=0", "stage_index=0",
             "stage_frac=0"],
    },
    "cde_rk4_adjoint_mlp_wide_prepare": {
        -3: ["C=0", "H=0", "n_intervals=0", "width=0", "n_sgrid=-1", "C=0 dtype=7"],
        -2: ["dtype=7", "dtype=7 H=33"],
        -4: ["dtype=1", "H=33", "C=16", "C=65", "width=129", "H=33 knots=0", "C=16 H=16"],
        -1: ["knots=0", "sgrid=0", "W1=0", "bias1=0", "W2=0", "bias2=0", "workspace=0", "workspace=0 workspace_bytes=0"],
        -5: ["workspace_bytes=SHORT"],
    },
    "cde_rk4_adjoint_mlp_wide_sweep": {
        -3: ["C=0", "H=0", "n_intervals=0", "B=0", "B=-1", "k_begin=-1", "k_begin=3 k_end=2", "k_end=5", "B=0 dtype=7"],
        -2: ["dtype=7", "dtype=7 act=5"],
        -4: ["dtype=1", "H=33", "C=16", "C=65", "act=5", "act=33", "act=256", "act=5 coeffs=0", "C=16 H=16"],
        -1: ["coeffs=0", "knots=0", "y_state=0", "a_state=0", "sgrid=0", "U=0", "G2=0", "G1=0", "Z=0", "workspace=0",
             "workspace=0 workspace_bytes=0"],
        -5: ["workspace_bytes=SHORT"],
    },
}


def test_wide_control_entry_points_reject_bad_calls_without_a_gpu():
    """Dummy pointers, no device: every row fails a check that comes before the first HIP call (tests/rejected_calls.py)."""
    lib = torchcde_amd.load()
    need = lib.cde_rk4_adjoint_mlp_wide_workspace_bytes(5)
    # [stage_index: 16 int64][stage_frac: 16 f32][layer-1 image | b1 | W1^T image | b2 [2048] | two padded copies [2048][128]]
    images = (4096 + 128) + 2 * 8 * 64 * 4 + 2048 + 2 * 2048 * 128
    assert need == 256 + 256 + 4 * images and need % 256 == 0
    assert lib.cde_rk4_adjoint_mlp_wide_workspace_bytes(1) == lib.cde_rk4_adjoint_mlp_wide_workspace_bytes(0) == 4 * images
    assert set(REJECTEDW) | {"cde_rk4_adjoint_mlp_wide_workspace_bytes"} == set(CALLSW) <= set(_lib.EXPORTED_SYMBOLS)
    wrong = []
    for name, by_code in REJECTEDW.items():
        call = getattr(lib, name)
        assert call(*build_args(CALLSW[name], "coeffs=0" if "coeffs" in CALLSW[name] else "knots=0")) == -1   # valid but for one pointer
        for code, cases in by_code.items():
            for overrides in cases:
                got = call(*build_args(CALLSW[name], overrides.replace("SHORT", str(need - 1))))
                if got != code:
                    wrong.append("%s(%s): %d, expected %d" % (name, overrides, got, code))
    assert not wrong, "\n".join(wrong)
    assert lib.cde_abi_version() == 3 == _lib.ABI_VERSION                     # the change is additive


# ------------------------------------------------------------------------------------------------ the index maps
LANES = [(l & 15, l >> 4) for l in range(64)]                                 # lane -> (n, q)
SLAB_STRIDE = 68                                                               # cde_mlp_tiled.h: TL_SLAB_STRIDE
ROWS, MW = 2048, 128                                                           # rows / columns of the sweep's padded copies


def _mfma_16x16x4(a_lane, b_lane, acc):
    """v_mfma_f32_16x16x4_f32: lane l supplies A[i=l&15][k=l>>4], B[k=l>>4][j=l&15]; register r of lane l holds
    D[4*(l>>4)+r][l&15] (tests/test_host.py), all 64 lanes at once."""
    P = np.asarray(a_lane).reshape(4, 16).T @ np.asarray(b_lane).reshape(4, 16)
    acc += P.reshape(4, 4, 16).transpose(0, 2, 1).reshape(64, 4)


def _fragment(x):
    """layer 1's C/D fragment: register 4 T + r of lane (n, q) = x[n, 16 T + 4 q + r]"""
    reg = np.zeros((64, 32))
    for l, (n, q) in enumerate(LANES):
        for T in range(8):
            reg[l, 4 * T:4 * T + 4] = x[n, 16 * T + 4 * q:16 * T + 4 * q + 4]
    return reg


def _flat_read(flat, at):
    assert 0 <= at < flat.size, "a read outside the tensor: %d of %d" % (at, flat.size)
    return flat[at]


def _inputs(H, C, w, seed):
    rng = np.random.default_rng(seed)
    W2 = rng.standard_normal((H * C, w)) * 0.3
    b2 = rng.standard_normal(H * C)
    u = np.full((16, 128), np.log(2.0))                                       # padded units as softplus(0) leaves them
    u[:, :w] = rng.standard_normal((16, w))
    dX = rng.standard_normal((16, C))
    a = rng.standard_normal((16, H))
    return W2, b2, u, dX, a


def _slab(dX, C, CP):
    """wc_control_slope: lane (n, q) writes channels q, 4 + q, .. < CP of series n, zero from C on"""
    slab = np.full(16 * SLAB_STRIDE, np.nan)
    for n, q in LANES:
        for c in range(q, CP, 4):
            slab[n * SLAB_STRIDE + c] = dX[n, c] if c < C else 0.0
    return slab


@pytest.mark.parametrize("H,C,w", SHAPES)
def test_control_slope_slab_from_the_packed_coefficients(H, C, w):
    """The slab's writes from the coefficient tensors' flat layouts -- cubic (B, n, 4 C) = a | b | 2c | 3d, linear (B, n + 1, C)
    -- and the float4 a lane reads back per tile, against the derivative computed on the reshaped arrays."""
    rng = np.random.default_rng(11 + C)
    CP, n_int, idx, frac, width = (C + 3) // 4 * 4, 5, 3, 0.37, 1.7
    assert CP <= SLAB_STRIDE - 4 and (SLAB_STRIDE * 4) % 16 == 0
    for degree in (3, 1):
        coeffs = rng.standard_normal((16, n_int, 4 * C) if degree == 3 else (16, n_int + 1, C))
        flat = coeffs.ravel()
        dX = np.zeros((16, C))
        for n in range(16):
            base = (n * n_int + idx) * 4 * C if degree == 3 else (n * (n_int + 1) + idx) * C
            for c in range(C):
                if degree == 3:
                    b, c2, d3 = (_flat_read(flat, base + part * C + c) for part in (1, 2, 3))
                    dX[n, c] = b + (c2 + d3 * frac) * frac
                else:
                    dX[n, c] = (_flat_read(flat, base + C + c) - _flat_read(flat, base + c)) / width
        if degree == 3:
            want = coeffs[:, idx, C:2 * C] + (coeffs[:, idx, 2 * C:3 * C] + coeffs[:, idx, 3 * C:] * frac) * frac
        else:
            want = (coeffs[:, idx + 1] - coeffs[:, idx]) / width
        assert np.allclose(dX, want, rtol=1e-13, atol=1e-13)
        slab = _slab(dX, C, CP)
        for n, q in LANES:
            for tb in range(CP // 4):
                got = slab[n * SLAB_STRIDE + 4 * tb:n * SLAB_STRIDE + 4 * tb + 4]
                pad = np.zeros(4)
                pad[:max(0, min(4, C - 4 * tb))] = want[n, 4 * tb:4 * tb + 4]
                assert np.array_equal(got, pad), (n, tb)


@pytest.mark.parametrize("H,C,w", SHAPES)
def test_output_layer_tiles_of_the_forward_kernel(H, C, w):
    """rk4_forward_mlp_tiled: per unit group P and tile tb the lane's A operands from the caller's W2 (vector and scalar form:
    the same guards), the bias as the accumulator's initial value, the 32 K steps on layer 1's fragment, tanh, and the
    contraction with the slab -- f for unit 4 P + q of series n, against einsum.  No read leaves W2 / b2."""
    W2, b2, u, dX, _ = _inputs(H, C, w, 3)
    CP, NP, NB = (C + 3) // 4 * 4, (H + 3) // 4, (C + 3) // 4
    w2f, b2f, slab, ureg = W2.ravel(), b2.ravel(), _slab(dX, C, CP), _fragment(u)
    f = np.zeros((64, 8))

    def load_tile(P, tb):
        a = np.zeros((64, 8, 4)); bias = np.zeros((64, 4))
        for l, (n, q) in enumerate(LANES):
            h, c = 4 * P + (n >> 2), 4 * tb + (n & 3)
            for g in range(8):
                for j in range(4):
                    col = 16 * g + 4 * q + j
                    if h < H and c < C and col < w:
                        a[l, g, j] = _flat_read(w2f, (h * C + c) * w + col)
            for r in range(4):
                if 4 * P + q < H and 4 * tb + r < C:
                    bias[l, r] = _flat_read(b2f, (4 * P + q) * C + 4 * tb + r)
        return a, bias

    for P in range(NP):
        for tb in range(NB):
            a, acc = load_tile(P, tb)
            for g in range(8):
                for j in range(4):
                    _mfma_16x16x4(a[:, g, j], ureg[:, 4 * g + j], acc)
            for l, (n, q) in enumerate(LANES):
                f[l, P] += np.tanh(acc[l]) @ slab[n * SLAB_STRIDE + 4 * tb:n * SLAB_STRIDE + 4 * tb + 4]
    # the requests past the last tile of a group / the last group read nothing and give zeros
    for P, tb in ((NP - 1, NB), (NP, 0)):
        a, bias = load_tile(P, tb)
        assert not a.any() and not bias.any()
    Y = np.tanh(u[:, :w] @ W2.T + b2).reshape(16, H, C)
    want = np.einsum("nhc,nc->nh", Y, dX)
    for l, (n, q) in enumerate(LANES):
        for P in range(8):
            assert np.isclose(f[l, P], want[n, 4 * P + q] if 4 * P + q < H else 0.0, rtol=1e-12, atol=1e-12), (l, P)


def _sweep_images(W2, b2, H, C, w):
    """mlp_tiled_adj_image_kernel: b2 at h CP + c; the plain copy [row][col]; the gu copy [row][8 n + T1] = W2[row][16 T1 + n]"""
    CP = (C + 3) // 4 * 4
    b2p, w2p, w2t = np.zeros(ROWS), np.zeros((ROWS, MW)), np.zeros((ROWS, MW))
    for row in range(ROWS):
        h, c = divmod(row, CP)
        if h < H and c < C:
            b2p[row] = b2[h * C + c]
            w2p[row, :w] = W2[h * C + c]
            for j in range(MW):
                col = 16 * (j & 7) + (j >> 3)
                if col < w:
                    w2t[row, j] = W2[h * C + c, col]
    return b2p, w2p.ravel(), w2t.ravel()


@pytest.mark.parametrize("H,C,w", SHAPES)
def test_sweep_tiles_g2_blocks_and_the_gradient_gather(H, C, w):
    """rk4_adjoint_mlp_tiled_sweep on one (stage, series-tile): Y2 from the padded plain copy, g2 = a_h dX_c (1 - tanh^2) into
    the G2 blocks (block at >> 8, column at & 255 of at = h CP + c; rows h >= H never written), gu = W2^T g2 through the gu
    copy in layer 1's fragment form; then the reduction G2_b^T [U | 1] per block and the host's gather
    (cdeint._mlp_wide_gradients) -- against einsum."""
    from torchcde_amd.cdeint import _mlp_wide_gradients
    W2, b2, u, dX, a = _inputs(H, C, w, 5)
    CP, NP, NB = (C + 3) // 4 * 4, (H + 3) // 4, (C + 3) // 4
    blocks = (H * CP + 255) // 256
    b2p, w2p, w2t = _sweep_images(W2, b2, H, C, w)
    slab, ureg = _slab(dX, C, CP), _fragment(u)
    G2 = np.zeros((blocks, 16, 256))                                          # one row per series of the tile
    written = np.zeros((blocks, 16, 256), dtype=bool)
    gu = np.zeros((8, 64, 4))
    for P in range(NP):
        for tb in range(NB):
            rows = 4 * P * CP + 4 * tb
            acc = np.zeros((64, 4)); ay = np.zeros((64, 8, 4)); ag = np.zeros((64, 4, 8))
            for l, (n, q) in enumerate(LANES):
                y_off = ((n >> 2) * CP + (n & 3)) * MW + 4 * q
                for g in range(8):
                    for j in range(4):
                        ay[l, g, j] = _flat_read(w2p, rows * MW + y_off + 16 * g + j)
                for r in range(4):
                    acc[l, r] = _flat_read(b2p, q * CP + rows + r)
                    for T1 in range(8):
                        ag[l, r, T1] = _flat_read(w2t, (q * CP + rows + r) * MW + 8 * n + T1)
            for g in range(8):
                for j in range(4):
                    _mfma_16x16x4(ay[:, g, j], ureg[:, 4 * g + j], acc)
            t = np.tanh(acc)
            g2 = np.zeros((64, 4))
            for l, (n, q) in enumerate(LANES):
                dx = slab[n * SLAB_STRIDE + 4 * tb:n * SLAB_STRIDE + 4 * tb + 4]
                a_P = a[n, 4 * P + q] if 4 * P + q < H else 0.0               # the state registers beyond H hold zeros
                g2[l] = a_P * (dx * (1 - t[l] * t[l]))
                if 4 * P + q < H:
                    at = (4 * P + q) * CP + 4 * tb
                    assert (at >> 8) == ((at + 3) >> 8) and (at >> 8) < blocks
                    G2[at >> 8, n, (at & 255):(at & 255) + 4] = g2[l]
                    assert not written[at >> 8, n, (at & 255):(at & 255) + 4].any()
                    written[at >> 8, n, (at & 255):(at & 255) + 4] = True
            for r in range(4):
                for T1 in range(8):
                    _mfma_16x16x4(ag[:, r, T1], g2[:, r], gu[T1])
    # the request after the last tile stays inside the copies: load_y(P + 1, 0) with rows = 0 for P + 1 = 8
    rows_after = 4 * NP * CP if NP < 8 else 0
    assert rows_after + 3 * CP + 3 < ROWS
    assert written.reshape(blocks * 16, 256).sum() == 16 * H * CP
    Y = np.tanh(u[:, :w] @ W2.T + b2).reshape(16, H, C)
    g2_want = a[:, :, None] * dX[:, None, :] * (1 - Y * Y)
    # gu in layer 1's fragment form; the columns beyond the width get nothing from the zero padding
    gu_want = np.zeros((16, 128)); gu_want[:, :w] = g2_want.reshape(16, H * C) @ W2
    want_reg = _fragment(gu_want)
    for T1 in range(8):
        assert np.allclose(gu[T1], want_reg[:, 4 * T1:4 * T1 + 4], rtol=1e-12, atol=1e-12), T1
    # the reduction of every block against [U | 1 | 0 0 0] and the host's gather
    U = np.zeros((16, 132)); U[:, :128] = u; U[:, 128] = 1
    acc2 = torch.from_numpy(np.stack([G2[b].T @ U for b in range(blocks)]))
    acc1 = torch.zeros(128, 36, dtype=torch.float64)
    _, _, dW2, db2 = _mlp_wide_gradients(acc1, acc2, H, C, w)
    assert dW2.shape == (H * C, w) and db2.shape == (H * C,)
    assert np.allclose(dW2.numpy(), np.einsum("nhc,nw->hcw", g2_want, u[:, :w]).reshape(H * C, w), rtol=1e-12, atol=1e-12)
    assert np.allclose(db2.numpy(), g2_want.sum(0).reshape(H * C), rtol=1e-12, atol=1e-12)
