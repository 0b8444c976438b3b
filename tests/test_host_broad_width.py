"""The two-layer field with an inner layer of 129 to 256 units as far as it goes without a GPU: the dispatch rows of kind
"mlp2b", the envelope (host and library), the argument checks of the new entry points, and a lane-level restatement of the
index maps of csrc/rk4_mlp_broad.hip / cde_mlp_broad.h -- the two K halves of a tile from the padded copies, the gu copy, the
factor rows in halves (U_lo | U_hi, G1_lo | G1_hi), the G2 blocks and the host's gather of all four gradients from the reduced
images -- against plain einsum."""
import itertools

import numpy as np
import pytest
import torch

import torchcde_amd
from torchcde_amd import _lib
from torchcde_amd import dispatch as D
from torchcde_amd.fields import probe
from rejected_calls import build_args
from helpers import TwoLayerField


# ------------------------------------------------------------------------------------------------ dispatch
def _ask(**kw):
    base = dict(prod=False, kind="mlp2b", tiles_ok=True, mfma_shape=False, method="rk4", adjoint=True, wants_grad=True,
                wants_t=False, wants_control=False, params="default", adjoint_method_ok=True, options_ok=True,
                adjoint_options_ok=True, t_ok=True, variant_generic=False, shared=False, narrow_control=False,
                backprop_ok=False, identity=False, control_block=False)
    base.update(kw)
    return D.select_path(D.Request(**base))


def test_dispatch_rows_of_the_broad_inner_layer():
    """select_path for kind "mlp2b" over every flag, three methods and the three parameter kinds (pruned as
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
                q = D.Request(kind="mlp2b", method=method, params=params, mfma_shape=False, backprop_ok=False, identity=False, **f)
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
    # the default method first: its reason names the inner layer and what is fused for it
    default = _ask(method="dopri5")
    assert default.path == D.STEPWISE and "inner layer" in default.reason and "rk4" in default.reason
    for kw in (dict(method="dopri5", wants_grad=False), dict(method="dopri5", shared=True), dict(method="midpoint"),
               dict(method="euler", wants_grad=False), dict(adjoint=False), dict(wants_t=True),
               dict(wants_control=True, params="own"), dict(params="foreign"), dict(adjoint_method_ok=False),
               dict(adjoint_options_ok=False), dict(options_ok=False)):
        verdict = _ask(**kw)
        assert verdict.path == D.STEPWISE and "inner layer" in verdict.reason and "rk4" in verdict.reason, (kw, verdict)
    assert "generic" in _ask(variant_generic=True).reason
    assert "tiles" in _ask(tiles_ok=False).reason and "increasing" in _ask(t_ok=False).reason
    # nothing moved for the other kinds
    assert _ask(kind="mlp2", backprop_ok=True).path == "mlp_rk4_adjoint"
    assert _ask(kind="mlp2", backprop_ok=True, adjoint=False).path == "mlp_rk4_backprop"
    assert _ask(kind="mlp2", method="dopri5").path == "mlp_dopri5_adjoint"
    assert _ask(kind="mlp2", tiles_ok=False).path == D.STEPWISE
    assert _ask(kind="mlp3").path == "mlp_rk4_adjoint"
    for kind, noun in (("mlp2w", "wide control"), ("mlp2h", "tall hidden state")):
        assert _ask(kind=kind).path == "mlp_rk4_adjoint" and _ask(kind=kind, wants_grad=False).path == "mlp_rk4_forward"
        assert noun in _ask(kind=kind, method="dopri5").reason


# ------------------------------------------------------------------------------------------------ the envelope
def _fusable(H, C, width, dtype=torch.float32):
    """(the broad predicate's verdict, whether any of the three older predicates claims the shape)"""
    from torchcde_amd.cdeint import _mlp_broad_fusable, _mlp_fusable, _mlp_wide_fusable, _mlp_tall_fusable
    func = TwoLayerField(H, C, width, dtype=dtype)
    z0 = torch.zeros(3, H, dtype=dtype)
    field = probe(func, torch.tensor(0.25, dtype=dtype), torch.randn(3, H, generator=torch.Generator().manual_seed(1)).to(dtype))[0]
    assert field is not None and field.kind == "mlp2"
    packed = torch.zeros(3, 4, C, dtype=dtype)
    broad = _mlp_broad_fusable(field, H, C, z0, packed)
    older = [p(field, H, C, z0, packed) for p in (_mlp_fusable, _mlp_wide_fusable, _mlp_tall_fusable)]
    assert broad + sum(older) <= 1                                            # one set of kernels claims a shape, or none
    return broad, any(older)


def test_broad_inner_layer_envelope_host_and_library_agree():
    lib = torchcde_amd.load()
    relu_tanh, softplus_id = _lib.field_act(_lib.ACT_TANH, _lib.HIDDEN_RELU), _lib.field_act(_lib.ACT_NONE, _lib.HIDDEN_SOFTPLUS)
    f32, f64 = _lib.dtype_enum(torch.float32), _lib.dtype_enum(torch.float64)
    inside = [(32, 8, 129), (32, 8, 256), (1, 1, 129), (32, 32, 256), (16, 64, 200), (5, 3, 130)]
    outside = [(32, 8, 128), (32, 8, 257), (33, 8, 200), (32, 33, 200), (32, 65, 129)]          # (32, 33): CP = 36, 1152 rows
    for H, C, width in inside:
        assert _fusable(H, C, width) == (True, False), (H, C, width)
        for act in (relu_tanh, softplus_id):
            assert lib.cde_rk4_mlp_broad_supported(C, H, width, f32, act) == 1, (H, C, width, act)
    for H, C, width in outside:
        assert not _fusable(H, C, width)[0], (H, C, width)
        assert lib.cde_rk4_mlp_broad_supported(C, H, width, f32, relu_tanh) == 0, (H, C, width)
    assert not _fusable(32, 8, 200, torch.float64)[0]
    assert lib.cde_rk4_mlp_broad_supported(8, 32, 200, f64, relu_tanh) == 0
    assert lib.cde_rk4_mlp_broad_supported(8, 32, 200, f32, _lib.field_act(_lib.ACT_TANH, 2)) == 0     # an unknown hidden code
    assert lib.cde_rk4_mlp_broad_supported(8, 32, 200, f32, 5) == 0 and lib.cde_rk4_mlp_broad_supported(8, 32, 200, 7, relu_tanh) == 0
    assert lib.cde_rk4_mlp_broad_supported(0, 32, 200, f32, relu_tanh) == 0 and lib.cde_rk4_mlp_broad_supported(8, 0, 200, f32, 0) == 0
    # the older predicates and entry points keep refusing width 129, on every shape of theirs
    for H, C in ((32, 8), (8, 21), (40, 8)):
        assert _fusable(H, C, 129)[1] is False, (H, C)
        assert _fusable(H, C, 128)[1] is True, (H, C)
    assert lib.cde_rk4_mlp_wide_supported(21, 8, 129, f32, relu_tanh) == 0 and lib.cde_rk4_mlp_wide_supported(21, 8, 128, f32, relu_tanh) == 1
    assert lib.cde_rk4_mlp_tall_supported(8, 40, 129, f32, relu_tanh) == 0 and lib.cde_rk4_mlp_tall_supported(8, 40, 128, f32, relu_tanh) == 1


# ------------------------------------------------------------------------------------------------ the C ABI
CALLSB = {
    "cde_rk4_forward_mlp_broad": "coeffs knots n_intervals=4 degree=3 W1 bias1 width=200 W2 bias2 act=1 z0 grid n_grid=5 t_out "
                                 "n_out=2 z_out B=64 C=8 H=32 dtype=0 time_dtype=0 stage_index stage_frac stream=0",
    "cde_rk4_adjoint_mlp_broad_workspace_bytes": "n_sgrid=5",
    "cde_rk4_adjoint_mlp_broad_prepare": "knots n_intervals=4 sgrid n_sgrid=5 W1 bias1 width=200 W2 bias2 C=8 H=32 dtype=0 "
                                         "time_dtype=0 workspace workspace_bytes=1073741824 stream=0",
    "cde_rk4_adjoint_mlp_broad_sweep": "coeffs knots n_intervals=4 degree=3 act=1 y_state a_state sgrid n_sgrid=5 k_begin=0 "
                                       "k_end=4 U_lo U_hi G2 G1_lo G1_hi Z B=64 C=8 H=32 dtype=0 time_dtype=0 workspace "
                                       "workspace_bytes=1073741824 stream=0",
}
# entry point -> {code: overrides of the valid call above that must return it}: the ORDER of the checks -- sizes (-3), unknown
# dtype (-2), the forward solve's empty batch (0), the envelope (-4), pointers (-1), the workspace one byte short (-5)
REJECTEDB = {
    "cde_rk4_forward_mlp_broad": {
        -3: ["C=0", "H=0", "n_intervals=0", "B=-1", "width=0", "n_out=0", "n_grid=0", "C=0 dtype=7", "H=0 coeffs=0"],
        -2: ["dtype=7", "time_dtype=7", "dtype=7 H=33", "dtype=7 B=0"],
        0: ["B=0", "B=0 H=33", "B=0 coeffs=0", "B=0 dtype=1"],
        -4: ["dtype=1", "H=33", "C=65", "C=33", "width=128", "width=1", "width=257", "act=5", "act=33", "act=256",
             "H=33 coeffs=0", "dtype=1 W2=0", "C=64 H=17"],
        -1: ["coeffs=0", "knots=0", "W1=0", "bias1=0", "W2=0", "bias2=0", "z0=0", "grid=0", "t_out=0", "z_out=0", "stage_index=0",
             "stage_frac=0"],
    },
    "cde_rk4_adjoint_mlp_broad_prepare": {
        -3: ["C=0", "H=0", "n_intervals=0", "width=0", "n_sgrid=-1", "C=0 dtype=7"],
        -2: ["dtype=7", "dtype=7 H=33"],
        -4: ["dtype=1", "H=33", "C=65", "C=33", "width=128", "width=257", "H=33 knots=0", "C=64 H=17"],
        -1: ["knots=0", "sgrid=0", "W1=0", "bias1=0", "W2=0", "bias2=0", "workspace=0", "workspace=0 workspace_bytes=0"],
        -5: ["workspace_bytes=SHORT"],
    },
    "cde_rk4_adjoint_mlp_broad_sweep": {
        -3: ["C=0", "H=0", "n_intervals=0", "B=0", "B=-1", "k_begin=-1", "k_begin=3 k_end=2", "k_end=5", "B=0 dtype=7"],
        -2: ["dtype=7", "dtype=7 act=5"],
        -4: ["dtype=1", "H=33", "C=65", "C=33", "act=5", "act=33", "act=256", "act=5 coeffs=0", "C=64 H=17"],
        -1: ["coeffs=0", "knots=0", "y_state=0", "a_state=0", "sgrid=0", "U_lo=0", "U_hi=0", "G2=0", "G1_lo=0", "G1_hi=0", "Z=0",
             "workspace=0", "workspace=0 workspace_bytes=0"],
        -5: ["workspace_bytes=SHORT"],
    },
}
ROWS, BW = 1024 + 3 * 64, 256                                                 # rows / columns of the sweep's padded copies


def test_broad_inner_layer_entry_points_reject_bad_calls_without_a_gpu():
    """Dummy pointers, no device: every row fails a check that comes before the first HIP call (tests/rejected_calls.py)."""
    lib = torchcde_amd.load()
    need = lib.cde_rk4_adjoint_mlp_broad_workspace_bytes(5)
    # [stage_index: 16 int64][stage_frac: 16 f32][layer-1 image | b1 | W1^T image | b2 [ROWS] | two padded copies [ROWS][256]]
    images = (8192 + 256) + 2 * 16 * 64 * 4 + ROWS + 2 * ROWS * BW
    assert need == 256 + 256 + 4 * images and need % 256 == 0
    assert lib.cde_rk4_adjoint_mlp_broad_workspace_bytes(1) == lib.cde_rk4_adjoint_mlp_broad_workspace_bytes(0) == 4 * images
    assert set(REJECTEDB) | {"cde_rk4_adjoint_mlp_broad_workspace_bytes"} == set(CALLSB) <= set(_lib.EXPORTED_SYMBOLS)
    assert "cde_rk4_mlp_broad_supported" in _lib.EXPORTED_SYMBOLS
    wrong = []
    for name, by_code in REJECTEDB.items():
        call = getattr(lib, name)
        assert call(*build_args(CALLSB[name], "coeffs=0" if "coeffs" in CALLSB[name] else "knots=0")) == -1   # valid but for one pointer
        for code, cases in by_code.items():
            for overrides in cases:
                got = call(*build_args(CALLSB[name], overrides.replace("SHORT", str(need - 1))))
                if got != code:
                    wrong.append("%s(%s): %d, expected %d" % (name, overrides, got, code))
    assert not wrong, "\n".join(wrong)
    assert lib.cde_abi_version() == 3 == _lib.ABI_VERSION                     # the change is additive


# ------------------------------------------------------------------------------------------------ the index maps
LANES = [(l & 15, l >> 4) for l in range(64)]                                 # lane -> (n, q)
SLAB_STRIDE = 68                                                               # cde_mlp_tiled.h: TL_SLAB_STRIDE


def _mfma_16x16x4(a_lane, b_lane, acc):
    """v_mfma_f32_16x16x4_f32: lane l supplies A[i=l&15][k=l>>4], B[k=l>>4][j=l&15]; register r of lane l holds
    D[4*(l>>4)+r][l&15] (tests/test_host.py), all 64 lanes at once."""
    P = np.asarray(a_lane).reshape(4, 16).T @ np.asarray(b_lane).reshape(4, 16)
    acc += P.reshape(4, 4, 16).transpose(0, 2, 1).reshape(64, 4)


def _fragment(x):
    """layer 1's C/D fragment of one 128-unit half: register 4 T + r of lane (n, q) = x[n, 16 T + 4 q + r]"""
    reg = np.zeros((64, 32))
    for l, (n, q) in enumerate(LANES):
        for T in range(8):
            reg[l, 4 * T:4 * T + 4] = x[n, 16 * T + 4 * q:16 * T + 4 * q + 4]
    return reg


def _flat_read(flat, at):
    assert 0 <= at < flat.size, "a read outside the tensor: %d of %d" % (at, flat.size)
    return flat[at]


def _sweep_images(W2, b2, H, C, w):
    """mlp_broad_adj_image_kernel: b2 at h CP + c; the plain copy [row][col]; the gu copy [row][16 n + T1] = W2[row][16 T1 + n]"""
    CP = (C + 3) // 4 * 4
    b2p, w2p, w2t = np.zeros(ROWS), np.zeros((ROWS, BW)), np.zeros((ROWS, BW))
    j = np.arange(BW)
    col = 16 * (j & 15) + (j >> 4)
    for row in range(ROWS):
        h, c = divmod(row, CP)
        if h < H and c < C:
            b2p[row] = b2[h * C + c]
            w2p[row, :w] = W2[h * C + c]
            w2t[row, col < w] = W2[h * C + c, col[col < w]]
    return b2p, w2p.ravel(), w2t.ravel()


@pytest.mark.parametrize("H,C,w", [(5, 3, 129), (32, 32, 256), (17, 60, 130)])       # the last: 20 x 60 rows of the copies, past H CP
def test_factor_rows_in_halves_g2_blocks_and_the_gradient_gather(H, C, w):
    """rk4_adjoint_mlp_broad_sweep on one (stage, series-tile).  Y2 of every tile from the padded plain copy as two K halves
    into one accumulator; g2 = a_h dX_c (1 - tanh^2) into the G2 blocks; gu_lo | gu_hi = W2^T g2 through the gu copy's two
    float4 pairs; the stores of U_lo | U_hi and G1_lo | G1_hi.  Every unit < width of U and of G1 and every (h < H, c < C) of
    G2 is written exactly once, in the half / block the header names, no read leaves the copies, and the reductions + the
    host's gather (cdeint._mlp_broad_gradients) give all four gradients -- against einsum."""
    from torchcde_amd.cdeint import _mlp_broad_gradients
    rng = np.random.default_rng(7 + H)
    W2 = rng.standard_normal((H * C, w)) * 0.3
    b2 = rng.standard_normal(H * C)
    u = np.full((16, 256), np.log(2.0))                                       # padded units as softplus(0) leaves them
    u[:, :w] = rng.standard_normal((16, w))
    dX, a, z = rng.standard_normal((16, C)), rng.standard_normal((16, H)), rng.standard_normal((16, H))
    slope1 = np.zeros((16, 256)); slope1[:, :w] = rng.uniform(0.1, 0.9, (16, w))       # hid'(pre1); whatever beyond the width
    slope1[:, w:] = 0.5
    CP, NP, NB = (C + 3) // 4 * 4, (H + 3) // 4, (C + 3) // 4
    blocks = (H * CP + 255) // 256
    assert blocks <= 4 and 4 * NP * CP <= ROWS
    b2p, w2p, w2t = _sweep_images(W2, b2, H, C, w)
    slab = np.zeros(16 * SLAB_STRIDE)
    for n in range(16):
        slab[n * SLAB_STRIDE:n * SLAB_STRIDE + C] = dX[n]
    ureg = [_fragment(u[:, :128]), _fragment(u[:, 128:])]
    G2 = np.zeros((blocks, 16, 256))
    hits2 = np.zeros((blocks, 16, 256), dtype=int)
    gu = np.zeros((2, 8, 64, 4))
    for P in range(NP):
        for tb in range(NB):
            rows = 4 * P * CP + 4 * tb
            acc = np.zeros((64, 4))
            ay = np.zeros((2, 64, 8, 4)); ag = np.zeros((2, 64, 4, 8))
            for l, (n, q) in enumerate(LANES):
                y_off = ((n >> 2) * CP + (n & 3)) * BW + 4 * q
                for half in range(2):
                    for g in range(8):
                        for j in range(4):
                            ay[half, l, g, j] = _flat_read(w2p, rows * BW + y_off + 128 * half + 16 * g + j)
                for r in range(4):
                    acc[l, r] = _flat_read(b2p, q * CP + rows + r)
                    for half in range(2):
                        for T1 in range(8):       # float4 2 half, 2 half + 1 of the lane's 16 floats at 16 n
                            ag[half, l, r, T1] = _flat_read(w2t, (q * CP + rows + r) * BW + 16 * n + 8 * half + T1)
            for half in range(2):                 # lower K half, then the upper one, into the same accumulator
                for g in range(8):
                    for j in range(4):
                        _mfma_16x16x4(ay[half, :, g, j], ureg[half][:, 4 * g + j], acc)
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
                    hits2[at >> 8, n, (at & 255):(at & 255) + 4] += 1
            for half in range(2):
                for r in range(4):
                    for T1 in range(8):
                        _mfma_16x16x4(ag[half, :, r, T1], g2[:, r], gu[half, T1])
    # the request after the last tile stays inside the copies: rows = 0 when the group does not exist
    assert 3 * CP + 3 < ROWS
    # G2: every (h < H, c < CP) once -- the padded channels c >= C carry zeros (dX is zero there) -- and nothing else
    want_hits = np.zeros(blocks * 256, dtype=int); want_hits[:H * CP] = 1
    assert (hits2.transpose(1, 0, 2).reshape(16, blocks * 256) == want_hits).all()
    Y = np.tanh(u[:, :w] @ W2.T + b2).reshape(16, H, C)
    g2_want = a[:, :, None] * dX[:, None, :] * (1 - Y * Y)
    flat = G2.transpose(1, 0, 2).reshape(16, blocks * 256)[:, :H * CP].reshape(16, H, CP)
    assert np.allclose(flat[:, :, :C], g2_want, rtol=1e-12, atol=1e-12) and not flat[:, :, C:].any()
    # gu in layer 1's fragment form, half by half; the units beyond the width get exact zeros from the zero padding
    gu_want = np.zeros((16, 256)); gu_want[:, :w] = g2_want.reshape(16, H * C) @ W2
    for half in range(2):
        want_reg = _fragment(gu_want[:, 128 * half:128 * half + 128])
        for T1 in range(8):
            assert np.allclose(gu[half, T1], want_reg[:, 4 * T1:4 * T1 + 4], rtol=1e-12, atol=1e-12), (half, T1)
    # the stores of the inner layer's rows: lane (n, q) writes columns 16 T1 + 4 q .. + 3 of row n of its half
    U = np.zeros((2, 16, 132)); G1 = np.zeros((2, 16, 128)); Z = np.zeros((16, 36))
    hits_u = np.zeros((2, 16, 132), dtype=int); hits_g1 = np.zeros((2, 16, 128), dtype=int); hits_z = np.zeros((16, 36), dtype=int)
    sreg = [_fragment(slope1[:, :128]), _fragment(slope1[:, 128:])]
    for l, (n, q) in enumerate(LANES):
        for half in range(2):
            for T1 in range(8):
                at = 16 * T1 + 4 * q
                U[half, n, at:at + 4] = ureg[half][l, 4 * T1:4 * T1 + 4]
                G1[half, n, at:at + 4] = gu[half, T1, l] * sreg[half][l, 4 * T1:4 * T1 + 4]
                hits_u[half, n, at:at + 4] += 1
                hits_g1[half, n, at:at + 4] += 1
        for m in range(8):
            if 4 * m + q < H:
                Z[n, 4 * m + q] = z[n, 4 * m + q]
                hits_z[n, 4 * m + q] += 1
    U[:, :, 128] = 1; Z[:, 32] = 1                                            # the caller's "1" columns
    for unit in range(w):                                                     # every unit once, in the half the header names
        assert (hits_u[unit >> 7, :, unit & 127] == 1).all() and (hits_g1[unit >> 7, :, unit & 127] == 1).all()
    assert not hits_u[:, :, 128:].any() and hits_u.max() == 1 and hits_g1.max() == 1
    assert (hits_z[:, :H] == 1).all() and not hits_z[:, H:].any()
    assert not G1[1, :, w - 128:].any()                                       # zeros, not garbage, beyond the width
    assert np.array_equal(np.concatenate((U[0, :, :128], U[1, :, :128]), axis=1), u)
    g1_want = gu_want * slope1
    # the reductions: every G2 block against each U half (layer 2), each G1 half against Z (layer 1); the host's gather
    acc2 = [torch.from_numpy(np.stack([G2[b].T @ U[half] for b in range(blocks)])) for half in range(2)]
    acc1 = []
    for half in range(2):
        image = np.zeros((128, 36)); image[:, :] = G1[half].T @ Z
        acc1.append(torch.from_numpy(image))
    dW1, db1, dW2, db2 = _mlp_broad_gradients(acc1[0], acc1[1], acc2[0], acc2[1], H, C, w)
    assert dW1.shape == (w, H) and db1.shape == (w,) and dW2.shape == (H * C, w) and db2.shape == (H * C,)
    assert dW2.is_contiguous() and dW1.is_contiguous()
    assert np.allclose(dW1.numpy(), g1_want[:, :w].T @ z, rtol=1e-12, atol=1e-12)
    assert np.allclose(db1.numpy(), g1_want[:, :w].sum(0), rtol=1e-12, atol=1e-12)
    assert np.allclose(dW2.numpy(), np.einsum("nhc,nw->hcw", g2_want, u[:, :w]).reshape(H * C, w), rtol=1e-12, atol=1e-12)
    assert np.allclose(db2.numpy(), g2_want.sum(0).reshape(H * C), rtol=1e-12, atol=1e-12)
