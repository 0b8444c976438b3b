"""The one-layer field on controls of 17 to 64 channels as far as it goes without a GPU: the envelope of the tiled kernels K2c /
K3c (csrc/rk4_affine_tiled.hip) behind CDE_VARIANT_AUTO, the workspace query, the argument checks of the two entry points at
these shapes, Choice.family, and a lane-level restatement of the index maps of cde_affine_tiled.h -- the Y tiles of both kernels,
the sweep's padded image, the va product, the G / Z factor rows and the gather of dW | db -- against plain einsum."""
import numpy as np
import pytest
import torch

import torchcde_amd
from torchcde_amd import _lib
from torchcde_amd import dispatch as D
from rejected_calls import CALLS, build_args

F32, F64 = _lib.F32, _lib.F64
INSIDE = [(17, 1), (17, 5), (21, 32), (36, 16), (64, 32), (64, 1)]            # (C, H)
OUTSIDE = [(16, 32), (8, 32), (65, 32), (21, 33), (21, 0)]


# ------------------------------------------------------------------------------------------------ the envelope
def test_tiled_envelope_and_what_the_other_variants_answer():
    lib = torchcde_amd.load()
    for C, H in INSIDE:
        for act in (_lib.ACT_NONE, _lib.ACT_TANH):
            assert lib.cde_rk4_affine_tiled_supported(C, H, F32, act) == 1, (C, H, act)
            for adjoint in (0, 1):
                assert lib.cde_rk4_supported(C, H, F32, act, adjoint, _lib.VARIANT_AUTO) == 1, (C, H, act)
                assert lib.cde_rk4_supported(C, H, F32, act, adjoint, _lib.VARIANT_MFMA) == 0, (C, H, act)
        assert lib.cde_rk4_affine_tiled_supported(C, H, F64, _lib.ACT_NONE) == 0, (C, H)
        assert lib.cde_rk4_affine_tiled_supported(C, H, F32, 2) == 0, (C, H)
        assert lib.cde_rk4_affine_tiled_supported(C, H, 7, _lib.ACT_NONE) == 0, (C, H)
    for C, H in OUTSIDE:
        for dtype in (F32, F64):
            assert lib.cde_rk4_affine_tiled_supported(C, H, dtype, _lib.ACT_NONE) == 0, (C, H, dtype)
    assert lib.cde_abi_version() == 3 == _lib.ABI_VERSION                     # the change is additive
    assert "cde_rk4_affine_tiled_supported" in _lib.EXPORTED_SYMBOLS


def test_adjoint_workspace_covers_either_kernel_and_grows_with_the_problem():
    lib = torchcde_amd.load()
    for C, H in INSIDE:
        last = 0
        for B in (1, 16, 17, 35, 4115, 32768):
            need = lib.cde_rk4_adjoint_workspace_bytes(B, C, H, 11, F32, _lib.VARIANT_AUTO)
            assert need >= lib.cde_rk4_adjoint_workspace_bytes(B, C, H, 11, F32, _lib.VARIANT_GENERIC), (C, H, B)
            assert need >= last, (C, H, B)
            last = need
        last = 0
        for n_sgrid in (0, 1, 2, 3, 11, 65, 1000):
            need = lib.cde_rk4_adjoint_workspace_bytes(35, C, H, n_sgrid, F32, _lib.VARIANT_AUTO)
            assert need >= last, (C, H, n_sgrid)
            last = need
    # one more RK step: its stage-table slots and 4 stages x 48 padded series x (G: 2048 + Z: 32) floats of factor rows
    step_rows = 4 * 48 * (2048 + 32) * 4
    one, two = (lib.cde_rk4_adjoint_workspace_bytes(35, 64, 32, n, F32, _lib.VARIANT_AUTO) for n in (2, 3))
    assert two - one == step_rows + _tables(2) - _tables(1)
    # the chunk budget bounds the factor rows: with room for two steps a long grid reserves only longer stage tables
    with torchcde_amd.tuning(wide_scratch_bytes=2 * step_rows):
        short, long = (lib.cde_rk4_adjoint_workspace_bytes(35, 64, 32, n, F32, _lib.VARIANT_AUTO) for n in (3, 11))
        assert long - short == _tables(10) - _tables(2)
        assert short == two


def _tables(n_steps):
    """[stage_index: 4 n_steps int64 | stage_frac: 4 n_steps f32], each part 256-byte aligned"""
    return (4 * n_steps * 8 + 255) // 256 * 256 + (4 * n_steps * 4 + 255) // 256 * 256


# ------------------------------------------------------------------------------------------------ the C ABI
AT = " C=21 H=32 variant=0"
# entry point -> {code: overrides of the valid call (tests/rejected_calls.py, at C = 21, H = 32 under AUTO) that must return it}:
# sizes (-3), an unknown activation / a variant without kernels here (-4), the forward solve's empty batch (0), an unknown dtype
# (-2), pointers (-1), the workspace one byte short (-5)
REJECTED = {
    "cde_rk4_forward_linear": {
        -3: ["C=0", "H=0", "n_intervals=0", "B=-1", "n_out=0", "n_grid=0", "H=0 coeffs=0"],
        -4: ["act=2", "act=17", "act=2 coeffs=0"],
        0: ["B=0", "B=0 coeffs=0"],
        -1: ["coeffs=0", "knots=0", "W=0", "bias=0", "z0=0", "grid=0", "t_out=0", "z_out=0", "stage_index=0", "stage_frac=0"],
        -2: ["dtype=7", "time_dtype=7"],
    },
    "cde_rk4_adjoint_linear": {
        -3: ["C=0", "H=0", "n_intervals=0", "B=0", "B=-1", "n_out=0", "n_sgrid=-1"],
        -4: ["act=2", "variant=2", "variant=3", "variant=4", "variant=9"],
        -1: ["coeffs=0", "knots=0", "W=0", "bias=0", "z_saved=0", "grad_out=0", "grad_z0=0", "grad_W=0", "grad_b=0", "workspace=0",
             "sgrid=0", "seg_off=0"],
        -2: ["dtype=7", "time_dtype=7"],
        -5: ["workspace_bytes=SHORT", "workspace_bytes=0"],
    },
}


def test_entry_points_reject_bad_calls_at_tiled_shapes_without_a_gpu():
    """Dummy pointers, no device: every row fails a check that comes before the first HIP call."""
    lib = torchcde_amd.load()
    need = lib.cde_rk4_adjoint_workspace_bytes(64, 21, 32, 5, F32, _lib.VARIANT_AUTO)
    wrong = []
    for name, by_code in REJECTED.items():
        call = getattr(lib, name)
        for code, cases in by_code.items():
            for overrides in cases:
                got = call(*build_args(CALLS[name], (AT + " " + overrides).replace("SHORT", str(need - 1))))
                if got != code:
                    wrong.append("%s(%s): %d, expected %d" % (name, overrides, got, code))
    assert not wrong, "\n".join(wrong)


# ------------------------------------------------------------------------------------------------ the dispatch record
def test_choice_family_is_an_attribute_beside_the_tuple():
    plain = D.Choice("rk4", "")
    assert plain.family == "" and plain.form == ""
    tiled = plain.with_form("exact", "tiled")
    assert (tiled.form, tiled.family) == ("exact", "tiled")
    assert tiled == plain == ("rk4", "") and hash(tiled) == hash(plain) and len(tiled) == 2
    assert plain.with_form("bf16x3").family == ""                            # the existing call keeps its meaning
    assert plain.family == ""                                                # ... and nothing leaks into the class


# ------------------------------------------------------------------------------------------------ the index maps
LANES = [(l & 15, l >> 4) for l in range(64)]                                 # lane -> (n, q)
ROWS, KW = 2048, 32                                                            # rows / columns of the sweep's padded image
SHAPES = [(5, 17), (32, 64)]                                                   # (H, C)


def _mfma_16x16x4(a_lane, b_lane, acc):
    """v_mfma_f32_16x16x4_f32: lane l supplies A[i=l&15][k=l>>4], B[k=l>>4][j=l&15]; register r of lane l holds
    D[4*(l>>4)+r][l&15] (tests/test_host.py), all 64 lanes at once."""
    P = np.asarray(a_lane).reshape(4, 16).T @ np.asarray(b_lane).reshape(4, 16)
    acc += P.reshape(4, 4, 16).transpose(0, 2, 1).reshape(64, 4)


def _flat_read(flat, at):
    assert 0 <= at < flat.size, "a read outside the tensor: %d of %d" % (at, flat.size)
    return flat[at]


def _inputs(H, C, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((H * C, H)) * 0.3, rng.standard_normal(H * C), rng.standard_normal((16, H)),
            rng.standard_normal((16, C)), rng.standard_normal((16, H)))


def _own(x, H):
    """a lane's state registers: register s of lane (n, q) = unit 8 q + s of series n, zero from H on"""
    reg = np.zeros((64, 8))
    for l, (n, q) in enumerate(LANES):
        for s in range(8):
            if 8 * q + s < H:
                reg[l, s] = x[n, 8 * q + s]
    return reg


def _dx(dX, n, tb, C):
    """the float4 of the dX slab a lane reads for tile tb: zero from C on"""
    out = np.zeros(4)
    out[:max(0, min(4, C - 4 * tb))] = dX[n, 4 * tb:4 * tb + 4]
    return out


@pytest.mark.parametrize("H,C", SHAPES)
def test_y_tiles_of_the_forward_kernel(H, C):
    """rk4_forward_affine_tiled: per unit group j and tile tb the lane's A operands from the caller's W (vector and scalar form:
    the same guards), the bias as the accumulator's initial value, the 8 K steps on the lane's OWN state registers, tanh and the
    contraction with the slab -- f for unit 8 q + j of series n, against einsum.  No read leaves W / b."""
    W, b, z, dX, _ = _inputs(H, C, 3)
    NJ, NB = min(H, 8), (C + 3) // 4
    wf, bf, zreg = W.ravel(), b.ravel(), _own(z, H)
    f = np.zeros((64, 8))

    def load_tile(j, tb):
        a = np.zeros((64, 8)); bias = np.zeros((64, 4))
        for l, (n, q) in enumerate(LANES):
            h, c = 8 * (n >> 2) + j, 4 * tb + (n & 3)
            for s in range(8):
                if j < NJ and h < H and c < C and 8 * q + s < H:
                    a[l, s] = _flat_read(wf, (h * C + c) * H + 8 * q + s)
            for r in range(4):
                if j < NJ and 8 * q + j < H and 4 * tb + r < C:
                    bias[l, r] = _flat_read(bf, (8 * q + j) * C + 4 * tb + r)
        return a, bias

    for j in range(NJ):
        for tb in range(NB):
            a, acc = load_tile(j, tb)
            for s in range(8):
                _mfma_16x16x4(a[:, s], zreg[:, s], acc)
            for l, (n, q) in enumerate(LANES):
                f[l, j] += np.tanh(acc[l]) @ _dx(dX, n, tb, C)
    for j, tb in ((NJ - 1, NB), (NJ, 0)):             # the requests past the last tile of a group / the last group give zeros
        a, bias = load_tile(j, tb)
        assert not a.any() and not bias.any()
    Y = np.tanh(z @ W.T + b).reshape(16, H, C)
    want = _own(np.einsum("nhc,nc->nh", Y, dX), H)
    assert np.allclose(f, want, rtol=1e-12, atol=1e-12)


def _image(W, b, H, C):
    """affine_tiled_image_kernel: [W plain [ROWS][32] | b [ROWS] | W for va [ROWS / 4][16][4][2]], rows h CP + c"""
    CP = (C + 3) // 4 * 4
    wp, bp, wt = np.zeros((ROWS, KW)), np.zeros(ROWS), np.zeros((ROWS // 4, 16, 4, 2))
    for row in range(ROWS):
        h, c = divmod(row, CP)
        if h < H and c < C:
            wp[row, :H] = W[h * C + c]
            bp[row] = b[h * C + c]
            for i in range(16):
                for T in range(2):
                    out = 8 * (i >> 2) + 4 * T + (i & 3)
                    if out < H:
                        wt[row // 4, i, row % 4, T] = W[h * C + c, out]
    return wp.ravel(), bp, wt.ravel()


@pytest.mark.parametrize("H,C", SHAPES)
def test_sweep_tiles_factor_rows_and_the_gradient_gather(H, C):
    """rk4_adjoint_affine_tiled_sweep on one (stage, series-tile): Y from the padded image, f, g = a_h dX_c (1 - tanh^2) into
    G [series][MP] at column h CP + c (every column below H CP written once, none beyond), Z [series][32], va = W^T g through the
    va copy onto the lane's own units; then acc = G^T [Z | 1] and affine_tiled_gather_kernel's map -- against einsum."""
    W, b, z, dX, a = _inputs(H, C, 5)
    CP, NJ, NB = (C + 3) // 4 * 4, min(H, 8), (C + 3) // 4
    MP = (H * CP + 255) // 256 * 256
    wp, bp, wt = _image(W, b, H, C)
    zreg, areg = _own(z, H), _own(a, H)
    G, written = np.zeros((16, MP)), np.zeros((16, MP), dtype=bool)
    Z = np.full((16, 32), np.nan)
    f, va = np.zeros((64, 8)), np.zeros((2, 64, 4))
    for l, (n, q) in enumerate(LANES):
        Z[n, 8 * q:8 * q + 8] = zreg[l]
    for j in range(NJ):
        for tb in range(NB):
            rows = j * CP + 4 * tb
            ay, acc, ag = np.zeros((64, 8)), np.zeros((64, 4)), np.zeros((64, 4, 2))
            for l, (n, q) in enumerate(LANES):
                y_off = (8 * (n >> 2) * CP + (n & 3)) * KW + 8 * q
                own_off = 8 * q * CP
                for s in range(8):
                    ay[l, s] = _flat_read(wp, rows * KW + y_off + s)
                for r in range(4):
                    acc[l, r] = _flat_read(bp, own_off + rows + r)
                    for T in range(2):
                        ag[l, r, T] = _flat_read(wt, (own_off + rows) * KW + 8 * n + 2 * r + T)
            for s in range(8):
                _mfma_16x16x4(ay[:, s], zreg[:, s], acc)
            t = np.tanh(acc)
            g = np.zeros((64, 4))
            for l, (n, q) in enumerate(LANES):
                dx = _dx(dX, n, tb, C)
                f[l, j] += t[l] @ dx
                g[l] = areg[l, j] * (dx * (1 - t[l] * t[l]))
                if 8 * q + j < H:
                    at = (8 * q + j) * CP + 4 * tb
                    assert not written[n, at:at + 4].any()
                    G[n, at:at + 4] = g[l]
                    written[n, at:at + 4] = True
            for r in range(4):
                for T in range(2):
                    _mfma_16x16x4(ag[:, r, T], g[:, r], va[T])
    assert written[:, :H * CP].all() and not written[:, H * CP:].any()
    assert not np.isnan(Z).any()
    Y = np.tanh(z @ W.T + b).reshape(16, H, C)
    g_want = a[:, :, None] * dX[:, None, :] * (1 - Y * Y)
    assert np.allclose(f, _own(np.einsum("nhc,nc->nh", Y, dX), H), rtol=1e-12, atol=1e-12)
    va_want = _own(g_want.reshape(16, H * C) @ W, H)          # register 4 T + r of lane (n, q) = unit 8 q + 4 T + r
    assert np.allclose(np.concatenate([va[0], va[1]], axis=1), va_want, rtol=1e-12, atol=1e-12)
    # the reduction acc (MP, 33) = G^T [Z | 1] and the gather into grad_W (H C, H), grad_b (H C)
    acc = G.T @ np.concatenate([Z, np.ones((16, 1))], axis=1)
    dW, db = np.zeros((H * C, H)), np.zeros(H * C)
    for e in range(H * C * (H + 1)):
        m, k = divmod(e, H + 1)
        h, c = divmod(m, C)
        v = acc[h * CP + c, k if k < H else 32]
        if k < H:
            dW[m, k] = v
        else:
            db[m] = v
    assert np.allclose(dW, np.einsum("nhc,nk->hck", g_want, z).reshape(H * C, H), rtol=1e-12, atol=1e-12)
    assert np.allclose(db, g_want.sum(0).reshape(H * C), rtol=1e-12, atol=1e-12)
