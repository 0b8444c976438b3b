"""CPU tests of the host logic: C-ABI library loads and exports what the header declares, error
behaviour mirrors the reference, solver grids equal the oracle's, field recognition, and a lane-level
emulation of the MFMA operand layouts used by csrc/rk4_mfma.hip (index math only -- no GPU compute)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import torchcde_amd
from torchcde_amd import _lib
from torchcde_amd.cdeint import _fixed_grid, _parse_fixed_options
from torchcde_amd.fields import probe
from oracle import odeint as oracle_ode
from helpers import LinearField

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the boundary
def test_library_builds_loads_and_exports_every_declared_symbol():
    torchcde_amd.build()
    lib = torchcde_amd.load()
    header = open(os.path.join(ROOT, "include", "cde_mi355x.h")).read()
    declared = set(re.findall(r"\b(cde_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_lib.EXPORTED_SYMBOLS), declared ^ set(_lib.EXPORTED_SYMBOLS)
    raw = ctypes.CDLL(_lib.SO_PATH)
    for name in declared:
        assert hasattr(raw, name), name
    assert lib.cde_abi_version() == 3
    assert lib.cde_error_string(0) == b"ok"
    assert b"workspace" in lib.cde_error_string(-5)


def test_tuning_table_is_explicit_and_restores_its_defaults():
    """The library reads no environment variable: kernel-form selectors live in one table that only cde_set_option writes
    (include/cde_mi355x.h, CDE_OPT_*).  Names and keys of the host mirror against the header's enum, defaults, the
    context manager's restore, and the source itself (getenv appears only inside the trace build's #ifdef)."""
    lib = torchcde_amd.load()
    header = open(os.path.join(ROOT, "include", "cde_mi355x.h")).read()
    enum = dict((name.lower(), int(val)) for name, val in re.findall(r"CDE_OPT_([A-Z0-9_]+) = (\d+)", header))
    count = enum.pop("count")
    assert enum == {name: key for name, (key, _) in _lib.OPTIONS.items()} and count == len(enum)
    lib.cde_reset_options()
    defaults = {name: torchcde_amd.get_option(name) for name in _lib.OPTIONS}
    assert defaults["k3_form"] == 0 and defaults["k3m_s8_tiles"] == -1 and defaults["wide_scratch_bytes"] == 0
    with torchcde_amd.tuning(k3_form="product", k3_waves=1, k4am_no_fsal=True, wide_scratch_bytes=12345):
        assert torchcde_amd.get_option("k3_form") == 1 and torchcde_amd.get_option("k3_waves") == 1
        assert torchcde_amd.get_option("k4am_no_fsal") == 1 and torchcde_amd.get_option("wide_scratch_bytes") == 12345
    assert {name: torchcde_amd.get_option(name) for name in _lib.OPTIONS} == defaults
    assert lib.cde_set_option(count, 1) != 0 and lib.cde_get_option(-1) == -2 ** 63
    with pytest.raises(KeyError):
        torchcde_amd.tuning(no_such_option=1)
    csrc = os.path.join(ROOT, "torchcde_amd", "csrc")
    for name in sorted(os.listdir(csrc)):
        guarded = False
        for line in open(os.path.join(csrc, name)):
            if line.startswith("#ifdef CDE_PHASE_TRACE"):
                guarded = True
            elif line.startswith("#else") or line.startswith("#endif"):
                guarded = False
            assert "getenv" not in line or guarded, (name, line)


def test_ctypes_signatures_match_the_header_prototypes():
    """Every prototype of include/cde_mi355x.h against the ctypes table of torchcde_amd/_lib.py: same number of
    parameters, pointers bound as c_void_p, integers / doubles / size_t as such, same return type."""
    header = open(os.path.join(ROOT, "include", "cde_mi355x.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    protos = re.findall(r"\b(int64_t|int|size_t|const char\*)\s+(cde_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", header, flags=re.S)
    assert len(protos) == len(_lib.EXPORTED_SYMBOLS)
    kinds = {ctypes.c_void_p: "ptr", ctypes.c_int: "int", ctypes.c_int64: "int64_t", ctypes.c_size_t: "size_t",
             ctypes.c_double: "double"}
    for ret, name, params in protos:
        restype, argtypes = _lib._SIGNATURES[name]
        params = [p.strip() for p in params.replace("\n", " ").split(",")] if params.strip() not in ("", "void") else []
        assert len(params) == len(argtypes), (name, len(params), len(argtypes))
        for text, ctype in zip(params, argtypes):
            want = "ptr" if "*" in text else text.split()[-2] if len(text.split()) > 1 else text
            assert kinds[ctype] == want, (name, text, ctype)
        assert {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t,
                "const char*": ctypes.c_char_p}[ret] is restype, name


def test_status_struct_mirror_matches_the_header():
    """cde_dopri5_status (include/cde_mi355x.h) against its ctypes mirror: same fields in the same order with the same
    widths -- the host reads the controller block of the adaptive kernels through it (112 bytes since the two interval
    hints were appended)."""
    header = open(os.path.join(ROOT, "include", "cde_mi355x.h")).read()
    body = re.search(r"typedef struct \{(.*?)\} cde_dopri5_status;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for ctype, names in re.findall(r"(double|int64_t|int32_t)\s+([^;]+);", body):
        fields += [(n.strip(), ctype) for n in names.split(",")]
    widths = {"double": ctypes.c_double, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32}
    assert [(n, widths[t]) for n, t in fields] == list(_lib.DopriStatus._fields_)
    assert ctypes.sizeof(_lib.DopriStatus) == 112


def test_argument_errors_come_back_as_codes_without_a_gpu():
    lib = torchcde_amd.load()
    null = ctypes.c_void_p(0)
    assert lib.cde_hermite_bdiff_coeffs(null, null, null, 4, 1, 3, 0, null) == -3      # L < 2
    assert lib.cde_hermite_bdiff_coeffs(null, null, null, 4, 5, 3, 0, null) == -1      # NULL pointers
    assert lib.cde_hermite_bdiff_coeffs(null, null, null, 0, 5, 3, 0, null) == 0       # empty batch is a no-op
    assert lib.cde_path_eval(null, null, null, 3, null, 2, 0, 3, 3, 1, 0, null) == -3
    assert lib.cde_rk4_adjoint_workspace_bytes(32768, 8, 32, 128, 0, 2) > 1024 * 8448 * 4
    # the fused solvers: every call of the table is turned away before the first HIP call, with the recorded code
    from rejected_calls import CALLS, REJECTED, build_args
    assert set(REJECTED) == set(CALLS)
    wrong = []
    for name, by_code in REJECTED.items():
        for code, cases in by_code.items():
            for overrides in cases:
                got = getattr(lib, name)(*build_args(CALLS[name], overrides))
                if got != code:
                    wrong.append("%s(%s): %d, expected %d" % (name, overrides, got, code))
    assert not wrong, "\n".join(wrong)


def test_adaptive_workspace_layouts_keep_their_recorded_sizes_and_offsets():
    """Every size / offset query of the adaptive solvers (K4, K4a, K4am) at default options against the values recorded
    in tests/rejected_calls.py: the batch sizes straddle every form switch of the layouts.  Pure host functions."""
    from rejected_calls import LAYOUT, LAYOUT_B, LAYOUT_CH
    lib = torchcde_amd.load()
    wrong = []
    for query, want in LAYOUT.items():
        name, _, extra = query.partition(" ")
        tail = [int(extra.partition("=")[2])] if extra else []
        call = getattr(lib, name)
        got = call() if isinstance(want, int) else [[call(B, C, H, *tail) for C, H in LAYOUT_CH] for B in LAYOUT_B]
        if got != want:
            wrong.append("%s: %r, expected %r" % (query, got, want))
    assert not wrong, "\n".join(wrong)


def test_no_cpu_fallback():
    x = torch.randn(2, 5, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        torchcde_amd.hermite_cubic_coefficients_with_backward_differences(x)
    X = torchcde_amd.CubicSpline(torch.randn(2, 4, 12))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        X.derivative(torch.tensor(0.5))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        torchcde_amd.cdeint(X, LinearField(4, 3), torch.randn(2, 4), X.interval, method="rk4")


def test_reference_error_messages():
    hermite = torchcde_amd.hermite_cubic_coefficients_with_backward_differences
    with pytest.raises(ValueError, match="floating point"):
        hermite(torch.zeros(3, 4, 2, dtype=torch.int64))
    with pytest.raises(ValueError, match="at least two dimensions"):
        hermite(torch.zeros(3))
    with pytest.raises(ValueError, match="monotonically increasing"):
        hermite(torch.zeros(2, 3, 1), torch.tensor([0., 2., 1.]))
    with pytest.raises(ValueError, match="time dimension of X must equal"):
        hermite(torch.zeros(2, 3, 1), torch.tensor([0., 1.]))
    with pytest.raises(ValueError, match="Passed invalid coeffs"):
        torchcde_amd.CubicSpline(torch.zeros(2, 3, 7))
    X = torchcde_amd.CubicSpline(torch.zeros(2, 3, 8))
    assert torch.equal(X.interval, torch.tensor([0., 3.]))
    assert torch.equal(X.grid_points, torch.linspace(0, 3, 4))
    assert set(dict(X.named_buffers())) == {"_t", "_a", "_b", "_two_c", "_three_d"}
    with pytest.raises(ValueError, match="X must have a 'derivative' method"):
        torchcde_amd.cdeint(object(), LinearField(4, 2), torch.zeros(2, 4), torch.tensor([0., 1.]))
    with pytest.raises(ValueError, match="Unrecognised backend=foo"):
        torchcde_amd.cdeint(X, LinearField(4, 2), torch.zeros(2, 4), torch.tensor([0., 1.]), backend="foo")
    with pytest.raises(ValueError, match="z0 must either a tensor"):
        torchcde_amd.cdeint(X, LinearField(4, 2), 3.0, torch.tensor([0., 1.]))


def test_packed_view_is_recovered_without_copy():
    coeffs = torch.randn(3, 5, 16)
    X = torchcde_amd.CubicSpline(coeffs)
    packed = X._packed()
    assert packed.data_ptr() == coeffs.data_ptr() and torch.equal(packed, coeffs)
    Y = torchcde_amd.CubicSpline(coeffs).double()          # buffers re-materialised separately
    assert torch.equal(Y._packed(), coeffs.double())


# ------------------------------------------------------------------ solver grids
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_fixed_grid_equals_oracle(dtype):
    for lo, hi, h in ((0., 127., 1.0), (0., 9., 0.7), (0.3, 4.1, 0.25), (-2., 3., 10.)):
        t = torch.tensor([lo, (lo + hi) / 2, hi], dtype=dtype)
        assert torch.equal(_fixed_grid(t, h), oracle_ode._grid_from_step(t, h))
    t = torch.tensor([0., 1., 4.], dtype=dtype)
    assert torch.equal(_fixed_grid(t, None), t)            # torchdiffeq: no step_size => grid = t


def test_option_parsing():
    assert _parse_fixed_options(dict(step_size=0.5), "solver") == 0.5
    assert _parse_fixed_options(None, "solver") is None
    with pytest.raises(NotImplementedError):
        _parse_fixed_options(dict(grid_constructor=lambda *a: None), "solver")
    with pytest.raises(NotImplementedError):
        _parse_fixed_options(dict(step_size=1.0, bogus=1), "solver")


# ------------------------------------------------------------------ vector-field recognition
def test_probe_accepts_exactly_the_fused_families():
    z, t = torch.randn(4, 3), torch.tensor(0.25)

    class Readme(torch.nn.Module):                       # reference README.md:42-49
        def __init__(self):
            super().__init__()
            self.linear = torch.nn.Linear(3, 6)

        def forward(self, t, z):
            return self.linear(z).view(4, 3, 2)

    class Irregular(Readme):                             # reference example/irregular_data.py:36-46
        def forward(self, t, z):
            return self.linear(z).tanh().view(*z.shape[:-1], 3, 2)

    class TimeDependent(Readme):
        def forward(self, t, z):
            return (self.linear(z) * (1 + t)).view(4, 3, 2)

    class Scaled(Readme):
        def forward(self, t, z):
            return (self.linear(z) * 1.0001).view(4, 3, 2)

    class TwoLayer(torch.nn.Module):                     # example/time_series_classification.py:37-51
        def __init__(self):
            super().__init__()
            self.l1, self.l2 = torch.nn.Linear(3, 5), torch.nn.Linear(5, 6)

        def forward(self, t, z):
            return self.l2(self.l1(z).relu()).tanh().view(4, 3, 2)

    field, system = probe(Readme(), t, z)
    assert field is not None and field.act == _lib.ACT_NONE and system.shape == (4, 3, 2)
    field, _ = probe(Irregular(), t, z)
    assert field is not None and field.act == _lib.ACT_TANH
    field, _ = probe(torchcde_amd.LinearCDEFunc(2, 3, tanh=True), t, z)
    assert field is not None and field.act == _lib.ACT_TANH
    field, system = probe(TwoLayer(), t, z)
    assert field is not None and field.kind == "mlp2" and field.act == _lib.ACT_TANH and system.shape == (4, 3, 2)
    assert field.hidden.out_features == 5 and field.output.out_features == 6

    class TwoLayerTanhInside(TwoLayer):                  # another hidden activation: not the fused formula
        def forward(self, t, z):
            return self.l2(self.l1(z).tanh()).tanh().view(4, 3, 2)

    class TwoLayerSkip(TwoLayer):
        def forward(self, t, z):
            return (self.l2(self.l1(z).relu()) + z.repeat(1, 2)).tanh().view(4, 3, 2)

    class SharedLayer(torch.nn.Module):                  # one Linear applied twice
        def __init__(self):
            super().__init__()
            self.l = torch.nn.Linear(3, 3)
            self.out = torch.nn.Linear(3, 6)

        def forward(self, t, z):
            return self.out(self.l(self.l(z).relu()).relu()).view(4, 3, 2)

    for bad in (TimeDependent(), Scaled(), TwoLayerTanhInside(), TwoLayerSkip(), SharedLayer()):
        field, system = probe(bad, t, z)
        assert field is None and system.shape == (4, 3, 2)

    class WithDropout(Readme):                           # identity in eval(), random in train()
        def __init__(self):
            super().__init__()
            self.drop = torch.nn.Dropout(0.5)

        def forward(self, t, z):
            return self.drop(self.linear(z)).view(4, 3, 2)

    module = WithDropout().eval()
    assert probe(module, t, z)[0] is not None            # verified (and cached) as the affine field
    assert probe(module, t, z)[0] is not None
    module.train()
    assert probe(module, t, z)[0] is None                # the cached verdict does not survive the mode switch


# ------------------------------------------------------------------ MFMA operand layouts (emulated)
def _mfma_32x32x2(a_lane, b_lane, acc):
    """v_mfma_f32_32x32x2_f32 lane semantics (cdna_hip_programming.md section 3): lane l supplies
    A[i=l&31][k=l>>5] and B[k=l>>5][j=l&31]; register r of lane l holds D[(r&3)+8(r>>2)+4(l>>5)][l&31]."""
    A = np.zeros((32, 2)); Bm = np.zeros((2, 32))
    for l in range(64):
        A[l & 31, l >> 5] = a_lane[l]
        Bm[l >> 5, l & 31] = b_lane[l]
    P = A @ Bm
    for l in range(64):
        for r in range(16):
            acc[l, r] += P[(r & 3) + 8 * (r >> 2) + 4 * (l >> 5), l & 31]


def _rho(i):
    return 2 * ((i & 3) + 4 * (i >> 3)) + ((i >> 2) & 1)


def _w1_image(W, bias, s, l, H=32, C=8):
    h_out, hk = _rho(l & 31), l >> 5
    if s < 128:
        j, c = s >> 3, s & 7
        return W[(h_out * C + c), 2 * j + hk]
    return bias[h_out * C + 2 * (s - 128) + hk]


def _w2_image(W, s, l, H=32, C=8):
    k_out, hk = _rho(l & 31), l >> 5
    j, c = s >> 3, s & 7
    return W[(2 * j + hk) * C + c, k_out]


def test_mfma_operand_layouts_reproduce_the_vector_field_and_its_vjps():
    rng = np.random.default_rng(0)
    H, C = 32, 8
    W = rng.standard_normal((H * C, H)); bias = rng.standard_normal(H * C)
    z = rng.standard_normal((32, H)); a = rng.standard_normal((32, H)); dX = rng.standard_normal((32, C))
    Y = z @ W.T + bias                                            # (32, H*C)
    f_ref = np.einsum("nhc,nc->nh", Y.reshape(32, H, C), dX)
    gY = (a[:, :, None] * dX[:, None, :]).reshape(32, H * C)      # a_h dX_c
    vjp_ref = gY @ W                                              # (a^T df/dz)
    gW_ref = gY.T @ z                                             # dL/dW
    gb_ref = gY.sum(0)

    lanes = np.arange(64)
    n, half = lanes & 31, lanes >> 5
    own = lambda v: np.stack([v[n, 2 * r + half] for r in range(16)], axis=1)   # lane register r <-> unit 2r+half
    z_own, a_own = own(z), own(a)

    # f chain (chain_field): 128 product steps + 4 bias steps
    acc = np.zeros((64, 16))
    for j in range(16):
        for c in range(8):
            s = 8 * j + c
            _mfma_32x32x2([_w1_image(W, bias, s, l) for l in lanes], z_own[:, j] * dX[n, c], acc)
    for sp in range(4):
        _mfma_32x32x2([_w1_image(W, bias, 128 + sp, l) for l in lanes], dX[n, 2 * sp + half], acc)
    assert np.allclose(acc, own(f_ref))

    # vjp chain (chain_vjp)
    acc = np.zeros((64, 16))
    for j in range(16):
        for c in range(8):
            _mfma_32x32x2([_w2_image(W, 8 * j + c, l) for l in lanes], a_own[:, j] * dX[n, c], acc)
    assert np.allclose(acc, own(vjp_ref))

    # dL/dW through the (series -> K) LDS transpose (layout of rk4_adjoint_mfma):
    #   scr_zt[(par*32 + u)*20 + s] = z_u of series 2s+par,  scr_dw[series*8 + c] = wq*dX_c
    wq = 0.375
    scr_zt = np.zeros(64 * 20); scr_at = np.zeros(64 * 20); scr_dw = np.zeros(32 * 8)
    for l in lanes:
        for r in range(16):
            scr_zt[((n[l] & 1) * 32 + half[l]) * 20 + (n[l] >> 1) + r * 40] = z_own[l, r]
            scr_at[((n[l] & 1) * 32 + half[l]) * 20 + (n[l] >> 1) + r * 40] = a_own[l, r]
        scr_dw[n[l] * 8 + 4 * half[l]: n[l] * 8 + 4 * half[l] + 4] = wq * dX[n[l], 4 * half[l]: 4 * half[l] + 4]
    accW = np.zeros((8, 64, 16)); gb = np.zeros((64, 8))
    for s2 in range(16):
        zb = scr_zt[(half * 32 + n) * 20 + s2]          # reader lane (k = n, half) -> series 2*s2 + half
        aa = scr_at[(half * 32 + n) * 20 + s2]          # row h = n
        for c in range(8):
            d = scr_dw[(2 * s2 + half) * 8 + c]
            gb[:, c] += aa * d
            _mfma_32x32x2(aa * d, zb, accW[c])
    gW = np.zeros((H * C, H)); gbv = np.zeros(H * C)
    for l in lanes:
        for c in range(8):
            for r in range(16):
                h = (r & 3) + 8 * (r >> 2) + 4 * half[l]
                gW[h * C + c, n[l]] = accW[c, l, r]
            if half[l] == 0:
                gbv[n[l] * C + c] = gb[l, c] + gb[l + 32, c]
    assert np.allclose(gW, wq * gW_ref) and np.allclose(gbv, wq * gb_ref)


# ------------------------------------------------------------------ 16x16x4 layouts (forward kernel, 2 waves/SIMD)
def _mfma_16x16x4(a_lane, b_lane, acc):
    """v_mfma_f32_16x16x4_f32: lane l supplies A[i=l&15][k=l>>4], B[k=l>>4][j=l&15]; register r of lane l
    holds D[4*(l>>4)+r][l&15]."""
    A = np.zeros((16, 4)); Bm = np.zeros((4, 16))
    for l in range(64):
        A[l & 15, l >> 4] = a_lane[l]
        Bm[l >> 4, l & 15] = b_lane[l]
    P = A @ Bm
    for l in range(64):
        for r in range(4):
            acc[l, r] += P[4 * (l >> 4) + r, l & 15]


def _w16_image(W, bias, T, s, l, H=32, C=8):
    """A operand of M-tile T for step s (mirrors w16_image in csrc/rk4_mfma.hip): lane quarter q owns hidden
    units 8q..8q+7; tile T row i is unit 8*(i>>2) + 4*T + (i&3)."""
    i, kq = l & 15, l >> 4
    unit_out = 8 * (i >> 2) + 4 * T + (i & 3)
    if s < 64:
        m, c = s >> 3, s & 7
        return W[unit_out * C + c, 8 * kq + m]
    return bias[unit_out * C + 4 * (s - 64) + kq]


def test_mfma16_forward_layout_reproduces_the_vector_field():
    rng = np.random.default_rng(1)
    H, C = 32, 8
    W = rng.standard_normal((H * C, H)); bias = rng.standard_normal(H * C)
    z = rng.standard_normal((16, H)); dX = rng.standard_normal((16, C))
    f_ref = np.einsum("nhc,nc->nh", (z @ W.T + bias).reshape(16, H, C), dX)
    lanes = np.arange(64)
    n, q = lanes & 15, lanes >> 4
    z_own = np.stack([z[n, 8 * q + m] for m in range(8)], axis=1)
    acc = [np.zeros((64, 4)), np.zeros((64, 4))]
    for m in range(8):
        for c in range(8):
            b = z_own[:, m] * dX[n, c]
            for T in range(2):
                _mfma_16x16x4([_w16_image(W, bias, T, 8 * m + c, l) for l in lanes], b, acc[T])
    for sp in range(2):
        b = dX[n, 4 * sp + q]
        for T in range(2):
            _mfma_16x16x4([_w16_image(W, bias, T, 64 + sp, l) for l in lanes], b, acc[T])
    got = np.concatenate(acc, axis=1)                       # register 4T + r  <->  unit 8q + 4T + r
    expect = np.stack([f_ref[n, 8 * q + m] for m in range(8)], axis=1)
    assert np.allclose(got, expect)


# ------------------------------------------------------------------ pre-activation / two-layer layouts (emulated)
def _lane_units(n, q):
    """field_act16 / field_mlp16 ownership: lane (n, q) holds hidden units q, 4+q, .., 28+q of series n."""
    return [4 * m + q for m in range(8)]


def test_preactivation_tiling_reproduces_tanh_field_and_two_layer_field():
    """Lane-level emulation of cde_mfma.h: field_act16 and field_mlp16 (index math of the weight/bias images, the
    in-lane contraction with dX, and the register hand-over from layer 1 to layer 2)."""
    rng = np.random.default_rng(5)
    H, C, Wd = 32, 8, 128
    z = rng.standard_normal((16, H))
    dX = rng.standard_normal((16, C))
    lanes = [(l & 15, l >> 4) for l in range(64)]

    # ---- one layer + tanh: tile T = 2P + tb, row i <-> (h = 4P + (i>>2), c = 4tb + (i&3)), K step s feeds unit 4s + kq
    W = rng.standard_normal((H * C, H)) * 0.2
    b = rng.standard_normal(H * C) * 0.2
    want = np.einsum("nhc,nc->nh", np.tanh(z @ W.T + b).reshape(16, H, C), dX)
    got = np.zeros((16, H))
    for P in range(8):
        acc = [np.zeros((64, 4)), np.zeros((64, 4))]
        for tb in range(2):
            for l, (n, q) in enumerate(lanes):                       # bias = initial accumulator: by16_image(T, q, r)
                for r in range(4):
                    acc[tb][l, r] = b[(4 * P + q) * C + 4 * tb + r]
            for s in range(8):
                a_lane = [W[(4 * P + (i >> 2)) * C + 4 * tb + (i & 3), 4 * s + kq] for i, kq in lanes]   # wy16_image
                b_lane = [z[n, _lane_units(n, kq)[s]] for n, kq in lanes]                                # own register s
                _mfma_16x16x4(a_lane, b_lane, acc[tb])
        for l, (n, q) in enumerate(lanes):
            y = np.concatenate([acc[0][l], acc[1][l]])                # channels 0..7 of unit 4P+q, all in this lane
            got[n, 4 * P + q] = np.tanh(y) @ dX[n]
    assert np.allclose(got, want, rtol=1e-12, atol=1e-12)

    # ---- two layers: layer-1 C/D fragment (unit 16*T1 + 4q + r) is layer 2's B operand of K step (T1, r)
    W1 = rng.standard_normal((Wd, H)) * 0.2
    b1 = rng.standard_normal(Wd) * 0.2
    W2 = rng.standard_normal((H * C, Wd)) * 0.1
    b2 = rng.standard_normal(H * C) * 0.1
    hidden = np.maximum(z @ W1.T + b1, 0)
    want = np.einsum("nhc,nc->nh", np.tanh(hidden @ W2.T + b2).reshape(16, H, C), dX)
    u = np.zeros((64, 32))                                            # per-lane registers u[4*T1 + r]
    for T1 in range(8):
        acc = np.zeros((64, 4))
        for l, (n, q) in enumerate(lanes):
            for r in range(4):
                acc[l, r] = b1[16 * T1 + 4 * q + r]
        for s in range(8):
            a_lane = [W1[16 * T1 + i, 4 * s + kq] for i, kq in lanes]
            b_lane = [z[n, 4 * s + kq] for n, kq in lanes]
            _mfma_16x16x4(a_lane, b_lane, acc)
        u[:, 4 * T1:4 * T1 + 4] = np.maximum(acc, 0)
    for l, (n, q) in enumerate(lanes):                                # ownership claimed in the header comment
        for T1 in range(8):
            assert np.allclose(u[l, 4 * T1:4 * T1 + 4], hidden[n, 16 * T1 + 4 * q:16 * T1 + 4 * q + 4])
    got = np.zeros((16, H))
    for P in range(8):
        acc = [np.zeros((64, 4)), np.zeros((64, 4))]
        for tb in range(2):
            for l, (n, q) in enumerate(lanes):
                for r in range(4):
                    acc[tb][l, r] = b2[(4 * P + q) * C + 4 * tb + r]
            for T1 in range(8):
                for j in range(4):                                    # K step (T1, r = j): column 16*T1 + 4*kq + j
                    a_lane = [W2[(4 * P + (i >> 2)) * C + 4 * tb + (i & 3), 16 * T1 + 4 * kq + j] for i, kq in lanes]
                    b_lane = [u[l, 4 * T1 + j] for l in range(64)]
                    _mfma_16x16x4(a_lane, b_lane, acc[tb])
        for l, (n, q) in enumerate(lanes):
            got[n, 4 * P + q] = np.tanh(np.concatenate([acc[0][l], acc[1][l]])) @ dX[n]
    assert np.allclose(got, want, rtol=1e-12, atol=1e-12)


def test_plain_w2_copy_permutation_is_bijective_and_bank_conflict_free():
    """rk4_mlp_adjoint.hip keeps ONE copy of W2 in LDS (row stride 132 floats, permuted rows) for two access patterns.
    Checks: the row permutation is a bijection, the lane-offset formulas of the kernel address the intended element, a
    ds_read_b128 wave access puts every 8-lane group on 8 distinct 16-byte bank slots, and a ds_read_b32 access puts
    each half-wave on 32 distinct banks."""
    S = 132

    def residue(h3, c3):
        return (2 * (((h3 & 1) << 1) | (h3 >> 1)) + c3) & 7

    def prow(h, c):
        return ((h >> 2) * 4 + (c >> 2) * 2 + ((h >> 1) & 1)) * 8 + residue(h & 3, c & 3)

    assert {prow(h, c) for h in range(32) for c in range(8)} == set(range(256))
    for P in range(8):
        for c in range(8):
            tb = c >> 2
            for T1 in range(8):
                for half in range(2):                                 # gu: lane (n, q) reads row (4P+q, c), column 16*T1 + n
                    banks = set()
                    for l in range(32 * half, 32 * half + 32):
                        n, q = l & 15, l >> 4
                        off = ((q >> 1) * 8 + residue(q, c & 3)) * S + n + (4 * P + 2 * tb) * 8 * S + 16 * T1
                        assert off == prow(4 * P + q, c) * S + 16 * T1 + n
                        banks.add(off % 32)
                    assert len(banks) == 32
                for group in range(8):                                # Y2: lane (n, q) reads 4 floats of row (4P+(n>>2), 4tb+(n&3))
                    slots = set()
                    for l in range(8 * group, 8 * group + 8):
                        n, q = l & 15, l >> 4
                        off = ((n >> 3) * 8 + residue(n >> 2, n & 3)) * S + 4 * q + (4 * P + 2 * tb) * 8 * S + 16 * T1
                        assert off == prow(4 * P + (n >> 2), 4 * tb + (n & 3)) * S + 16 * T1 + 4 * q and off % 4 == 0
                        slots.add((off // 4) % 8)
                    assert len(slots) == 8


def test_probe_refuses_value_dependent_lookalikes_and_tracks_module_state():
    """relu6 / hardtanh / clamp agree with relu / identity on small values; a Python switch or a patched
    forward changes the field without changing a parameter.  The probe must refuse / re-verify (CPU tensors: the probe
    is host logic)."""
    import torch
    from torchcde_amd.fields import probe, LinearCDEFunc
    z = torch.randn(5, 4) * 1e-3
    t0 = torch.tensor(0.)

    class Relu6(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a, self.b = torch.nn.Linear(4, 16), torch.nn.Linear(16, 12)

        def forward(self, t, z):
            return self.b(torch.nn.functional.relu6(self.a(z))).tanh().view(-1, 4, 3)

    class HardTanh(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a = torch.nn.Linear(4, 12)

        def forward(self, t, z):
            return torch.nn.functional.hardtanh(self.a(z)).view(-1, 4, 3)

    class Clamp(HardTanh):
        def forward(self, t, z):
            return self.a(z).clamp(-1, 1).view(-1, 4, 3)

    class Dropout(HardTanh):
        def __init__(self):
            super().__init__()
            self.drop = torch.nn.Dropout(0.5)

        def forward(self, t, z):
            return self.drop(self.a(z)).view(-1, 4, 3)

    for cls in (Relu6, HardTanh, Clamp):
        assert probe(cls(), t0, z)[0] is None, cls.__name__
    d = Dropout().eval()
    assert probe(d, t0, z)[0] is not None                      # eval mode: dropout is the identity, no operator runs
    d.train()                                                  # the train flag is part of the fingerprint: probed again,
    assert probe(d, t0, z)[0] is None                          # and now a foreign operator shows up

    f = LinearCDEFunc(3, 4)
    assert probe(f, t0, z)[0].act == 0
    assert probe(f, t0, z)[1].device.type == "meta"            # cached: no second evaluation
    f.use_tanh = True                                          # plain attribute flips the field
    assert probe(f, t0, z)[0].act == 1
    f.forward = lambda t, zz: f.linear(zz).view(-1, 4, 3) * 2  # instance-level monkey patch
    assert probe(f, t0, z)[0] is None
    g = LinearCDEFunc(3, 4)
    assert probe(g, t0, z)[0] is not None
    original = LinearCDEFunc.forward
    try:
        LinearCDEFunc.forward = lambda self, t, zz: self.linear(zz).view(-1, 4, 3) + 1.0   # class-level patch
        assert probe(g, t0, z)[0] is None
    finally:
        LinearCDEFunc.forward = original
    assert probe(g, t0, z)[0] is not None


def test_closed_form_adjoint_dynamics_equal_autograd(monkeypatch):
    """stepwise._explicit_dynamics (the augmented dynamics of the continuous adjoint written out for a recognised
    field) against torch.autograd.grad on the same module: affine / tanh / two-layer fields, a Linear without bias,
    parameters given as a reordered subset and as views of the same memory (what backward() gets back from
    save_for_backward), extra batch dimensions; a parameter the field does not own makes it step aside."""
    from torchcde_amd import stepwise

    class CpuContract:                                    # cde_contract needs the GPU; the formula is all that matters here
        @staticmethod
        def apply(F, dX):
            return (F * dX.unsqueeze(-2)).sum(-1)

    monkeypatch.setattr(stepwise, "_Contract", CpuContract)

    class Path:
        def __init__(self, slope):
            self.slope = slope

        def derivative(self, t):
            return self.slope * (1 + t)

    class Two(torch.nn.Module):
        def __init__(self, H, C, width, final_tanh, bias):
            super().__init__()
            self.H, self.C, self.final_tanh = H, C, final_tanh
            self.a, self.b = torch.nn.Linear(H, width, bias=bias), torch.nn.Linear(width, H * C, bias=bias)

        def forward(self, t, z):
            y = self.b(self.a(z).relu())
            return (y.tanh() if self.final_tanh else y).view(*z.shape[:-1], self.H, self.C)

    class One(torch.nn.Module):
        def __init__(self, H, C, tanh, bias):
            super().__init__()
            self.H, self.C, self.tanh = H, C, tanh
            self.lin = torch.nn.Linear(H, H * C, bias=bias)

        def forward(self, t, z):
            y = self.lin(z)
            return (y.tanh() if self.tanh else y).view(*z.shape[:-1], self.H, self.C)

    torch.manual_seed(3)
    H, C = 5, 3
    for lead in ((7,), (2, 4)):
        for func in (One(H, C, False, True), One(H, C, True, True), Two(H, C, 9, True, True), Two(H, C, 9, False, True)):
            func = func.double()
            y = torch.randn(*lead, H, dtype=torch.float64)
            a = torch.randn(*lead, H, dtype=torch.float64)
            t = torch.tensor(0.3, dtype=torch.float64)
            recognised, _ = probe(func, t, y)
            assert recognised is not None
            field = stepwise.ControlledField(Path(torch.randn(*lead, C, dtype=torch.float64)), func)
            field.recognised = recognised
            params = tuple(reversed([p for p in func.parameters()]))[:3]
            saved = tuple(p.detach().view_as(p) for p in params)          # same memory, different tensor objects
            run = stepwise._explicit_dynamics(field, saved)
            assert run is not None
            with torch.no_grad():
                fe, vy, vp = run(t, y, a)
            yy = y.clone().requires_grad_(True)
            want_f = field(t, yy)
            want = torch.autograd.grad(want_f, (yy,) + params, -a, allow_unused=True)
            assert torch.allclose(fe, want_f.detach(), rtol=1e-12, atol=1e-13)
            assert torch.allclose(vy, want[0], rtol=1e-11, atol=1e-12)
            for got, ref, p in zip(vp, want[1:], params):
                assert got.shape == p.shape
                assert torch.allclose(got, ref, rtol=1e-11, atol=1e-12)
            stranger = torch.nn.Parameter(torch.zeros(3, dtype=torch.float64))
            assert stepwise._explicit_dynamics(field, saved + (stranger,)) is None
    plain = stepwise.ControlledField(Path(torch.zeros(1, C)), func)
    assert stepwise._explicit_dynamics(plain, ()) is None                # not recognised: autograd


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_stepwise_solvers_equal_the_oracle_bitwise_on_plain_functions(dtype):
    """torchcde_amd/stepwise.py drives torchdiffeq's time stepping from the host; on a plain tensor function (no native
    kernel involved, so this runs without a GPU) it must reproduce oracle/odeint.py -- the restatement of torchdiffeq --
    bit for bit: dopri5 with and without jump times, increasing and decreasing output times, two output times inside
    one step, tuple state; rk4 / midpoint / euler on a fixed grid."""
    from torchcde_amd import stepwise
    torch.manual_seed(0)
    A = (torch.randn(6, 6, dtype=torch.float64) * 0.5).to(dtype)

    def f(t, y):
        return torch.tanh(y @ A.T) * (1 + 0.1 * torch.sin(t))

    y0 = torch.randn(4, 6, dtype=torch.float64).to(dtype)
    for t in (torch.tensor([0., 0.7, 1.9, 1.95, 3.0], dtype=dtype), torch.tensor([3.0, 1.1, 0.], dtype=dtype)):
        for opts in ({}, {"jump_t": torch.tensor([0.5, 1.5, 2.5], dtype=dtype)}):
            got = stepwise.odeint(f, y0, t, method="dopri5", options=dict(opts), rtol=1e-5, atol=1e-7)
            want = oracle_ode.odeint(f, y0, t, method="dopri5", options=dict(opts), rtol=1e-5, atol=1e-7)
            assert torch.equal(got, want)
    ts = torch.tensor([0., 1., 2.], dtype=dtype)
    g = lambda t, s: (f(t, s[0]), -s[1])
    got = stepwise.odeint(g, (y0, y0[:, :2]), ts, method="dopri5", options={}, rtol=1e-6, atol=1e-8)
    want = oracle_ode.odeint(g, (y0, y0[:, :2]), ts, method="dopri5", options={}, rtol=1e-6, atol=1e-8)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    grid = torch.tensor([0., 0.7, 1.9, 3.0], dtype=dtype)
    for method in ("rk4", "midpoint", "euler"):
        got = stepwise.odeint(f, y0, grid, method=method, options=dict(step_size=0.25), rtol=0, atol=0)
        want = oracle_ode.odeint(f, y0, grid, method=method, options=dict(step_size=0.25), rtol=0, atol=0)
        assert torch.equal(got, want)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_stepwise_adjoint_equals_the_oracle_adjoint_on_plain_modules(dtype):
    """The host-driven continuous adjoint (stepwise._Adjoint: augmented state, per-interval reverse solves, re-seeding
    from the stored solution, output-time gradients) against oracle/odeint.py's restatement of torchdiffeq's
    odeint_adjoint on a plain nn.Module (no native kernel: runs without a GPU): trajectories and the gradients of z0
    and of every parameter bit for bit, dL/dt to round-off (a sum against a dot product).  rk4 and dopri5, jump times.
    When `t` needs no gradient the module is time-independent: torchdiffeq's wrapper hands func a time that ALWAYS
    carries requires_grad (its detach shares the tensor), so for a time-dependent func its |vjp_t| error component is
    alive even then; the native paths compute vjp_t only when dL/dt is asked for."""
    from torchcde_amd import stepwise

    class Field(torch.nn.Module):
        def __init__(self, timed):
            super().__init__()
            torch.manual_seed(1)
            self.lin = torch.nn.Linear(5, 5).to(dtype)
            self.scale = torch.nn.Parameter(torch.tensor(0.3, dtype=dtype))
            self.timed = timed

        def forward(self, t, y):
            return torch.tanh(self.lin(y)) * self.scale * ((1 + 0.2 * torch.cos(t)) if self.timed else 1.0)

    for method, opts in (("rk4", dict(step_size=0.25)), ("dopri5", {}),
                         ("dopri5", {"jump_t": torch.tensor([0.5, 1.5], dtype=dtype)})):
        for need_t in (False, True):
            results = []
            for which in ("native", "oracle"):
                func = Field(need_t)
                y0 = torch.randn(3, 5, generator=torch.Generator().manual_seed(2), dtype=torch.float64).to(dtype)
                y0.requires_grad_(True)
                t = torch.tensor([0., 0.8, 2.0], dtype=dtype, requires_grad=need_t)
                if which == "native":
                    cfg = dict(func=func, method=method, options=dict(opts), rtol=1e-5, atol=1e-7, adjoint_method=method,
                               adjoint_options=dict(opts), adjoint_rtol=1e-5, adjoint_atol=1e-7, t_requires_grad=need_t)
                    out = stepwise._Adjoint.apply(cfg, y0, t, *func.parameters())
                else:
                    out = oracle_ode.odeint_adjoint(func, y0, t, method=method, options=dict(opts), rtol=1e-5, atol=1e-7)
                (out * torch.linspace(0.5, 1.5, out.numel(), dtype=dtype).view_as(out)).sum().backward()
                results.append(([out.detach(), y0.grad] + [p.grad for p in func.parameters()], t.grad))
            (got, got_t), (want, want_t) = results
            assert all(torch.equal(a, b) for a, b in zip(got, want)), (method, need_t)
            if need_t:
                assert torch.allclose(got_t, want_t, rtol=1e-5 if dtype == torch.float32 else 1e-13, atol=1e-6 if dtype == torch.float32 else 1e-14)


def test_log_ode_window_bookkeeping_equals_the_reference_loop():
    """torchcde_amd/log_ode.py evaluates the reference's per-window Python loop (log_ode.py:18-49: `value <= t[pointer]`
    or allclose, pointer never moving back) for all window ends at once; oracle.logsig.window_plan restates the loop
    itself (pinned to the reference by tests/golden/logsig_windows.pt).  Same boundary rows, same fresh times, same
    merged order -- regular and irregular times, window lengths that divide the span, overshoot it, or land within
    allclose of an observation time."""
    from oracle import logsig as oracle_logsig
    from torchcde_amd import log_ode
    gen = torch.Generator().manual_seed(5)
    cases = []
    for dtype in (torch.float32, torch.float64):
        regular = torch.linspace(0, 16, 17, dtype=dtype)
        irregular = (torch.rand(23, generator=gen, dtype=torch.float64) + 0.2).cumsum(0).to(dtype)
        for t in (regular, irregular, regular * 0.37 + 2.0):
            span = (t[-1] - t[0]).item()
            for window in (span / 4, span / 4 * (1 + 1e-9), 3.0, 2.6, span, span * 1.7, 1.0, 0.73):
                cases.append((t, float(window)))
    assert len(cases) == 48
    for t, window in cases:
        new_t, rows, fresh = oracle_logsig.window_plan(t, window)
        log_ode._plans.clear()
        plan = log_ode._plan(t, True, window, t.numel(), 3, 2, 1, t.dtype, torch.device("cpu"))
        assert plan["rows"].tolist() == rows
        assert plan["n_windows"] == len(rows) - 1
        assert torch.equal(plan["new_t"], new_t)
        if fresh:
            merged, order = torch.cat([t, *fresh]).sort()
            assert torch.equal(plan["merged"], merged)
            assert torch.equal(plan["order"], order.clamp(0, t.numel()))
        else:
            assert plan["order"] is None and plan["merged"] is None
        scale0 = log_ode._plan(t, True, window, t.numel(), 3, 2, 0, t.dtype, torch.device("cpu"))["scale"]
        assert torch.equal(scale0, (new_t[1:] - new_t[:-1]).to(t.dtype))
    # the word table: signatory's order (by length, then lexicographic), flat index = base-C digits of the word
    words = log_ode._plan(regular, True, 4.0, 17, 3, 3, 1, torch.float64, torch.device("cpu"))["words"].tolist()
    assert [tuple(w) for w in words[:6]] == [(1, 0), (1, 1), (1, 2), (2, 1), (2, 2), (2, 5)]
    assert len(words) == log_ode.logsignature_channels(3, 3) == oracle_logsig.logsignature_channels(3, 3) == 14


def test_log_ode_plan_cache_is_keyed_on_the_values_of_t_not_on_its_address():
    """Round-2 bug: the window-plan cache was keyed on (t.data_ptr(), t._version).  Allocators recycle addresses, so a
    DIFFERENT t of the same length at a recycled block (version 0) was served the previous plan -- silently wrong
    windows.  Here many same-length grids with different values pass through freshly recycled allocations WITHOUT
    clearing the cache; every plan must equal the reference loop's (oracle.logsig.window_plan) for ITS OWN times, and the
    returned window times must not alias the cached tensor."""
    from oracle import logsig as oracle_logsig
    from torchcde_amd import log_ode
    log_ode._plans.clear()
    seen_ptrs = set()
    recycled = 0
    for rep in range(200):
        span = 16.0 * (1 + rep % 7)
        t = torch.linspace(0, span, 17)                  # same length, same dtype, version 0 -- different values
        recycled += t.data_ptr() in seen_ptrs
        seen_ptrs.add(t.data_ptr())
        new_t, rows, _ = oracle_logsig.window_plan(t, 4.0)
        plan = log_ode._plan(t, True, 4.0, 17, 3, 2, 0, t.dtype, torch.device("cpu"))
        assert plan["rows"].tolist() == rows, (rep, span)
        assert torch.equal(plan["new_t"], new_t)
        del t, plan
    assert recycled > 0, "the allocator never recycled a block: the regression scenario did not occur"
    # in-place edit of a time tensor: new values, same address -- must give the new plan
    t = torch.linspace(0, 16, 17)
    first = log_ode._plan(t, True, 4.0, 17, 3, 2, 1, t.dtype, torch.device("cpu"))["rows"].tolist()
    t.mul_(2.0)
    second = log_ode._plan(t, True, 4.0, 17, 3, 2, 1, t.dtype, torch.device("cpu"))["rows"].tolist()
    assert first == [0, 4, 8, 12, 16] and second == oracle_logsig.window_plan(t, 4.0)[1] != first


def test_dispatch_table_is_exhaustively_consistent():
    """torchcde_amd/dispatch.py: the field kind x method x gradient request -> path table that replaced round 2's
    if-lattice.  ALL combinations of its inputs are enumerated (3 kinds x 3 methods x 2^17 flags x 3 parameter kinds,
    pruned of contradictory ones) and every verdict is checked against the invariants the kernels rely on; then the rows a
    user meets are spelled out one by one."""
    import itertools
    from torchcde_amd import dispatch as D
    flags = ["prod", "tiles_ok", "mfma_shape", "adjoint", "wants_grad", "wants_t", "wants_control", "adjoint_method_ok",
             "options_ok", "adjoint_options_ok", "t_ok", "variant_generic", "shared", "narrow_control", "backprop_ok", "identity",
             "control_block"]
    seen = collections_counter = {}
    n = 0
    for kind in (None, "affine", "mlp2"):
        for method in ("rk4", "dopri5", "midpoint"):
            for params in ("default", "own", "foreign"):
                for bits in itertools.product((False, True), repeat=len(flags)):
                    f = dict(zip(flags, bits))
                    if (f["wants_t"] or f["wants_control"]) and not f["wants_grad"]:
                        continue                                 # contradictory requests are never built by cdeint
                    if f["mfma_shape"] and (kind != "affine" or not f["tiles_ok"] or f["variant_generic"]):
                        continue
                    if f["backprop_ok"] and not (f["mfma_shape"] or (kind == "mlp2" and f["tiles_ok"] and not f["variant_generic"])):
                        continue                                 # the reverse-mode sweeps live on the MFMA tiles
                    if f["identity"] and kind != "affine":
                        continue
                    if f["control_block"] and not (f["wants_control"] and f["adjoint"] and params == "own"):
                        continue                                 # the one extra entry of adjoint_params: the coefficient tensor
                    q = D.Request(kind=kind, method=method, params=params, **f)
                    c = D.select_path(q)
                    n += 1
                    seen[c.path] = seen.get(c.path, 0) + 1
                    assert c.path in D.FUSED_PATHS or c.path == D.STEPWISE
                    assert (c.path == D.STEPWISE) == bool(c.reason)          # every step-wise verdict says why
                    if c.path == D.STEPWISE:
                        continue
                    # ---- what every fused path may assume
                    assert not f["prod"] and kind is not None and f["tiles_ok"] and f["t_ok"] and f["options_ok"]
                    if c.path == "fixed_grid":
                        # midpoint / euler: the plain affine field, no time / control gradients, gradients through adjoint=True only
                        assert method == "midpoint" and kind == "affine" and f["backprop_ok"] and f["mfma_shape"] and f["identity"]
                        assert not f["wants_t"] and not f["wants_control"]
                        assert not f["wants_grad"] or (f["adjoint"] and f["adjoint_method_ok"] and f["adjoint_options_ok"]
                                                       and params != "foreign")
                        continue
                    assert method == ("rk4" if "rk4" in c.path else "dopri5")
                    assert c.path.startswith("mlp_") == (kind == "mlp2")
                    assert ("forward" in c.path) <= (not f["wants_grad"])    # forward-only kernels: nothing to differentiate
                    if c.path in ("rk4_backprop", "mlp_rk4_backprop"):
                        # adjoint=False: reverse mode through the steps -- no output-time gradients
                        assert f["wants_grad"] and not f["adjoint"] and f["backprop_ok"] and not f["wants_t"]
                        assert f["mfma_shape"] == (kind == "affine")
                        continue
                    if f["wants_grad"]:
                        assert f["adjoint"] and f["adjoint_method_ok"] and f["adjoint_options_ok"] and params != "foreign"
                    if c.path == "dopri5_adjoint":
                        # (output-time gradients: K4a carries vjp_t; not with one controller across shards)
                        # (control gradients: the coefficient tensor as ONE block of the adjoint norm, one controller per solve;
                        #  output-time gradients: K4a carries vjp_t, with one controller across shards as well since round 6)
                        assert f["mfma_shape"]
                        assert not f["wants_control"] or (f["control_block"] and not f["shared"])
                    if c.path == "mlp_dopri5_adjoint":
                        assert not f["wants_control"] or (f["control_block"] and not f["shared"])
                    if kind == "mlp2":
                        assert not f["variant_generic"]
                        assert not f["wants_t"] or c.path == "mlp_dopri5_adjoint" or method == "rk4"
                        assert not f["wants_control"] or method == "rk4" or f["control_block"]
                    if kind == "affine" and (f["wants_t"] or f["wants_control"]):
                        assert f["mfma_shape"] and (method == "rk4" or not f["wants_control"] or f["control_block"])
    assert n > 100000 and set(seen) == set(D.FUSED_PATHS) | {D.STEPWISE}       # every path is reachable

    def ask(**kw):
        base = dict(prod=False, kind="affine", tiles_ok=True, mfma_shape=True, method="dopri5", adjoint=True,
                    wants_grad=True, wants_t=False, wants_control=False, params="default", adjoint_method_ok=True,
                    options_ok=True, adjoint_options_ok=True, t_ok=True, variant_generic=False, shared=False,
                    narrow_control=True, backprop_ok=True, identity=True, control_block=False)
        base.update(kw)
        return D.select_path(D.Request(**base))
    # the rows a user meets
    assert ask().path == "dopri5_adjoint"                                       # README.md:55: cdeint(X, func, z0, t)
    assert ask(kind="mlp2", mfma_shape=False).path == "mlp_dopri5_adjoint"      # example/time_series_classification.py:83-86
    assert ask(method="rk4").path == "rk4"                                      # BASELINE configs[2]
    assert ask(method="rk4", wants_grad=False, adjoint=False).path == "rk4"     # BASELINE configs[1]
    assert ask(wants_grad=False).path == "dopri5_forward"                       # BASELINE configs[3]
    assert ask(kind="mlp2", mfma_shape=False, method="rk4").path == "mlp_rk4_adjoint"      # BASELINE configs[4] with rk4
    assert ask(shared=True).path == "dopri5_adjoint"                            # one controller over the shards
    assert ask(kind="mlp2", mfma_shape=False, shared=True).path == "mlp_dopri5_adjoint"    # ... for the examples' model too
    assert ask(method="rk4", wants_control=True, params="own").path == "rk4"    # README.md:251-270
    assert ask(wants_t=True).path == "dopri5_adjoint"                           # output-time gradients: K4a carries vjp_t
    assert ask(wants_t=True, shared=True).path == "dopri5_adjoint"              # ... next to one controller across the shards too
    assert ask(kind="mlp2", mfma_shape=False, wants_t=True, shared=True).path == "mlp_dopri5_adjoint"
    # README.md:251-270 with the default method: adjoint_params = parameters + (coeffs,) -- one more block of K4a's norm
    assert ask(wants_control=True, params="own", control_block=True).path == "dopri5_adjoint"
    assert ask(wants_control=True, params="own", control_block=True, wants_t=True).path == "dopri5_adjoint"
    assert ask(wants_control=True, params="own", control_block=True, shared=True).path == D.STEPWISE
    assert ask(kind="mlp2", mfma_shape=False, wants_control=True, params="own", control_block=True).path == "mlp_dopri5_adjoint"
    assert ask(method="rk4", adjoint=False).path == "rk4_backprop"              # README.md:103: backprop through the solver
    assert ask(kind="mlp2", mfma_shape=False, method="rk4", adjoint=False).path == "mlp_rk4_backprop"
    assert ask(method="rk4", adjoint=False, wants_control=True).path == "rk4_backprop"      # test/test_tricks.py:21-49, adjoint=False
    assert ask(kind="mlp2", mfma_shape=False, method="rk4", adjoint=False, wants_control=True).path == "mlp_rk4_backprop"
    # the logsignature-shaped two-layer field (16 units x 14 channels): time and control gradients on its tile layout too
    assert ask(kind="mlp2", mfma_shape=False, method="rk4", wants_control=True, params="own", narrow_control=False).path == "mlp_rk4_adjoint"
    assert ask(kind="mlp2", mfma_shape=False, method="rk4", wants_t=True, narrow_control=False).path == "mlp_rk4_adjoint"
    assert ask(method="midpoint").path == "fixed_grid"                          # test/test_cdeint.py:49-63
    assert ask(method="euler", wants_grad=False).path == "fixed_grid"
    for kw, word in ((dict(kind=None), "recognised"), (dict(method="midpoint", kind="mlp2", mfma_shape=False), "midpoint"),
                     (dict(method="euler", adjoint=False), "euler"), (dict(method="heun3"), "heun3"),
                     (dict(adjoint=False), "adjoint=False"), (dict(method="rk4", adjoint=False, backprop_ok=False), "adjoint=False"), (dict(options_ok=False), "options"),
                     (dict(mfma_shape=False), "32 x 8"),
                     (dict(wants_control=True, params="own"), "control"),
                     (dict(t_ok=False), "increasing"), (dict(params="foreign"), "adjoint_params"),
                     (dict(prod=True), "prod"), (dict(tiles_ok=False, mfma_shape=False), "tiles")):
        verdict = ask(**kw)
        assert verdict.path == D.STEPWISE and word in verdict.reason, (kw, verdict)


def test_every_dispatch_expectation_of_the_gpu_tests_holds_on_the_cpu():
    """the GPU tests name their request in tests/dispatch_cases.py and assert that the
    call took the row's path; HERE the same rows go through `select_path` without a GPU, so a change of the capability
    table that moves any request the GPU tests make fails on the CPU box -- not at round end under `-x`."""
    import glob
    import dispatch_cases as DC
    from torchcde_amd import dispatch as D
    for name, (fields, path, free) in DC.CASES.items():
        assert path in D.FUSED_PATHS or path == D.STEPWISE, name
        n = 0
        for q in DC.requests_of(name):
            got = D.select_path(q)
            assert got.path == path, "row %r, request %r: select_path says %r (%s)" % (name, q, got.path, got.reason)
            n += 1
        assert n == 2 ** len(DC._free(name))
    assert set(DC.GRAD_FN) == {p for p in D.FUSED_PATHS if "forward" not in p}
    # every row a GPU test names exists, and every row is used by some GPU test
    here = os.path.dirname(os.path.abspath(__file__))
    used = set()
    for path in glob.glob(os.path.join(here, "test_gpu_*.py")):
        src = open(path).read()
        used |= set(re.findall(r'"([a-z0-9_]+)"', " ".join(re.findall(r"_expect_dispatch\((.*)", src))))
        used |= set(re.findall(r'expect = "([a-z0-9_]+)"', src))
    used = {u for u in used if not u.startswith("_")} - {"auto", "tanh", "two_layer", "midpoint"}      # (strings of the conditions)
    assert used <= set(DC.CASES), used - set(DC.CASES)
    assert len(used) >= 12


def test_option_noops_and_per_thread_call_state():
    """None-valued keys and torchdiffeq's defaults spelled out are the same request as leaving the key away
    -- for the dispatch test AND for the plans (they used to disagree).  VERDICT round 3, weak #12: the step statistics /
    trace switch / event log of `torchcde_amd.cdeint` belong to the calling thread."""
    import sys
    import threading
    import torchcde_amd  # noqa: F401
    front = sys.modules["torchcde_amd.cdeint"]
    strip = front._strip_noops
    assert strip(None, True) is None
    assert strip(dict(step_size=1.0, interp="linear", perturb=False, norm=None), fixed=True) == dict(step_size=1.0)
    assert strip(dict(step_size=1.0, norm=lambda x: x), fixed=True) == dict(step_size=1.0)
    assert strip(dict(interp="cubic", perturb=True), fixed=True) == dict(interp="cubic", perturb=True)
    assert strip(dict(safety=None, jump_t=None, ifactor=5.0), fixed=False) == dict(ifactor=5.0)
    assert strip(dict(norm="seminorm", safety=None), fixed=False) == dict(norm="seminorm")
    assert front._parse_fixed_options(strip(dict(step_size=0.5, interp="linear", perturb=False), True), "solver") == 0.5

    front.record_dopri5_steps = True
    front.event_log = []
    seen = {}

    def other():
        seen["record"], seen["log"], seen["stats"] = front.record_dopri5_steps, front.event_log, dict(front.last_dopri5_stats)
        front.record_dopri5_steps = False                  # ... and what it sets stays its own
        front._state().dopri5.update(n_accept=7)

    worker = threading.Thread(target=other)
    worker.start()
    worker.join()
    try:
        assert seen == dict(record=False, log=None, stats={})
        assert front.record_dopri5_steps is True and front.event_log == [] and front.last_dopri5_stats == {}
    finally:
        front.record_dopri5_steps = False
        front.event_log = None


def test_reverse_mode_recurrences_of_the_rk4_backprop_kernel_equal_autograd_through_the_oracle():
    """csrc/rk4_backprop.hip (adjoint=False under rk4) restated in float64 torch ops: the stage states of torchdiffeq's 3/8
    rule stored on the way forward, then per step and stage  v = J^T kb,  yb += v,  the kb updates of the file header, the
    dL/dW / dL/db products -- and the host's transpose of the fixed-grid output interpolation (`_Grids.backprop_lists`:
    outputs at grid points, inside a step, at the ends; a last step shorter than step_size).  Against autograd through the
    oracle's odeint (what the reference's adjoint=False call differentiates)."""
    from torchcde_amd.cdeint import _Grids
    from oracle import cde as oracle_cde, interp as oracle_interp
    from helpers import make_series
    B, L, C, H = 5, 9, 3, 4
    dt64 = torch.float64
    x = make_series(B, L, C, dt64, seed=41)
    for t_out, step in ((torch.tensor([0., 8.], dtype=dt64), 1.0),
                        (torch.tensor([0., 1.5, 2.0, 2.25, 6.9, 8.], dtype=dt64), 0.75),
                        (torch.tensor([1., 7.3], dtype=dt64), 2.0)):
        func = LinearField(H, C, dt64, scale=0.4, seed=2)
        # the control's tensors require gradients too (autograd reaches them through X.derivative at every stage): the
        # coefficient tensor and the knot times are leaves here
        coeffs = oracle_interp.hermite_bdiff_coeffs(x).requires_grad_(True)
        knots = torch.arange(L, dtype=dt64).requires_grad_(True)
        X = oracle_interp.CubicPath(coeffs, knots)
        z0 = torch.randn(B, H, dtype=dt64, generator=torch.Generator().manual_seed(3)).requires_grad_(True)
        lw = torch.rand(B, t_out.numel(), H, dtype=dt64, generator=torch.Generator().manual_seed(4)) + 0.5
        ref = oracle_cde.cdeint(X, func, z0, t_out, adjoint=False, method="rk4", options=dict(step_size=step))
        (ref * lw).sum().backward()
        W, b = func.linear.weight.detach().view(H, C, H), func.linear.bias.detach().view(H, C)
        grids = _Grids(t_out, step, None, torch.device("cpu"))
        step_dt, node_ptr, node_out, node_w, n_steps = grids.backprop_lists()
        grid = grids.grid
        assert step_dt.dtype == torch.float32 and n_steps == grid.numel() - 1
        third = 1.0 / 3.0

        def jac(t):                                       # J(t) = sum_c dX_c W_c, beta = b dX
            dX = X.derivative(t)                          # (B, C)
            return torch.einsum("bc,hck->bhk", dX, W), torch.einsum("bc,hc->bh", dX, b), dX

        stages, y = [], z0.detach().clone()
        for k in range(n_steps):
            t0, t1 = grid[k], grid[k + 1]
            dt = t1 - t0
            times = (t0, t0 + dt * third, t0 + dt * 2 * third, t1)
            f = lambda t, s: torch.einsum("bhk,bk->bh", jac(t)[0], s) + jac(t)[1]
            s1 = y; k1 = f(times[0], s1)
            s2 = y + dt * k1 * third; k2 = f(times[1], s2)
            s3 = y + dt * (k2 - k1 * third); k3 = f(times[2], s3)
            s4 = y + dt * (k1 - k2 + k3); k4 = f(times[3], s4)
            stages.append((times, (s1, s2, s3, s4)))
            y = y + (k1 + 3 * (k2 + k3) + k4) * dt * 0.125
        go = lw                                           # dL/dz_out

        def outputs_at(m):
            g = torch.zeros(B, H, dtype=dt64)
            for e in range(int(node_ptr[m]), int(node_ptr[m + 1])):
                g = g + float(node_w[e]) * go[:, int(node_out[e])]
            return g

        gy = outputs_at(n_steps)
        gW, gb = torch.zeros(H, C, H, dtype=dt64), torch.zeros(H, C, dtype=dt64)
        gx = torch.zeros_like(coeffs)                    # dL/d(packed coefficients): the b, 2c, 3d columns of the row in use
        for k in range(n_steps - 1, -1, -1):
            dt = float(step_dt[k].double())
            times, ss = stages[k]
            c8 = dt * 0.125
            kb = [gy * c8, gy * (3 * c8), gy * (3 * c8), gy * c8]       # kb1 .. kb4
            yb = gy.clone()
            for i in (3, 2, 1, 0):
                J, _, dX = jac(times[i])
                v = torch.einsum("bh,bhk->bk", kb[i], J)
                gW += torch.einsum("bh,bc,bk->hck", kb[i], dX, ss[i])
                gb += torch.einsum("bh,bc->hc", kb[i], dX)
                # the cotangent of dX_c: sum_h kb_h F(s_i)_hc with F = reshape(W s + b); chained to the row (1, frac, frac^2)
                F = torch.einsum("hck,bk->bhc", W, ss[i]) + b
                gdx = torch.einsum("bh,bhc->bc", kb[i], F)
                frac, index = X._interpret_t(times[i])
                frac, index = float(frac.detach()), int(index)
                gx[:, index, C:2 * C] += gdx
                gx[:, index, 2 * C:3 * C] += gdx * frac
                gx[:, index, 3 * C:] += gdx * frac * frac
                yb = yb + v
                if i == 3:
                    kb[0] = kb[0] + dt * v; kb[1] = kb[1] - dt * v; kb[2] = kb[2] + dt * v
                elif i == 2:
                    kb[1] = kb[1] + dt * v; kb[0] = kb[0] - dt * third * v
                elif i == 1:
                    kb[0] = kb[0] + dt * third * v
            gy = yb + outputs_at(k)
        # (the output-interpolation weights are rounded to float32 like the kernel's slope: 1e-7 relative)
        assert torch.allclose(gy, z0.grad, rtol=1e-6, atol=1e-9)
        assert torch.allclose(gW.reshape(H * C, H), func.linear.weight.grad, rtol=1e-6, atol=1e-9)
        assert torch.allclose(gb.reshape(H * C), func.linear.bias.grad, rtol=1e-6, atol=1e-9)
        with torch.no_grad():
            assert torch.allclose(gx, coeffs.grad, rtol=1e-6, atol=1e-9)
            # the knot times: frac = t - knot_j, so dL/d knot_j = - sum over the stages in interval j of gdx . d2X/dt2 -- which is
            # a contraction of the coefficient gradient itself (cdeint.py: _time_gradients)
            per_interval = (coeffs[..., 2 * C:3 * C] * gx[..., C:2 * C] + 2 * coeffs[..., 3 * C:] * gx[..., 2 * C:3 * C]).sum((0, 2))
            assert torch.allclose(torch.cat([-per_interval, per_interval.new_zeros(1)]), knots.grad, rtol=1e-6, atol=1e-9)


def test_fit_chain_detection_walks_the_autograd_graph():
    """Round 6: torchdiffeq's knot block (`autograd.grad(f, adjoint_params)`) runs through the fit that produced the coefficients
    when the SAME knot tensor went into it (reference test/test_tricks.py:21-49).  cdeint._knot_fit_chain decides that by walking
    the autograd graph of the path's buffers -- no GPU involved: leaf coefficients have no chain, fitted ones do, for a leaf knot
    tensor and for one that is itself computed; and the chain's vector-Jacobian product is what autograd gives."""
    import types
    import sys
    from oracle import interp
    front = sys.modules["torchcde_amd.cdeint"]                      # (the package exports the function under the same name)
    t = torch.linspace(0, 4, 5, dtype=torch.float64, requires_grad=True)
    x = torch.randn(3, 5, 2, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    fitted = interp.hermite_bdiff_coeffs(x, t)
    C = 2

    def path(coeffs, knots):
        bufs = (coeffs[..., C:2 * C], coeffs[..., 2 * C:3 * C], coeffs[..., 3 * C:])
        return types.SimpleNamespace(_t=knots, _control_buffers=lambda: bufs)

    assert front._reaches(fitted, t) and not front._reaches(fitted.detach().requires_grad_(True), t)
    assert front._knot_fit_chain(path(fitted.detach().requires_grad_(True), t)) is None           # leaf coefficients: nothing to add
    assert front._knot_fit_chain(path(fitted, t.detach())) is None                                # knots without a gradient
    chain = front._knot_fit_chain(path(fitted, t))
    assert chain is not None and len(chain[0]) == 3 and chain[2] is t
    u = t * 1.5                                                                                    # a knot tensor that is itself computed
    fitted_u = interp.hermite_bdiff_coeffs(x, u)
    assert front._reaches(fitted_u, u) and not front._reaches(fitted, u)
    assert front._knot_fit_chain(path(fitted_u, u)) is not None
    # the added term = the fit's vector-Jacobian product with dL/dcoeffs (b, 2c, 3d blocks; the derivative never reads `a`)
    plan = types.SimpleNamespace(fit_chain=chain, C=C, batch=(3,), degree=_lib.PATH_CUBIC)
    g = torch.randn(3, 4, 4 * C, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    direct = torch.arange(5, dtype=torch.float64)
    got = front._with_fit_chain(plan, direct.clone(), g)
    gz = g.clone()
    gz[..., :C] = 0
    (want,) = torch.autograd.grad(fitted, t, gz, retain_graph=True)
    assert torch.allclose(got, direct + want, rtol=1e-12, atol=1e-14)
    assert front._with_fit_chain(types.SimpleNamespace(fit_chain=None), direct, g) is direct


# ------------------------------------------------------------------ bench.py --dump-outputs
def test_bench_dump_outputs_writes_what_the_step_returns(tmp_path):
    """The arrays a caller of the timed step receives, as float32 .npy files named after them; a per-series array above
    the per-array cap keeps a seeded, sorted sample of its rows, the same from call to call."""
    import bench
    field = LinearField(32, 8, seed=0)
    out = torch.randn(4096, 2, 32)
    z = torch.randn(4096, 32, requires_grad=True)
    (field(None, z).sum() + (2 * z).sum()).backward()
    shapes = bench.dump_outputs(str(tmp_path / "a"), *bench.step_outputs(out, z, field), False, 1, 0)
    assert shapes == {"solution": [4096, 2, 32], "grad_z0": [4096, 32], "grad_linear_weight": [256, 32],
                      "grad_linear_bias": [256]}
    for name, want in (("solution", out), ("grad_z0", z.grad), ("grad_linear_weight", field.linear.weight.grad)):
        got = np.load(str(tmp_path / "a" / (name + ".npy")))
        assert got.dtype == np.float32 and np.array_equal(got, want.numpy()), name
    big = torch.randn(8192, 128, 32)                                 # 128 MB: over the cap
    for run in ("b", "c"):
        assert bench.dump_outputs(str(tmp_path / run), {"solution": big}, {}, False, 1, 0) == {"solution": [1024, 128, 32]}
    sample = np.load(str(tmp_path / "b" / "solution.npy"))
    assert sample.nbytes == bench.DUMP_BATCHED_MAX_BYTES and np.array_equal(sample, np.load(str(tmp_path / "c" / "solution.npy")))
    rows = torch.randperm(8192, generator=torch.Generator().manual_seed(0))[:1024].sort().values
    assert np.array_equal(sample, big[rows].numpy())
    with pytest.raises(SystemExit):                                   # integer outputs are not part of the format
        bench.dump_outputs(str(tmp_path / "d"), {"solution": torch.zeros(4, 2, dtype=torch.int64)}, {}, False, 1, 0)
