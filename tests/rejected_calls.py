"""Calls of the fixed-grid entry points that are rejected before anything touches the device, with the code each one returns.

Every row fails an argument check (shape, dtype, unsupported combination, empty batch, NULL pointer, workspace one byte too
small) that comes before the first HIP call, so the table runs without a GPU -- and must stay that way: the pointers are
dummies.  The codes pin the ORDER of the checks of each entry point (csrc/api.hip)."""

# entry point -> its C parameters in order; "name": a pointer (a non-null dummy, never dereferenced), "name=v": an integer
CALLS = {
    "cde_rk4_forward_linear": "coeffs knots n_intervals=4 degree=3 W bias act=0 z0 grid n_grid=5 t_out n_out=2 z_out B=64 C=8 H=32 "
                              "dtype=0 time_dtype=0 variant=0 stage_index stage_frac stream=0",
    "cde_rk4_forward_linear_stages": "coeffs knots n_intervals=4 degree=3 W bias act=0 z0 grid n_grid=5 t_out n_out=2 z_out stages "
                                     "B=64 C=8 H=32 dtype=0 time_dtype=0 stage_index stage_frac stream=0",
    "cde_rk4_forward_mlp": "coeffs knots n_intervals=4 degree=3 W1 bias1 width=32 W2 bias2 act=1 z0 grid n_grid=5 t_out n_out=2 "
                           "z_out B=64 C=8 H=32 dtype=0 time_dtype=0 stage_index stage_frac stream=0",
    "cde_rk4_forward_mlp_stages": "coeffs knots n_intervals=4 degree=3 W1 bias1 width=32 W2 bias2 act=1 z0 grid n_grid=5 t_out "
                                  "n_out=2 z_out stages B=64 C=8 H=32 dtype=0 time_dtype=0 stage_index stage_frac stream=0",
    "cde_fixed_forward_linear": "method=1 coeffs knots n_intervals=4 degree=3 W bias z0 grid n_grid=5 t_out n_out=2 z_out B=64 C=8 "
                                "H=32 dtype=0 time_dtype=0 stage_index stage_frac stream=0",
    "cde_fixed_adjoint_linear": "method=1 coeffs knots n_intervals=4 degree=3 W bias z_saved grad_out sgrid n_sgrid=5 seg_off "
                                "n_out=2 grad_z0 grad_W grad_b B=64 C=8 H=32 dtype=0 time_dtype=0 workspace "
                                "workspace_bytes=1073741824 stream=0",
    "cde_rk4_adjoint_linear": "coeffs knots n_intervals=4 degree=3 W bias act=0 z_saved grad_out sgrid n_sgrid=5 seg_off "
                              "seg_off_host n_out=2 grad_z0 grad_W grad_b B=64 C=8 H=32 dtype=0 time_dtype=0 variant=2 workspace "
                              "workspace_bytes=1073741824 stream=0",
    "cde_rk4_adjoint_linear_dcontrol": "coeffs knots n_intervals=4 degree=3 W bias act=0 z_saved grad_out sgrid n_sgrid=5 seg_off "
                                       "n_out=2 grad_z0 grad_W grad_b grad_coeffs B=64 C=8 H=32 dtype=0 time_dtype=0 workspace "
                                       "workspace_bytes=1073741824 stream=0",
    "cde_rk4_backprop_linear": "coeffs knots n_intervals=4 degree=3 W bias act=0 stages grad_out n_out=2 step_dt n_steps=4 node_ptr "
                               "node_out node_weight grad_z0 grad_W grad_b B=64 C=8 H=32 dtype=0 stage_index stage_frac workspace "
                               "workspace_bytes=1073741824 stream=0",
    "cde_rk4_backprop_linear_dcontrol": "coeffs knots n_intervals=4 degree=3 W bias act=0 stages grad_out n_out=2 step_dt n_steps=4 "
                                        "node_ptr node_out node_weight grad_z0 grad_W grad_b grad_coeffs B=64 C=8 H=32 dtype=0 "
                                        "stage_index stage_frac workspace workspace_bytes=1073741824 stream=0",
    "cde_rk4_adjoint_mlp_prepare": "knots n_intervals=4 sgrid n_sgrid=5 W1 bias1 width=32 W2 bias2 C=8 H=32 dtype=0 time_dtype=0 "
                                   "workspace workspace_bytes=1073741824 stream=0",
    "cde_rk4_backprop_mlp_prepare": "knots n_intervals=4 grid n_grid=5 W1 bias1 width=32 W2 bias2 C=8 H=32 dtype=0 time_dtype=0 "
                                    "workspace workspace_bytes=1073741824 stream=0",
    "cde_rk4_adjoint_mlp_sweep": "coeffs knots n_intervals=4 degree=3 act=1 y_state a_state sgrid n_sgrid=5 k_begin=0 k_end=4 U G2 "
                                 "G1 Z grad_coeffs B=64 C=8 H=32 dtype=0 time_dtype=0 workspace workspace_bytes=1073741824 stream=0",
    "cde_rk4_backprop_mlp_sweep": "coeffs knots n_intervals=4 degree=3 act=1 stages g_state grid n_grid=5 k_begin=0 k_end=4 U G2 G1 "
                                  "Z B=64 C=8 H=32 dtype=0 time_dtype=0 workspace workspace_bytes=1073741824 stream=0",
    "cde_rk4_backprop_mlp_sweep_dcontrol": "coeffs knots n_intervals=4 degree=3 act=1 stages g_state grid n_grid=5 k_begin=0 "
                                           "k_end=4 U G2 G1 Z grad_coeffs B=64 C=8 H=32 dtype=0 time_dtype=0 workspace "
                                           "workspace_bytes=1073741824 stream=0",
}
DUMMY = 0x1000

# entry point -> {code: overrides of the valid call above that must return it}; "a=1 b=2" changes both at once
REJECTED = {
    "cde_rk4_forward_linear": {
        -3: ["C=0", "H=0", "n_intervals=0", "B=-1", "n_out=0", "n_grid=0"],
        -2: ["dtype=7", "time_dtype=7"],
        0: ["B=0"],
        -4: ["act=5"],
        -1: ["coeffs=0", "knots=0", "W=0", "bias=0", "z0=0", "grid=0", "t_out=0", "z_out=0", "stage_index=0",
             "stage_frac=0"],
    },
    "cde_rk4_forward_linear_stages": {
        -3: ["C=0", "H=0", "n_intervals=0", "B=-1", "n_out=0", "n_grid=0"],
        -2: ["dtype=7", "time_dtype=7"],
        0: ["B=0"],
        -4: ["dtype=1", "act=5", "H=33", "C=17 H=16", "H=64 C=8", "C=9"],
        -1: ["coeffs=0", "knots=0", "W=0", "bias=0", "z0=0", "grid=0", "t_out=0", "z_out=0", "stages=0",
             "stage_index=0", "stage_frac=0"],
    },
    "cde_rk4_forward_mlp": {
        -3: ["C=0", "H=0", "n_intervals=0", "B=-1", "width=0", "n_out=0", "n_grid=0"],
        -2: ["dtype=7", "time_dtype=7"],
        0: ["B=0"],
        -4: ["dtype=1"],
        -1: ["coeffs=0", "knots=0", "W1=0", "bias1=0", "W2=0", "bias2=0", "z0=0", "grid=0", "t_out=0", "z_out=0",
             "stage_index=0", "stage_frac=0"],
    },
    "cde_rk4_forward_mlp_stages": {
        -3: ["C=0", "H=0", "n_intervals=0", "B=-1", "width=0", "n_out=0", "n_grid=0"],
        -2: ["dtype=7", "time_dtype=7"],
        0: ["B=0"],
        -4: ["dtype=1"],
        -1: ["coeffs=0", "knots=0", "W1=0", "bias1=0", "W2=0", "bias2=0", "z0=0", "grid=0", "t_out=0", "z_out=0",
             "stages=0", "stage_index=0", "stage_frac=0"],
    },
    "cde_fixed_forward_linear": {
        -3: ["C=0", "H=0", "n_intervals=0", "B=-1", "n_out=0", "n_grid=0"],
        -2: ["dtype=7", "time_dtype=7"],
        0: ["B=0"],
        -4: ["method=0", "method=7", "dtype=1", "H=33", "C=17 H=16", "H=64 C=8", "C=9"],
        -1: ["coeffs=0", "knots=0", "W=0", "bias=0", "z0=0", "grid=0", "t_out=0", "z_out=0", "stage_index=0",
             "stage_frac=0"],
    },
    "cde_fixed_adjoint_linear": {
        -3: ["C=0", "H=0", "n_intervals=0", "B=0", "B=-1", "n_out=0"],
        -2: ["dtype=7", "time_dtype=7"],
        -4: ["method=0", "method=7", "dtype=1", "H=33", "C=17 H=16", "H=64 C=8", "C=9"],
        -1: ["coeffs=0", "knots=0", "W=0", "bias=0", "z_saved=0", "grad_out=0", "sgrid=0", "seg_off=0",
             "grad_z0=0", "grad_W=0", "grad_b=0", "workspace=0"],
        -5: ["workspace_bytes=68095"],
    },
    "cde_rk4_adjoint_linear": {
        -3: ["C=0", "H=0", "n_intervals=0", "B=0", "B=-1", "n_out=0"],
        -2: ["dtype=7", "time_dtype=7"],
        -4: ["dtype=1", "act=5", "H=33", "C=17 H=16", "H=64 C=8", "C=9", "variant=4 act=1", "variant=9",
             "variant=3 H=64"],
        -1: ["coeffs=0", "knots=0", "W=0", "bias=0", "z_saved=0", "grad_out=0", "sgrid=0", "seg_off=0",
             "grad_z0=0", "grad_W=0", "grad_b=0", "workspace=0"],
        -5: ["workspace_bytes=68095"],
    },
    "cde_rk4_adjoint_linear_dcontrol": {
        -3: ["C=0", "H=0", "n_intervals=0", "B=0", "B=-1", "n_out=0"],
        -2: ["dtype=7", "time_dtype=7"],
        -4: ["dtype=1", "act=5", "H=33", "C=17 H=16", "H=64 C=8", "C=9"],
        -1: ["coeffs=0", "knots=0", "W=0", "bias=0", "z_saved=0", "grad_out=0", "sgrid=0", "seg_off=0",
             "grad_z0=0", "grad_W=0", "grad_b=0", "grad_coeffs=0", "workspace=0"],
        -5: ["workspace_bytes=68095"],
    },
    "cde_rk4_backprop_linear": {
        -3: ["C=0", "H=0", "n_intervals=0", "B=0", "B=-1", "n_out=0", "n_steps=-1"],
        -2: ["dtype=7"],
        -4: ["dtype=1", "act=5", "H=33", "C=17 H=16", "H=64 C=8", "C=9"],
        -1: ["coeffs=0", "knots=0", "W=0", "bias=0", "stages=0", "grad_out=0", "step_dt=0", "node_ptr=0",
             "node_out=0", "node_weight=0", "grad_z0=0", "grad_W=0", "grad_b=0", "stage_index=0", "stage_frac=0",
             "workspace=0"],
        -5: ["workspace_bytes=67583"],
    },
    "cde_rk4_backprop_linear_dcontrol": {
        -3: ["C=0", "H=0", "n_intervals=0", "B=0", "B=-1", "n_out=0", "n_steps=-1"],
        -2: ["dtype=7"],
        -4: ["dtype=1", "act=5", "H=33", "C=17 H=16", "H=64 C=8", "C=9"],
        -1: ["coeffs=0", "knots=0", "W=0", "bias=0", "stages=0", "grad_out=0", "step_dt=0", "node_ptr=0",
             "node_out=0", "node_weight=0", "grad_z0=0", "grad_W=0", "grad_b=0", "grad_coeffs=0",
             "stage_index=0", "stage_frac=0", "workspace=0"],
        -5: ["workspace_bytes=67583"],
    },
    "cde_rk4_adjoint_mlp_prepare": {
        -3: ["C=0", "H=0", "n_intervals=0", "width=0"],
        -2: ["dtype=7", "time_dtype=7"],
        -4: ["dtype=1", "H=33", "C=17 H=16", "H=64 C=8"],
        -1: ["knots=0", "sgrid=0", "W1=0", "bias1=0", "W2=0", "bias2=0", "workspace=0"],
        -5: ["workspace_bytes=433151"],
    },
    "cde_rk4_backprop_mlp_prepare": {
        -3: ["C=0", "H=0", "n_intervals=0", "width=0"],
        -2: ["dtype=7", "time_dtype=7"],
        -4: ["dtype=1", "H=33", "C=17 H=16", "H=64 C=8"],
        -1: ["knots=0", "grid=0", "W1=0", "bias1=0", "W2=0", "bias2=0", "workspace=0"],
        -5: ["workspace_bytes=433151"],
    },
    "cde_rk4_adjoint_mlp_sweep": {
        -3: ["C=0", "H=0", "n_intervals=0", "B=0", "B=-1", "k_end=5", "k_begin=-1", "k_begin=3 k_end=2"],
        -2: ["dtype=7", "time_dtype=7"],
        -4: ["dtype=1", "H=33", "C=17 H=16", "H=64 C=8"],
        -1: ["coeffs=0", "knots=0", "y_state=0", "a_state=0", "sgrid=0", "U=0", "G2=0", "G1=0", "Z=0",
             "workspace=0"],
        -5: ["workspace_bytes=433151"],
    },
    "cde_rk4_backprop_mlp_sweep": {
        -3: ["C=0", "H=0", "n_intervals=0", "B=0", "B=-1", "k_end=5", "k_begin=-1", "k_begin=3 k_end=2"],
        -2: ["dtype=7", "time_dtype=7"],
        -4: ["dtype=1", "H=33", "C=17 H=16", "H=64 C=8"],
        -1: ["coeffs=0", "knots=0", "stages=0", "g_state=0", "grid=0", "U=0", "G2=0", "G1=0", "Z=0",
             "workspace=0"],
        -5: ["workspace_bytes=433151"],
    },
    "cde_rk4_backprop_mlp_sweep_dcontrol": {
        -3: ["C=0", "H=0", "n_intervals=0", "B=0", "B=-1", "k_end=5", "k_begin=-1", "k_begin=3 k_end=2"],
        -2: ["dtype=7", "time_dtype=7"],
        -4: ["dtype=1", "H=33", "C=17 H=16", "H=64 C=8"],
        -1: ["coeffs=0", "knots=0", "stages=0", "g_state=0", "grid=0", "U=0", "G2=0", "G1=0", "Z=0",
             "grad_coeffs=0", "workspace=0"],
        -5: ["workspace_bytes=433151"],
    },
}


def build_args(spec, overrides=""):
    over = dict(tok.split("=") for tok in overrides.split())
    args = []
    for tok in spec.split():
        name, _, value = tok.partition("=")
        args.append(int(over.get(name, value or DUMMY)))
    assert not set(over) - {t.partition("=")[0] for t in spec.split()}, overrides
    return args
