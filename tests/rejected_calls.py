"""Calls of the fixed-grid, the adaptive and the interpolation / log-signature entry points that are rejected before anything
touches the device, with the code each one returns.

Every row fails an argument check (shape, dtype, unsupported combination, empty batch, NULL pointer, workspace one byte too
small) that comes before the first HIP call, so the table runs without a GPU -- and must stay that way: the pointers are
dummies.  The codes pin the ORDER of the checks of each entry point (csrc/api.hip, csrc/dopri5*.hip, csrc/interp_kernels.hip,
csrc/logsig_kernels.hip); a layout table of the adaptive workspaces follows them."""

# entry point -> its C parameters in order; "name": a pointer (a non-null dummy, never dereferenced), "name=v": an integer
# (decimal or 0x..) or, for the doubles of the adaptive protocol, a float ("rtol=1e-4", "s0=-1.0")
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
    "cde_dopri5_advance": "coeffs knots n_intervals=4 degree=3 W bias act=0 z0 t_out n_out=2 jump_t n_jump=0 rtol=1e-4 "
                          "atol=1e-6 safety=0.9 ifactor=10.0 dfactor=0.2 z_out B=64 C=8 H=32 dtype=0 variant=0 workspace "
                          "workspace_bytes=1073741824 first_launch=0 n_launches=1 stream=0",
    "cde_dopri5_advance_sharded": "coeffs knots n_intervals=4 degree=3 W bias act=0 z0 t_out n_out=2 jump_t n_jump=0 rtol=1e-4 "
                                  "atol=1e-6 safety=0.9 ifactor=10.0 dfactor=0.2 z_out B=64 C=8 H=32 dtype=0 variant=0 "
                                  "workspace workspace_bytes=1073741824 first_launch=0 reduced_sums B_global=128 stream=0",
    "cde_dopri5_advance_mlp": "coeffs knots n_intervals=4 degree=3 W1 bias1 width=32 W2 bias2 act=1 z0 t_out n_out=2 jump_t "
                              "n_jump=0 rtol=1e-4 atol=1e-6 safety=0.9 ifactor=10.0 dfactor=0.2 z_out B=64 C=8 H=32 dtype=0 "
                              "workspace workspace_bytes=1073741824 first_launch=0 n_launches=1 stream=0",
    "cde_dopri5_advance_mlp_sharded": "coeffs knots n_intervals=4 degree=3 W1 bias1 width=32 W2 bias2 act=1 z0 t_out n_out=2 "
                                      "jump_t n_jump=0 rtol=1e-4 atol=1e-6 safety=0.9 ifactor=10.0 dfactor=0.2 z_out B=64 C=8 "
                                      "H=32 dtype=0 workspace workspace_bytes=1073741824 first_launch=0 reduced_sums "
                                      "B_global=128 stream=0",
    "cde_dopri5_pending_sums": "workspace workspace_bytes=1073741824 B=64 C=8 H=32 dtype=0 variant=0 act=0 total_launches=1 "
                               "sums stream=0",
    "cde_dopri5_pending_sums_mlp": "workspace workspace_bytes=1073741824 B=64 C=8 H=32 dtype=0 total_launches=1 sums stream=0",
    "cde_dopri5_adjoint_advance": "coeffs knots n_intervals=4 degree=3 W bias act=0 y_init a_init s0=-1.0 s1=0.0 jump_s "
                                  "n_jump=0 rtol=1e-4 atol=1e-6 safety=0.9 ifactor=10.0 dfactor=0.2 norm_kind=0 a_out B=64 C=8 "
                                  "H=32 dtype=0 first_interval=1 workspace workspace_bytes=1073741824 first_launch=0 "
                                  "n_launches=1 reduced_sums=0 B_global=0 stream=0",
    "cde_dopri5_adjoint_advance_dcontrol": "coeffs knots n_intervals=4 degree=3 W bias act=0 y_init a_init s0=-1.0 s1=0.0 "
                                           "jump_s n_jump=0 rtol=1e-4 atol=1e-6 safety=0.9 ifactor=10.0 dfactor=0.2 "
                                           "norm_kind=0 a_out B=64 C=8 H=32 dtype=0 first_interval=1 workspace "
                                           "workspace_bytes=1073741824 first_launch=0 n_launches=1 grad_coeffs "
                                           "control_numel=8192 grad_knots stream=0",
    "cde_dopri5_adjoint_pending_sums": "workspace workspace_bytes=1073741824 B=64 C=8 H=32 total_launches=1 sums stream=0",
    "cde_dopri5_adjoint_state_sums": "workspace workspace_bytes=1073741824 B=64 C=8 H=32 total_launches=1 sums stream=0",
    "cde_dopri5_adjoint_apply_state_sums": "workspace workspace_bytes=1073741824 B=64 C=8 H=32 total_launches=1 reduced "
                                           "stream=0",
    "cde_dopri5_adjoint_apply_reduced": "workspace workspace_bytes=1073741824 B=64 C=8 H=32 rtol=1e-4 atol=1e-6 "
                                        "total_launches=1 reduced stream=0",
    "cde_dopri5_adjoint_finish": "workspace workspace_bytes=1073741824 grad_W grad_b B=64 C=8 H=32 sharded=0 stream=0",
    "cde_dopri5_adjoint_mlp_advance": "coeffs knots n_intervals=4 degree=3 W1 bias1 width=32 W2 bias2 act=1 y_init a_init "
                                      "s0=-1.0 s1=0.0 jump_s n_jump=0 rtol=1e-4 atol=1e-6 safety=0.9 ifactor=10.0 dfactor=0.2 "
                                      "norm_kind=0 a_out B=64 C=8 H=32 dtype=0 first_interval=1 workspace "
                                      "workspace_bytes=1073741824 first_launch=0 n_launches=1 stream=0",
    "cde_dopri5_adjoint_mlp_advance_dcontrol": "coeffs knots n_intervals=4 degree=3 W1 bias1 width=32 W2 bias2 act=1 y_init "
                                               "a_init s0=-1.0 s1=0.0 jump_s n_jump=0 rtol=1e-4 atol=1e-6 safety=0.9 "
                                               "ifactor=10.0 dfactor=0.2 norm_kind=0 a_out B=64 C=8 H=32 dtype=0 "
                                               "first_interval=1 workspace workspace_bytes=1073741824 first_launch=0 "
                                               "n_launches=1 grad_coeffs control_numel=8192 grad_knots stream=0",
    "cde_dopri5_adjoint_mlp_advance_sharded": "coeffs knots n_intervals=4 degree=3 W1 bias1 width=32 W2 bias2 act=1 y_init "
                                              "a_init s0=-1.0 s1=0.0 jump_s n_jump=0 rtol=1e-4 atol=1e-6 safety=0.9 "
                                              "ifactor=10.0 dfactor=0.2 norm_kind=0 a_out B=64 C=8 H=32 dtype=0 "
                                              "first_interval=1 workspace workspace_bytes=1073741824 first_launch=0 "
                                              "reduced_sums B_global=128 stream=0",
    "cde_dopri5_adjoint_mlp_pending_sums": "workspace workspace_bytes=1073741824 B=64 C=8 H=32 total_launches=1 sums stream=0",
    "cde_dopri5_adjoint_mlp_state_sums": "workspace workspace_bytes=1073741824 B=64 C=8 H=32 total_launches=1 sums stream=0",
    "cde_dopri5_adjoint_mlp_apply_state_sums": "workspace workspace_bytes=1073741824 B=64 C=8 H=32 total_launches=1 reduced "
                                               "stream=0",
    "cde_dopri5_adjoint_mlp_apply_reduced": "workspace workspace_bytes=1073741824 B=64 C=8 H=32 rtol=1e-4 atol=1e-6 "
                                            "total_launches=1 reduced stream=0",
    # interpolation, fills and log-signature windows (csrc/interp_kernels.hip, csrc/logsig_kernels.hip)
    "cde_hermite_bdiff_coeffs": "x t coeffs B=2 L=5 C=3 dtype=0 stream=0",
    "cde_hermite_bdiff_coeffs_checked": "x t coeffs B=2 L=5 C=3 dtype=0 nan_flag stream=0",
    "cde_hermite_bdiff_coeffs_nonblocking": "x t coeffs scratch B=2 L=5 C=3 dtype=0 nan_flag generation=1 stream=0",
    "cde_hermite_bdiff_coeffs_backward": "grad_coeffs t grad_x B=2 L=5 C=3 dtype=0 stream=0",
    "cde_hermite_bdiff_coeffs_backward_dt": "grad_coeffs x t grad_h B=2 L=5 C=3 dtype=0 stream=0",
    "cde_linear_fill_missing": "x t out B=2 L=5 C=3 dtype=0 stream=0",
    "cde_linear_fill_missing_backward": "grad_out x t grad_x B=2 L=5 C=3 dtype=0 stream=0",
    "cde_forward_fill": "x out B=2 L=5 C=3 dtype=0 stream=0",
    "cde_forward_fill_backward": "grad_out x grad_x B=2 L=5 C=3 dtype=0 stream=0",
    "cde_rectilinear_prepare": "x out B=2 L=5 C=3 time_index=0 dtype=0 stream=0",
    "cde_rectilinear_prepare_backward": "grad_out x grad_x B=2 L=5 C=3 time_index=0 dtype=0 stream=0",
    "cde_natural_cubic_coeffs": "x t coeffs B=2 L=5 C=3 version=0 has_missing=0 dtype=0 stream=0",
    "cde_natural_cubic_coeffs_backward_workspace_bytes": "L=5 dtype=0",
    "cde_natural_cubic_coeffs_backward": "grad_coeffs t grad_x workspace workspace_bytes=40 B=2 L=5 C=3 dtype=0 x kd_scratch "
                                         "grad_t_rows stream=0",
    "cde_natural_cubic_coeffs_backward_missing": "grad_coeffs x t grad_x workspace B=2 L=5 C=3 version=0 dtype=0 stream=0",
    "cde_logsig_windows": "x rows scale words out B=2 L=5 C=3 depth=2 n_windows=2 n_words=6 dtype=0 stream=0",
    "cde_logsig_windows_backward": "grad_out x rows scale words grad_x workspace B=2 L=5 C=3 depth=2 n_windows=2 n_words=6 "
                                   "dtype=0 stream=0",
    "cde_interpret_t": "knots n_intervals=4 tq nq=3 index_out frac_out dtype=0 stream=0",
    "cde_path_eval": "coeffs knots tq nq=3 out B=2 n_intervals=4 C=3 degree=3 what=0 dtype=0 stream=0",
    "cde_path_eval_backward": "grad_out knots tq nq=3 grad_coeffs B=2 n_intervals=4 C=3 degree=3 what=0 dtype=0 stream=0",
    "cde_contract": "F dX out B=2 H=4 C=3 dtype=0 stream=0",
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
    "cde_dopri5_advance": {
        -3: ["B=0", "B=-1", "C=0", "C=-1", "H=0", "H=-1", "n_intervals=0", "n_intervals=-1", "n_out=0", "n_out=-1",
             "n_launches=-1", "n_jump=-1", "H=257", "variant=9 H=300"],
        # (the generic form's dtype check is its last: past the first launch nothing is queued before it)
        -2: ["dtype=7 first_launch=1", "dtype=7 first_launch=1 variant=1"],
        -4: ["act=5", "act=2", "act=0x21", "act=0x11", "act=0x101", "act=16", "degree=2", "variant=2 H=33", "variant=2 dtype=1",
             "variant=2 H=64", "variant=2 C=16"],
        -1: ["coeffs=0", "knots=0", "W=0", "bias=0", "z0=0", "t_out=0", "z_out=0", "workspace=0", "n_jump=1 jump_t=0"],
        -5: ["workspace_bytes=345855", "H=64 workspace_bytes=427775", "variant=2 H=33 workspace_bytes=16"],
    },
    "cde_dopri5_advance_sharded": {
        -3: ["B=0", "B=-1", "C=0", "C=-1", "H=0", "H=-1", "n_intervals=0", "n_intervals=-1", "n_out=0", "n_out=-1", "n_jump=-1",
             "B_global=0", "B_global=-1", "H=257", "variant=9 H=300", "B_global=63"],
        -2: ["dtype=7 first_launch=1", "dtype=7 first_launch=1 variant=1"],
        -4: ["act=5", "act=2", "act=0x21", "act=0x11", "act=0x101", "act=16", "degree=2", "variant=2 H=33", "variant=2 dtype=1",
             "variant=2 H=64", "variant=2 C=16"],
        -1: ["coeffs=0", "knots=0", "W=0", "bias=0", "z0=0", "t_out=0", "z_out=0", "workspace=0", "reduced_sums=0",
             "n_jump=1 jump_t=0", "B_global=64 reduced_sums=0", "first_launch=1 reduced_sums=0"],
        -5: ["workspace_bytes=345855"],
    },
    "cde_dopri5_advance_mlp": {
        -3: ["B=0", "B=-1", "C=0", "C=-1", "H=0", "H=-1", "n_intervals=0", "n_intervals=-1", "n_out=0", "n_out=-1", "width=0",
             "width=-1", "n_launches=-1", "n_jump=-1", "H=257", "bias1=0 width=0"],
        -4: ["dtype=7", "dtype=1", "act=5", "act=2", "act=0x21", "act=0x101", "degree=2", "H=33", "C=17", "C=17 H=16", "H=64",
             "H=64 C=16"],
        -1: ["coeffs=0", "knots=0", "W1=0", "bias1=0", "W2=0", "bias2=0", "z0=0", "t_out=0", "z_out=0", "workspace=0",
             "n_jump=1 jump_t=0"],
        -5: ["workspace_bytes=345855"],
    },
    "cde_dopri5_advance_mlp_sharded": {
        -3: ["B=0", "B=-1", "C=0", "C=-1", "H=0", "H=-1", "n_intervals=0", "n_intervals=-1", "n_out=0", "n_out=-1", "width=0",
             "width=-1", "n_jump=-1", "B_global=0", "B_global=-1", "H=257", "bias1=0 width=0", "B_global=63"],
        -4: ["dtype=7", "dtype=1", "act=5", "act=2", "act=0x21", "act=0x101", "degree=2", "H=33", "C=17", "C=17 H=16", "H=64",
             "H=64 C=16", "C=16 H=32 width=32 W2=4100"],
        -1: ["coeffs=0", "knots=0", "W1=0", "bias1=0", "W2=0", "bias2=0", "z0=0", "t_out=0", "z_out=0", "workspace=0",
             "reduced_sums=0", "n_jump=1 jump_t=0", "B_global=64 reduced_sums=0", "first_launch=1 reduced_sums=0"],
        -5: ["workspace_bytes=345855"],
    },
    "cde_dopri5_pending_sums": {
        # (H=0 under every form the call can name: the generic form's grid divides by H, so the shape check comes first)
        -3: ["B=0", "B=-1", "C=0", "C=-1", "H=0", "H=-1", "H=0 dtype=1", "H=0 variant=1", "H=0 C=9", "H=0 act=5"],
        -1: ["workspace=0", "sums=0"],
        -5: ["workspace_bytes=345855"],
    },
    "cde_dopri5_pending_sums_mlp": {
        -3: ["B=0", "B=-1", "C=0", "C=-1", "H=0", "H=-1"],
        -1: ["workspace=0", "sums=0"],
        -5: ["workspace_bytes=345855"],
    },
    "cde_dopri5_adjoint_advance": {
        -3: ["B=0", "B=-1", "C=0", "C=-1", "H=0", "H=-1", "n_intervals=0", "n_intervals=-1", "n_launches=-1", "n_jump=-1",
             "s0=0.0 s1=0.0", "s0=1.0 s1=0.0", "s0=nan", "B_global=63", "n_launches=2 B_global=64", "B_global=63 n_launches=1",
             "n_launches=2 reduced_sums=4096", "B_global=64 n_launches=0"],
        -2: ["dtype=7"],
        -4: ["dtype=1", "act=5", "act=2", "act=0x21", "act=0x11", "act=0x101", "act=16", "degree=2", "norm_kind=2",
             "norm_kind=-1", "H=33", "C=9", "C=17", "C=17 H=16", "H=64", "H=64 C=16", "H=257", "C=16 H=16", "C=16 H=32",
             "reduced_sums=4096 B_global=64 first_launch=1 n_launches=1 H=33"],
        -1: ["coeffs=0", "knots=0", "W=0", "bias=0", "y_init=0", "a_init=0", "a_out=0", "workspace=0", "n_jump=1 jump_s=0",
             "first_launch=1 B_global=64 n_launches=1"],
        -5: ["workspace_bytes=19985151"],
    },
    "cde_dopri5_adjoint_advance_dcontrol": {
        -3: ["B=0", "B=-1", "C=0", "C=-1", "H=0", "H=-1", "n_intervals=0", "n_intervals=-1", "n_launches=-1", "n_jump=-1",
             "s0=0.0 s1=0.0", "s0=1.0 s1=0.0", "s0=nan"],
        -2: ["dtype=7"],
        -4: ["control_numel=0", "control_numel=-1", "dtype=1", "act=5", "act=2", "act=0x21", "act=0x11", "act=0x101", "act=16",
             "degree=2", "norm_kind=2", "norm_kind=-1", "H=33", "C=9", "C=17", "C=17 H=16", "H=64", "H=64 C=16", "H=257",
             "C=16 H=16", "C=16 H=32"],
        -1: ["coeffs=0", "knots=0", "W=0", "bias=0", "y_init=0", "a_init=0", "a_out=0", "workspace=0", "grad_coeffs=0",
             "n_jump=1 jump_s=0", "grad_coeffs=0 grad_knots=0"],
        -5: ["workspace_bytes=20051199", "workspace_bytes=19985152"],
    },
    "cde_dopri5_adjoint_pending_sums": {
        -3: ["B=0", "B=-1", "C=0", "C=-1", "H=0", "H=-1", "total_launches=0", "total_launches=-1"],
        -1: ["workspace=0", "sums=0"],
        -5: ["workspace_bytes=19985151"],
    },
    "cde_dopri5_adjoint_state_sums": {
        -3: ["B=0", "B=-1", "C=0", "C=-1", "H=0", "H=-1", "total_launches=0", "total_launches=-1"],
        -1: ["workspace=0", "sums=0"],
        -5: ["workspace_bytes=19985151"],
    },
    "cde_dopri5_adjoint_apply_state_sums": {
        -3: ["B=0", "B=-1", "C=0", "C=-1", "H=0", "H=-1", "total_launches=0", "total_launches=-1"],
        -1: ["workspace=0", "reduced=0"],
        -5: ["workspace_bytes=19985151"],
    },
    "cde_dopri5_adjoint_apply_reduced": {
        -3: ["B=0", "B=-1", "C=0", "C=-1", "H=0", "H=-1", "total_launches=0", "total_launches=-1"],
        -1: ["workspace=0", "reduced=0"],
        -5: ["workspace_bytes=19985151"],
    },
    "cde_dopri5_adjoint_finish": {
        -3: ["B=0", "B=-1", "C=0", "C=-1", "H=0", "H=-1", "H=33", "C=9", "C=17", "C=17 H=16", "H=64", "H=64 C=16", "H=257",
             "C=16 H=16", "C=16 H=32"],
        -1: ["workspace=0", "grad_W=0", "grad_b=0"],
        -5: ["workspace_bytes=19985151"],
    },
    "cde_dopri5_adjoint_mlp_advance": {
        -3: ["B=0", "B=-1", "C=0", "C=-1", "H=0", "H=-1", "n_intervals=0", "n_intervals=-1", "width=0", "width=-1",
             "n_launches=-1", "n_jump=-1", "s0=0.0 s1=0.0", "s0=1.0 s1=0.0", "s0=nan", "bias1=0 width=0"],
        -2: ["dtype=7"],
        -4: ["dtype=1", "act=5", "act=2", "act=0x21", "act=0x101", "degree=2", "norm_kind=2", "norm_kind=-1", "H=33", "C=17",
             "C=17 H=16", "H=64", "H=64 C=16", "H=257"],
        -1: ["coeffs=0", "knots=0", "W1=0", "bias1=0", "W2=0", "bias2=0", "y_init=0", "a_init=0", "a_out=0", "workspace=0",
             "n_jump=1 jump_s=0"],
        -5: ["workspace_bytes=7474943"],
    },
    "cde_dopri5_adjoint_mlp_advance_dcontrol": {
        -3: ["B=0", "B=-1", "C=0", "C=-1", "H=0", "H=-1", "n_intervals=0", "n_intervals=-1", "width=0", "width=-1",
             "n_launches=-1", "n_jump=-1", "s0=0.0 s1=0.0", "s0=1.0 s1=0.0", "s0=nan", "bias1=0 width=0"],
        -2: ["dtype=7"],
        -4: ["control_numel=0", "control_numel=-1", "dtype=1", "act=5", "act=2", "act=0x21", "act=0x101", "degree=2",
             "norm_kind=2", "norm_kind=-1", "H=33", "C=17", "C=17 H=16", "H=64", "H=64 C=16", "H=257"],
        -1: ["coeffs=0", "knots=0", "W1=0", "bias1=0", "W2=0", "bias2=0", "y_init=0", "a_init=0", "a_out=0", "workspace=0",
             "grad_coeffs=0", "n_jump=1 jump_s=0", "grad_coeffs=0 grad_knots=0"],
        -5: ["workspace_bytes=7508735", "workspace_bytes=7474944"],
    },
    "cde_dopri5_adjoint_mlp_advance_sharded": {
        -3: ["B=0", "B=-1", "C=0", "C=-1", "H=0", "H=-1", "n_intervals=0", "n_intervals=-1", "width=0", "width=-1", "n_jump=-1",
             "B_global=0", "B_global=-1", "s0=0.0 s1=0.0", "s0=1.0 s1=0.0", "s0=nan", "bias1=0 width=0", "B_global=63"],
        -2: ["dtype=7"],
        -4: ["dtype=1", "act=5", "act=2", "act=0x21", "act=0x101", "degree=2", "norm_kind=2", "norm_kind=-1", "H=33", "C=9",
             "C=17", "C=17 H=16", "H=64", "H=64 C=16", "H=257", "C=16 H=32", "width=32 C=16 H=32", "C=16 H=32 width=32",
             "C=16 H=32 width=32 W2=4100"],
        -1: ["coeffs=0", "knots=0", "W1=0", "bias1=0", "W2=0", "bias2=0", "y_init=0", "a_init=0", "a_out=0", "workspace=0",
             "n_jump=1 jump_s=0", "first_launch=1 reduced_sums=0"],
        -5: ["workspace_bytes=7474943"],
    },
    "cde_dopri5_adjoint_mlp_pending_sums": {
        -3: ["B=0", "B=-1", "C=0", "C=-1", "H=0", "H=-1", "total_launches=0", "total_launches=-1"],
        -1: ["workspace=0", "sums=0"],
        -5: ["workspace_bytes=7474943"],
    },
    "cde_dopri5_adjoint_mlp_state_sums": {
        -3: ["B=0", "B=-1", "C=0", "C=-1", "H=0", "H=-1", "total_launches=0", "total_launches=-1"],
        -1: ["workspace=0", "sums=0"],
        -5: ["workspace_bytes=7474943"],
    },
    "cde_dopri5_adjoint_mlp_apply_state_sums": {
        -3: ["B=0", "B=-1", "C=0", "C=-1", "H=0", "H=-1", "total_launches=0", "total_launches=-1"],
        -1: ["workspace=0", "reduced=0"],
        -5: ["workspace_bytes=7474943"],
    },
    "cde_dopri5_adjoint_mlp_apply_reduced": {
        -3: ["B=0", "B=-1", "C=0", "C=-1", "H=0", "H=-1", "total_launches=0", "total_launches=-1"],
        -1: ["workspace=0", "reduced=0"],
        -5: ["workspace_bytes=7474943"],
    },
    # ---- interpolation, fills, log-signature windows: sizes, then the empty batch (a no-op whatever else is wrong), then
    # the pointers, then the dtype -- which nothing looks at before the kernel is chosen
    "cde_hermite_bdiff_coeffs": {
        -3: ["B=-1", "L=1", "C=0", "L=1 B=0", "C=0 x=0", "L=1 dtype=7"],
        0: ["B=0", "B=0 x=0", "B=0 dtype=7"],
        -1: ["x=0", "t=0", "coeffs=0", "x=0 dtype=7"],
        -2: ["dtype=7", "dtype=-1"],
    },
    "cde_hermite_bdiff_coeffs_checked": {
        -3: ["B=-1", "L=1", "C=0", "L=1 B=0", "C=0 nan_flag=0"],
        0: ["B=0", "B=0 nan_flag=0", "B=0 dtype=7"],
        -1: ["x=0", "t=0", "coeffs=0", "nan_flag=0", "nan_flag=0 dtype=7"],
        -2: ["dtype=7"],
    },
    "cde_hermite_bdiff_coeffs_nonblocking": {
        -3: ["B=-1", "L=1", "C=0", "generation=0", "generation=-1", "generation=0 B=0", "generation=0 x=0"],
        0: ["B=0", "B=0 scratch=0", "B=0 dtype=7"],
        -1: ["x=0", "t=0", "coeffs=0", "scratch=0", "nan_flag=0", "scratch=0 dtype=7"],
        -2: ["dtype=7"],
    },
    "cde_hermite_bdiff_coeffs_backward": {
        -3: ["B=-1", "L=1", "C=0", "L=1 B=0"],
        0: ["B=0", "B=0 t=0", "B=0 dtype=7"],
        -1: ["grad_coeffs=0", "t=0", "grad_x=0", "t=0 dtype=7"],
        -2: ["dtype=7"],
    },
    "cde_hermite_bdiff_coeffs_backward_dt": {
        -3: ["B=-1", "L=1", "C=0", "L=1 B=0"],
        0: ["B=0", "B=0 x=0", "B=0 dtype=7"],
        -1: ["grad_coeffs=0", "x=0", "t=0", "grad_h=0", "grad_h=0 dtype=7"],
        -2: ["dtype=7"],
    },
    "cde_linear_fill_missing": {
        -3: ["B=-1", "L=1", "C=0", "L=1 B=0"],
        0: ["B=0", "B=0 out=0", "B=0 dtype=7"],
        -1: ["x=0", "t=0", "out=0", "out=0 dtype=7"],
        -2: ["dtype=7"],
    },
    "cde_linear_fill_missing_backward": {
        -3: ["B=-1", "L=1", "C=0", "L=1 B=0"],
        0: ["B=0", "B=0 grad_x=0", "B=0 dtype=7"],
        -1: ["grad_out=0", "x=0", "t=0", "grad_x=0", "grad_out=0 dtype=7"],
        -2: ["dtype=7"],
    },
    # (the fills accept a single sample: L=1)
    "cde_forward_fill": {
        -3: ["B=-1", "L=0", "C=0", "L=0 B=0"],
        0: ["B=0", "B=0 x=0", "B=0 dtype=7"],
        -1: ["x=0", "out=0", "L=1 out=0", "x=0 dtype=7"],
        -2: ["dtype=7", "L=1 dtype=7"],
    },
    "cde_forward_fill_backward": {
        -3: ["B=-1", "L=0", "C=0", "L=0 B=0"],
        0: ["B=0", "B=0 x=0", "B=0 dtype=7"],
        -1: ["grad_out=0", "x=0", "grad_x=0", "L=1 grad_x=0", "x=0 dtype=7"],
        -2: ["dtype=7"],
    },
    "cde_rectilinear_prepare": {
        -3: ["B=-1", "L=0", "C=0", "time_index=-1", "time_index=3", "time_index=3 B=0", "time_index=-1 x=0"],
        0: ["B=0", "B=0 x=0", "B=0 dtype=7", "B=0 time_index=2"],
        -1: ["x=0", "out=0", "time_index=2 out=0", "x=0 dtype=7"],
        -2: ["dtype=7"],
    },
    "cde_rectilinear_prepare_backward": {
        -3: ["B=-1", "L=0", "C=0", "time_index=-1", "time_index=3", "time_index=3 B=0", "time_index=-1 x=0"],
        0: ["B=0", "B=0 x=0", "B=0 dtype=7", "B=0 time_index=2"],
        -1: ["grad_out=0", "x=0", "grad_x=0", "time_index=2 grad_x=0", "x=0 dtype=7"],
        -2: ["dtype=7"],
    },
    "cde_natural_cubic_coeffs": {
        -3: ["B=-1", "L=1", "C=0", "version=2", "version=-1", "version=2 B=0", "version=2 x=0"],
        0: ["B=0", "B=0 x=0", "B=0 dtype=7", "B=0 version=1"],
        -1: ["x=0", "t=0", "coeffs=0", "version=1 coeffs=0", "has_missing=1 x=0", "x=0 dtype=7"],
        -2: ["dtype=7", "version=1 has_missing=1 dtype=7"],
    },
    # a size query: the "code" of a row is the number of bytes (an unknown dtype counts as four-byte elements)
    "cde_natural_cubic_coeffs_backward_workspace_bytes": {
        40: ["", "dtype=7"],
        80: ["dtype=1"],
        16: ["L=2"],
        0: ["L=0"],
    },
    # (x and kd_scratch are needed only with grad_t_rows; the workspace is sized after the dtype is known)
    "cde_natural_cubic_coeffs_backward": {
        -3: ["B=-1", "L=1", "C=0", "L=1 B=0", "C=0 workspace_bytes=0"],
        0: ["B=0", "B=0 workspace=0", "B=0 dtype=7", "B=0 workspace_bytes=0"],
        -1: ["grad_coeffs=0", "t=0", "grad_x=0", "workspace=0", "x=0", "kd_scratch=0", "workspace=0 dtype=7",
             "kd_scratch=0 dtype=7", "x=0 workspace_bytes=0", "grad_t_rows=0 workspace=0"],
        -2: ["dtype=7", "dtype=7 workspace_bytes=0", "grad_t_rows=0 x=0 kd_scratch=0 dtype=7"],
        -5: ["workspace_bytes=39", "workspace_bytes=0", "dtype=1 workspace_bytes=79", "dtype=1",
             "grad_t_rows=0 workspace_bytes=39", "grad_t_rows=0 x=0 kd_scratch=0 workspace_bytes=39",
             "L=6 workspace_bytes=47"],
    },
    "cde_natural_cubic_coeffs_backward_missing": {
        -3: ["B=-1", "L=1", "C=0", "version=2", "version=-1", "version=2 B=0", "version=2 workspace=0"],
        0: ["B=0", "B=0 workspace=0", "B=0 dtype=7", "B=0 version=1"],
        -1: ["grad_coeffs=0", "x=0", "t=0", "grad_x=0", "workspace=0", "version=1 workspace=0", "workspace=0 dtype=7"],
        -2: ["dtype=7", "version=1 dtype=7"],
    },
    # the envelopes (8 channels, depth 3), (5, 4), (32, 2) are looked at before the empty batch and the pointers; the rows
    # inside an envelope fail a later check
    "cde_logsig_windows": {
        -3: ["B=-1", "L=0", "C=0", "n_windows=-1", "n_words=0", "L=0 depth=5", "n_words=0 C=33", "n_windows=-1 B=0"],
        -4: ["depth=0", "depth=-1", "depth=5", "depth=4 C=6", "depth=3 C=9", "C=33", "depth=1 C=33", "depth=3 C=33",
             "depth=4 C=6 B=0", "depth=5 B=0", "depth=5 x=0", "depth=3 C=9 dtype=7"],
        0: ["B=0", "B=0 x=0", "B=0 dtype=7", "B=0 depth=3 C=8", "B=0 depth=4 C=5", "B=0 C=32"],
        -1: ["x=0", "rows=0", "scale=0", "words=0", "out=0", "depth=3 C=8 x=0", "depth=1 C=8 rows=0", "depth=4 C=5 scale=0",
             "depth=4 C=1 words=0", "C=32 out=0", "depth=1 C=32 x=0", "depth=3 C=8 out=0 dtype=7", "n_windows=0 x=0"],
        -2: ["dtype=7", "depth=3 C=8 dtype=7", "depth=4 C=5 dtype=7", "C=32 dtype=7", "n_windows=0 dtype=7", "L=1 dtype=7"],
    },
    "cde_logsig_windows_backward": {
        -3: ["B=-1", "L=0", "C=0", "n_windows=-1", "n_words=0", "L=0 depth=5", "n_words=0 C=33", "n_windows=-1 B=0"],
        -4: ["depth=0", "depth=-1", "depth=5", "depth=4 C=6", "depth=3 C=9", "C=33", "depth=1 C=33", "depth=3 C=33",
             "depth=4 C=6 B=0", "depth=5 B=0", "depth=5 x=0", "depth=3 C=9 dtype=7"],
        0: ["B=0", "B=0 x=0", "B=0 dtype=7", "B=0 depth=3 C=8", "B=0 depth=4 C=5", "B=0 C=32"],
        -1: ["grad_out=0", "x=0", "rows=0", "scale=0", "words=0", "grad_x=0", "workspace=0", "depth=3 C=8 x=0",
             "depth=1 C=8 rows=0", "depth=4 C=5 scale=0", "depth=4 C=1 words=0", "C=32 grad_x=0", "depth=1 C=32 workspace=0",
             "depth=3 C=8 grad_out=0 dtype=7", "n_windows=0 x=0"],
        -2: ["dtype=7", "depth=3 C=8 dtype=7", "depth=4 C=5 dtype=7", "C=32 dtype=7", "n_windows=0 dtype=7", "L=1 dtype=7"],
    },
    "cde_interpret_t": {
        -3: ["n_intervals=0", "n_intervals=-1", "nq=-1", "n_intervals=0 nq=0", "nq=-1 knots=0"],
        0: ["nq=0", "nq=0 knots=0", "nq=0 dtype=7"],
        -1: ["knots=0", "tq=0", "index_out=0", "frac_out=0", "n_intervals=1 tq=0", "frac_out=0 dtype=7"],
        -2: ["dtype=7", "n_intervals=1 dtype=7"],
    },
    # an unknown degree or `what` is noticed where the kernel is chosen: after the pointers and the dtype
    "cde_path_eval": {
        -3: ["B=-1", "n_intervals=0", "C=0", "nq=-1", "n_intervals=0 B=0", "nq=-1 B=0", "C=0 degree=2", "C=0 nq=0"],
        0: ["B=0", "nq=0", "B=0 nq=0", "B=0 coeffs=0", "nq=0 out=0", "B=0 dtype=7", "nq=0 degree=2", "B=0 what=2"],
        -1: ["coeffs=0", "knots=0", "tq=0", "out=0", "coeffs=0 degree=2", "out=0 what=2", "coeffs=0 dtype=7",
             "degree=1 knots=0", "what=1 tq=0"],
        -2: ["dtype=7", "dtype=7 degree=2", "dtype=7 what=2", "dtype=7 degree=1 what=1"],
        -4: ["degree=2", "degree=0", "degree=-1", "what=2", "what=-1", "degree=2 what=2", "degree=1 what=2",
             "degree=2 what=1", "dtype=1 degree=2", "dtype=1 what=2"],
    },
    "cde_path_eval_backward": {
        -3: ["B=-1", "n_intervals=0", "C=0", "nq=-1", "n_intervals=0 B=0", "nq=-1 B=0", "C=0 degree=2", "C=0 nq=0"],
        0: ["B=0", "nq=0", "B=0 nq=0", "B=0 grad_out=0", "nq=0 grad_coeffs=0", "B=0 dtype=7", "nq=0 degree=2", "B=0 what=2"],
        -1: ["grad_out=0", "knots=0", "tq=0", "grad_coeffs=0", "grad_out=0 degree=2", "grad_coeffs=0 what=2",
             "grad_out=0 dtype=7", "degree=1 knots=0", "what=1 tq=0"],
        -2: ["dtype=7", "dtype=7 degree=2", "dtype=7 what=2", "dtype=7 degree=1 what=1"],
        -4: ["degree=2", "degree=0", "degree=-1", "what=2", "what=-1", "degree=2 what=2", "degree=1 what=2",
             "degree=2 what=1", "dtype=1 degree=2", "dtype=1 what=2"],
    },
    "cde_contract": {
        -3: ["B=-1", "H=0", "C=0", "H=0 B=0", "C=0 F=0"],
        0: ["B=0", "B=0 F=0", "B=0 dtype=7"],
        -1: ["F=0", "dX=0", "out=0", "out=0 dtype=7"],
        -2: ["dtype=7"],
    },
}

# Every size / offset query of the adaptive solvers at default options: LAYOUT[query][i][j] for batch LAYOUT_B[i] and
# (C, H) = LAYOUT_CH[j]; the batch sizes straddle every form switch of the layouts.  "name key=v": one more int argument.
LAYOUT_B = [1, 16, 17, 256 * 16, 256 * 16 + 1, 1024 * 16 + 1]
LAYOUT_CH = [(3, 5), (8, 32), (16, 16), (16, 32), (8, 64)]
LAYOUT = {
    "cde_dopri5_workspace_bytes dtype=0": [
        [264192, 265216, 264704, 265216, 266496],
        [267264, 284416, 274176, 284416, 304896],
        [267520, 285696, 274944, 285696, 307456],
        [1083136, 5506816, 2885376, 5506816, 10766080],
        [1083392, 5508352, 2886144, 5508352, 10768896],
        [3557632, 21285888, 10767104, 21285888, 42258688],
    ],
    "cde_dopri5_workspace_bytes dtype=1": [
        [264448, 266496, 265216, 266496, 269056],
        [270336, 304896, 284416, 304896, 345856],
        [270848, 307456, 285696, 307456, 350976],
        [1902336, 10749696, 5506816, 10749696, 21251840],
        [1902848, 10752512, 5508096, 10752512, 21257216],
        [6834688, 42258688, 21253376, 42258688, 84204288],
    ],
    "cde_dopri5_trace_offset dtype=0": [
        [165888, 166912, 166400, 166912, 168192],
        [168960, 186112, 175872, 186112, 206592],
        [169216, 187392, 176640, 187392, 209152],
        [984832, 5408512, 2787072, 5408512, 10667776],
        [985088, 5410048, 2787840, 5410048, 10670592],
        [3459328, 21187584, 10668800, 21187584, 42160384],
    ],
    "cde_dopri5_trace_offset dtype=1": [
        [166144, 168192, 166912, 168192, 170752],
        [172032, 206592, 186112, 206592, 247552],
        [172544, 209152, 187392, 209152, 252672],
        [1804032, 10651392, 5408512, 10651392, 21153536],
        [1804544, 10654208, 5409792, 10654208, 21158912],
        [6736384, 42160384, 21155072, 42160384, 84105984],
    ],
    "cde_dopri5_adjoint_workspace_bytes": [
        [19919872, 19920640, 19920128, 19920640, 19921664],
        [19922176, 19936000, 19927808, 19936000, 19952384],
        [19922432, 19937024, 19928320, 19937024, 19954432],
        [20574976, 24113920, 22016768, 24113920, 28308224],
        [20575232, 24114944, 22017280, 24114944, 28310272],
        [22541312, 36697856, 28308736, 36697856, 53476096],
    ],
    "cde_dopri5_adjoint_dcontrol_workspace_bytes": [
        [19953664, 19954432, 19953920, 19954432, 19955456],
        [19963648, 19977472, 19969280, 19977472, 19993856],
        [19964416, 19979008, 19970304, 19979008, 19996416],
        [22709504, 26248448, 24151296, 26248448, 30442752],
        [22710272, 26249984, 24152320, 26249984, 30445312],
        [30980096, 45136640, 36747520, 45136640, 61914880],
    ],
    "cde_dopri5_adjoint_trace_offset": [
        [19166208, 19166976, 19166464, 19166976, 19168000],
        [19168512, 19182336, 19174144, 19182336, 19198720],
        [19168768, 19183360, 19174656, 19183360, 19200768],
        [19821312, 23360256, 21263104, 23360256, 27554560],
        [19821568, 23361280, 21263616, 23361280, 27556608],
        [21787648, 35944192, 27555072, 35944192, 52722432],
    ],
    "cde_dopri5_adjoint_attempt_trace_offset": [
        [19264512, 19265280, 19264768, 19265280, 19266304],
        [19266816, 19280640, 19272448, 19280640, 19297024],
        [19267072, 19281664, 19272960, 19281664, 19299072],
        [19919616, 23458560, 21361408, 23458560, 27652864],
        [19919872, 23459584, 21361920, 23459584, 27654912],
        [21885952, 36042496, 27653376, 36042496, 52820736],
    ],
    "cde_dopri5_adjoint_carry_offset": [
        [70144, 70144, 70144, 70144, 70144],
        [70144, 70144, 70144, 70144, 70144],
        [70144, 70144, 70144, 70144, 70144],
        [70144, 70144, 70144, 70144, 70144],
        [70144, 70144, 70144, 70144, 70144],
        [70144, 70144, 70144, 70144, 70144],
    ],
    "cde_dopri5_adjoint_mlp_workspace_bytes": [
        [7271424, 7272960, 7271936, 11944960, 7274752],
        [7276288, 7300352, 7286016, 11972352, 7329024],
        [7305472, 7331072, 7315712, 12003072, 7361536],
        [116394240, 122587392, 118917376, 187446016, 129927424],
        [116423680, 122618368, 118922752, 187452416, 129960192],
        [330402816, 355176960, 340495872, 507198464, 384538880],
    ],
    "cde_dopri5_adjoint_mlp_dcontrol_workspace_bytes": [
        [7272704, 7274240, 7273728, 11946752, 7276032],
        [7285248, 7309312, 7303168, 11989504, 7337984],
        [7314944, 7340544, 7333888, 12021248, 7371008],
        [118528768, 124721920, 123153152, 191681792, 132061952],
        [118558976, 124753664, 123135232, 191664896, 132095488],
        [338825472, 363599616, 357324032, 524026624, 392961536],
    ],
    "cde_dopri5_adjoint_mlp_carry_offset": [
        [149760, 149760, 149760, 298752, 149760],
        [149760, 149760, 149760, 298752, 149760],
        [149760, 149760, 149760, 298752, 149760],
        [182272, 182272, 182272, 331264, 182272],
        [182528, 182528, 157952, 306944, 182528],
        [166144, 166144, 166144, 315136, 166144],
    ],
    "cde_dopri5_adjoint_mlp_gradient_offset": [
        [582912, 583680, 583168, 732672, 584704],
        [585216, 599040, 590848, 748032, 615424],
        [585472, 600064, 591360, 749056, 617472],
        [1270528, 4809472, 2712320, 4958464, 9003776],
        [1271040, 4810752, 2688512, 4935168, 9006080],
        [3220736, 17377280, 8988160, 17526272, 34155520],
    ],
    "cde_dopri5_adjoint_mlp_gradient_upper_offset": [
        [0, 0, 0, 1626624, 0],
        [0, 0, 0, 1641984, 0],
        [0, 0, 0, 1643008, 0],
        [0, 0, 0, 5852416, 0],
        [0, 0, 0, 5829120, 0],
        [0, 0, 0, 18420224, 0],
    ],
    "cde_dopri5_adjoint_mlp_trace_offset which=0": [
        [6517760, 6519296, 6518272, 11191296, 6521088],
        [6522624, 6546688, 6532352, 11218688, 6575360],
        [6551808, 6577408, 6562048, 11249408, 6607872],
        [115640576, 121833728, 118163712, 186692352, 129173760],
        [115670016, 121864704, 118169088, 186698752, 129206528],
        [329649152, 354423296, 339742208, 506444800, 383785216],
    ],
    "cde_dopri5_adjoint_mlp_trace_offset which=1": [
        [6616064, 6617600, 6616576, 11289600, 6619392],
        [6620928, 6644992, 6630656, 11316992, 6673664],
        [6650112, 6675712, 6660352, 11347712, 6706176],
        [115738880, 121932032, 118262016, 186790656, 129272064],
        [115768320, 121963008, 118267392, 186797056, 129304832],
        [329747456, 354521600, 339840512, 506543104, 383883520],
    ],
    "cde_dopri5_adjoint_status_stride": 256,
    "cde_dopri5_adjoint_reduced_count": 18440,
    "cde_dopri5_adjoint_mlp_reduced_count": 74504,
}


def _value(text):
    try:
        return int(text, 0)
    except ValueError:
        return float(text)


def build_args(spec, overrides=""):
    over = dict(tok.split("=") for tok in overrides.split())
    args = []
    for tok in spec.split():
        name, _, value = tok.partition("=")
        args.append(_value(over.get(name, value or str(DUMMY))))
    assert not set(over) - {t.partition("=")[0] for t in spec.split()}, overrides
    return args
