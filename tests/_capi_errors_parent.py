"""Return codes of the 18 single-set per-point entry points for the argument cases of tests/test_capi_errors.py, recorded once from the
build before the entry points were folded into one table-driven helper; never regenerated.  entry point -> {case: code}; 0 = PINN_OK,
-1 = PINN_ERR_NULL, -2 = _LAYERS, -3 = _PRECISION, -4 = _WORKSPACE, -5 = _SIZE.  Recorded from the x86 emulator build; the gfx950 library
gave the same code for every case that is negative here (those return before any HIP call)."""
CODES = {
    "pinn_wave2d_loss_grad": {
        "valid": 0, "params NULL": -1, "workspace NULL": -1, "x NULL": -1, "y NULL": -1, "t NULL": -1, "term_weights NULL": -1,
        "loss_terms_out NULL": -1, "grad_flat_out NULL": -1, "n = -1": -5, "normalize, lb NULL": -1, "precision 7": -3, "layers [3, 32, 48, 7]": -2,
        "wrong output count": -2, "wrong input count": -2, "n = -1, params NULL": -1, "loss_terms_out NULL, wrong output count": -1,
    },
    "pinn_data_loss_grad": {
        "valid": 0, "params NULL": -1, "workspace NULL": -1, "x NULL": -1, "y NULL": -1, "t NULL": -1, "targets NULL": 0, "out_weights NULL": -1,
        "loss_terms_out NULL": -1, "grad_flat_out NULL": -1, "n = -1": -5, "normalize, lb NULL": -1, "precision 7": -3, "layers [3, 32, 48, 7]": -2,
        "wrong output count": 0, "wrong input count": -2, "n = -1, params NULL": -1, "loss_terms_out NULL, wrong output count": -1,
    },
    "pinn_wave2d_fields": {
        "valid": 0, "params NULL": -1, "workspace NULL": -1, "x NULL": -1, "y NULL": -1, "t NULL": -1, "fields_out NULL": -1, "n = -1": -5,
        "normalize, lb NULL": -1, "precision 7": -3, "layers [3, 32, 48, 7]": -2, "wrong output count": 0, "wrong input count": -2,
        "n = -1, params NULL": -1, "fields_out NULL, wrong output count": -1,
    },
    "pinn_wave2d_residual_score": {
        "valid": 0, "params NULL": -1, "workspace NULL": -1, "x NULL": -1, "y NULL": -1, "t NULL": -1, "term_weights NULL": -1, "score_out NULL": -1,
        "n = -1": -5, "normalize, lb NULL": -1, "precision 7": -3, "layers [3, 32, 48, 7]": -2, "wrong output count": -2, "wrong input count": -2,
        "n = -1, params NULL": -1, "score_out NULL, wrong output count": -1,
    },
    "pinn_wave2d_predict": {
        "valid": 0, "params NULL": -1, "workspace NULL": -1, "x NULL": -1, "y NULL": -1, "t NULL": -1, "out NULL": -1, "n = -1": -5,
        "normalize, lb NULL": -1, "precision 7": -3, "layers [3, 32, 48, 7]": -2, "wrong output count": -2, "wrong input count": -2,
        "n = -1, params NULL": -1, "out NULL, wrong output count": -1,
    },
    "pinn_wave2d_material_sums": {
        "valid": 0, "params NULL": -1, "workspace NULL": -1, "x NULL": -1, "y NULL": -1, "t NULL": -1, "sums_out NULL": -1, "sums_workspace NULL": -1,
        "n = -1": -5, "normalize, lb NULL": -1, "precision 7": -3, "layers [3, 32, 48, 7]": -2, "wrong output count": -2, "wrong input count": -2,
        "sums workspace off alignment": -4, "sums workspace one byte short": -4, "n = -1, params NULL": -1, "sums_out NULL, wrong output count": -1,
        "wrong output count, sums workspace one byte short": -2,
    },
    "pinn_net_streams": {
        "valid": 0, "params NULL": -1, "workspace NULL": -1, "x NULL": -1, "y NULL": -1, "t NULL": -1, "streams_out NULL": -1, "n = -1": -5,
        "normalize, lb NULL": -1, "precision 7": -3, "bf16": -3, "f16": -2, "layers [3, 32, 48, 7]": -2, "wrong output count": 0,
        "wrong input count": -2, "n = -1, params NULL": -1, "streams_out NULL, wrong output count": -1,
    },
    "pinn_plate2d_loss_grad": {
        "valid": 0, "params NULL": -1, "workspace NULL": -1, "x NULL": -1, "y NULL": -1, "t NULL": -1, "frozen_streams NULL": -1,
        "term_weights NULL": -1, "loss_terms_out NULL": -1, "grad_flat_out NULL": -1, "n = -1": -5, "normalize, lb NULL": -1, "precision 7": -3,
        "bf16": -3, "f16": -2, "layers [3, 32, 48, 7]": -2, "wrong output count": -2, "wrong input count": -2, "n = -1, params NULL": -1,
        "loss_terms_out NULL, wrong output count": -1,
    },
    "pinn_plate2d_residual_score": {
        "valid": 0, "params NULL": -1, "workspace NULL": -1, "x NULL": -1, "y NULL": -1, "t NULL": -1, "frozen_streams NULL": -1,
        "term_weights NULL": -1, "score_out NULL": -1, "n = -1": -5, "normalize, lb NULL": -1, "precision 7": -3, "bf16": -3, "f16": -2,
        "layers [3, 32, 48, 7]": -2, "wrong output count": -2, "wrong input count": -2, "n = -1, params NULL": -1,
        "score_out NULL, wrong output count": -1,
    },
    "pinn_plate2d_material_sums": {
        "valid": 0, "params NULL": -1, "workspace NULL": -1, "x NULL": -1, "y NULL": -1, "t NULL": -1, "frozen_streams NULL": -1, "sums_out NULL": -1,
        "sums_workspace NULL": -1, "n = -1": -5, "normalize, lb NULL": -1, "precision 7": -3, "bf16": -3, "f16": -2, "layers [3, 32, 48, 7]": -2,
        "wrong output count": -2, "wrong input count": -2, "sums workspace off alignment": -4, "sums workspace one byte short": -4,
        "n = -1, params NULL": -1, "sums_out NULL, wrong output count": -1, "wrong output count, sums workspace one byte short": -2,
    },
    "pinn_plate2d_predict": {
        "valid": 0, "params NULL": -1, "workspace NULL": -1, "x NULL": -1, "y NULL": -1, "t NULL": -1, "frozen_streams NULL": -1, "out NULL": -1,
        "n = -1": -5, "normalize, lb NULL": -1, "precision 7": -3, "bf16": -3, "f16": -2, "layers [3, 32, 48, 7]": -2, "wrong output count": -2,
        "wrong input count": -2, "n = -1, params NULL": -1, "out NULL, wrong output count": -1,
    },
    "pinn_plate2d_traction_loss_grad": {
        "valid": 0, "params NULL": -1, "workspace NULL": -1, "x NULL": -1, "y NULL": -1, "t NULL": -1, "frozen_and_normals NULL": -1,
        "weights NULL": -1, "loss_terms_out NULL": -1, "grad_flat_out NULL": -1, "n = -1": -5, "normalize, lb NULL": -1, "precision 7": -3,
        "bf16": -3, "f16": -2, "layers [3, 32, 48, 7]": -2, "wrong output count": -2, "wrong input count": -2, "n = -1, params NULL": -1,
        "loss_terms_out NULL, wrong output count": -1,
    },
    "pinn_stream_loss_grad": {
        "valid": 0, "params NULL": -1, "workspace NULL": -1, "x NULL": -1, "y NULL": -1, "t NULL": -1, "targets NULL": 0, "weights NULL": -1,
        "loss_terms_out NULL": -1, "grad_flat_out NULL": -1, "n = -1": -5, "normalize, lb NULL": -1, "precision 7": -3, "bf16": -3, "f16": -2,
        "layers [3, 32, 48, 7]": -2, "wrong output count": 0, "wrong input count": -2, "n = -1, params NULL": -1,
        "loss_terms_out NULL, wrong output count": -1,
    },
    "pinn_nc3d_loss_grad": {
        "valid": 0, "params NULL": -1, "workspace NULL": -1, "x NULL": -1, "y NULL": -1, "z NULL": -1, "t NULL": -1, "term_weights NULL": -1,
        "loss_terms_out NULL": -1, "grad_flat_out NULL": -1, "n = -1": -5, "normalize, lb NULL": -1, "precision 7": -3, "bf16": -3, "f16": -2,
        "layers [3, 32, 48, 7]": -2, "wrong output count": -2, "wrong input count": -2, "n = -1, params NULL": -1,
        "loss_terms_out NULL, wrong output count": -1,
    },
    "pinn_nc3d_data_loss_grad": {
        "valid": 0, "params NULL": -1, "workspace NULL": -1, "x NULL": -1, "y NULL": -1, "z NULL": -1, "t NULL": -1, "targets NULL": 0,
        "out_weights NULL": -1, "loss_terms_out NULL": -1, "grad_flat_out NULL": -1, "n = -1": -5, "normalize, lb NULL": -1, "precision 7": -3,
        "bf16": -3, "f16": -2, "layers [3, 32, 48, 7]": -2, "wrong output count": 0, "wrong input count": -2, "n = -1, params NULL": -1,
        "loss_terms_out NULL, wrong output count": -1,
    },
    "pinn_nc3d_fields": {
        "valid": 0, "params NULL": -1, "workspace NULL": -1, "x NULL": -1, "y NULL": -1, "z NULL": -1, "t NULL": -1, "fields_out NULL": -1,
        "n = -1": -5, "normalize, lb NULL": -1, "precision 7": -3, "bf16": -3, "f16": -2, "layers [3, 32, 48, 7]": -2, "wrong output count": 0,
        "wrong input count": -2, "n = -1, params NULL": -1, "fields_out NULL, wrong output count": -1,
    },
    "pinn_nc3d_residual_score": {
        "valid": 0, "params NULL": -1, "workspace NULL": -1, "x NULL": -1, "y NULL": -1, "z NULL": -1, "t NULL": -1, "term_weights NULL": -1,
        "score_out NULL": -1, "n = -1": -5, "normalize, lb NULL": -1, "precision 7": -3, "bf16": -3, "f16": -2, "layers [3, 32, 48, 7]": -2,
        "wrong output count": -2, "wrong input count": -2, "n = -1, params NULL": -1, "score_out NULL, wrong output count": -1,
    },
    "pinn_nc3d_material_sums": {
        "valid": 0, "params NULL": -1, "workspace NULL": -1, "x NULL": -1, "y NULL": -1, "z NULL": -1, "t NULL": -1, "sums_out NULL": -1,
        "sums_workspace NULL": -1, "n = -1": -5, "normalize, lb NULL": -1, "precision 7": -3, "bf16": -3, "f16": -2, "layers [3, 32, 48, 7]": -2,
        "wrong output count": -2, "wrong input count": -2, "sums workspace off alignment": -4, "sums workspace one byte short": -4,
        "n = -1, params NULL": -1, "sums_out NULL, wrong output count": -1, "wrong output count, sums workspace one byte short": -2,
    },
}
