"""
_lib.py -- ctypes binding of libtdaeeg.so (the C ABI in include/tdaeeg.h).

The HIP library is the product; there is NO CPU fallback.  If the shared object is
missing or no MI355X is visible, every entry point raises.  Build it with
``python -c "import __graft_entry__ as g; g.build()"`` or ``make -C tda_eeg_audio_amd/csrc``.
"""
import contextlib
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# TDA_LIB=libtdaeeg_<variant>.so: a diagnostic / A-B build from csrc/Makefile (same directory); the product library otherwise
LIB_PATH = os.path.join(_HERE, os.path.basename(os.environ.get("TDA_LIB", "libtdaeeg.so")))

c_dp = C.POINTER(C.c_double)
c_ip = C.POINTER(C.c_int)
c_vp = C.c_void_p

TDA_WIN_H1_TRUNCATED = 1
TDA_WIN_CLASS_OVERFLOW = 2
TDA_WIN_DEGENERATE = 4
TDA_WIN_NOT_CONVERGED = 8
TDA_WIN_TOO_LARGE = 16
TDA_WIN_NO_PAIR = 32          # tda_wasserstein_cross_dev: no partner at this position (mvm:89)
TDA_WIN_NOT_FINITE = 64       # tda_sublevel_batch / tda_plv_dist_batch: a sample of the signal / window is not finite
N_FEATURES = 11
MAX_LANDSCAPES = 8          # TDA_MAX_LANDSCAPES
MAX_GRID = 256              # TDA_MAX_GRID
MAX_IMAGE_SIDE = 32         # TDA_MAX_IMAGE_SIDE
EC_MAX_DIM = 3              # TDA_EC_MAX_DIM: highest simplex dimension of the Euler characteristic curves
MAX_POINTS = 128
NET_ROWS = 10               # TDA_NET_ROWS: integer rows of the network curves (include/tdaeeg.h, "Network curves")
NET_MEASURES = 4            # TDA_NET_MEASURES: their float64 rows
NET_NODAL = 5               # TDA_NET_NODAL: their per-vertex rows
NET_COUNT_NAMES = ("edges", "isolated", "max_degree", "wedges", "triangles", "components", "largest", "pairs", "hops",
                   "diameter")
NET_MEASURE_NAMES = ("transitivity", "clustering", "efficiency", "path_length")
NET_NODAL_NAMES = ("degree", "triangles", "reach", "farness", "eccentricity")
RQA_ROWS = 7                # TDA_RQA_ROWS: integer rows of the recurrence curves (include/tdaeeg.h, "Recurrence curves")
RQA_MEASURES = 7            # TDA_RQA_MEASURES: their float64 rows
RQA_COUNT_NAMES = ("recurrences", "diag_lines", "diag_points", "diag_longest", "vert_lines", "vert_points", "vert_longest")
RQA_MEASURE_NAMES = ("recurrence_rate", "determinism", "diag_mean", "diag_entropy", "laminarity", "trapping_time",
                     "vert_entropy")
AMI_MAX_SAMPLES = 8192      # TDA_AMI_MAX_SAMPLES: longest window of the average mutual information (include/tdaeeg.h,
AMI_MAX_BINS = 32           # TDA_AMI_MAX_BINS           "Delay and dimension selection")
FNN_MAX_SAMPLES = 2048      # TDA_FNN_MAX_SAMPLES: longest window of the false nearest neighbours
FNN_MAX_DIM = 8             # TDA_FNN_MAX_DIM: highest dimension they test
FNN_COLS = 4                # TDA_FNN_COLS: the columns of their counts
FNN_COUNT_NAMES = ("valid", "false_distance", "false_size", "false_either")
TDA_GEN_BIRTH_TIED = 1       # tda_generators_*: flags of an H1 row (include/tdaeeg.h)
TDA_GEN_DEATH_TIED = 2
TDA_GEN_CYCLE_TRUNCATED = 4
TDA_GEN_NO_EDGE = 8
MAX_DIRECTIONS = 128        # TDA_MAX_DIRECTIONS
SW_MAX_POINTS = 512         # TDA_SW_MAX_POINTS
FM_MAX_ITER = 64            # TDA_FM_MAX_ITER
FM_MAX_POINTS = 512         # TDA_FM_MAX_POINTS
TDA_GROUND_L2 = 0           # tda_wasserstein_q_batch: (d - b) / sqrt 2 to the diagonal
TDA_GROUND_LINF = 1         # ... (d - b) / 2, the convention of the bottleneck distance
TDA_KW_ONE = 0              # tda_diagram_kernel_*: row weight 1.0
TDA_KW_PERS = 1             # ... the persistence d - b
TDA_KW_ATAN = 2             # ... atan(wc * (d - b))
PF_MAX_POINTS = 512         # TDA_PF_MAX_POINTS
LM_MAX_POINTS = 1024        # TDA_LM_MAX_POINTS: largest cloud the greedy permutation (n_perm) takes
LM_MAX_SAMPLES = 4096       # TDA_LM_MAX_SAMPLES
SL_MAX_SAMPLES = 4096       # TDA_SL_MAX_SAMPLES: longest signal of the sublevel-set persistence
PLV_MAX_CHANNELS = 64       # TDA_PLV_MAX_CHANNELS: most channels of a phase-locking value window
PLV_MAX_SAMPLES = 256       # TDA_PLV_MAX_SAMPLES: longest one
CONN_TAU = 2.0 ** -40       # TDA_CONN_TAU: the threshold of the analytic-signal connectivity's degenerate cases
TDA_CONN_WPLI = 0           # tda_connectivity_dist_batch: the weighted phase-lag index
TDA_CONN_IMCOH = 1          # ... the imaginary part of coherency
TDA_CONN_COH = 2            # ... coherence
TDA_CONN_AEC = 3            # ... amplitude-envelope correlation
PT_ROW_BLOCK = 64           # TDA_PT_ROW_BLOCK: rows per block of the permutation sums' written order
PT_MAX_ITEMS = 4096         # TDA_PT_MAX_ITEMS: largest matrix side of tda_perm_sums_batch
PT_MAX_PERM = 1048576       # TDA_PT_MAX_PERM: most relabellings of a call
PT_MAX_MATRICES = 4096      # TDA_PT_MAX_MATRICES: most matrices of a call


def pt_words(n_perm):
    """TDA_PT_WORDS: 64-bit label words per item."""
    return (int(n_perm) + 63) // 64


def pt_blocks(n):
    """TDA_PT_BLOCKS: row blocks of an n x n matrix."""
    return (int(n) + PT_ROW_BLOCK - 1) // PT_ROW_BLOCK


def pt_work_doubles(n_mat, n, n_perm):
    """TDA_PT_WORK_DOUBLES: doubles of device work space tda_perm_sums_batch_dev needs."""
    return int(n_mat) * pt_blocks(n) * 3 * 64 * pt_words(n_perm)


# every symbol include/tdaeeg.h declares: (name, restype, argtypes)
_I, _D = C.c_int, C.c_double
# the row inputs and outputs the tda_generators_* entry points share: h0, h0_cap, h0_cnt, h1, h1_cap, h1_cnt, rips_status,
# skip_mask, cyc_cap, h1_gen, h1_flag, cyc, cyc_len, part, h0_edge, work
_GEN = [c_vp, _I, c_vp, c_vp, _I, c_vp, c_vp, _I, _I, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]
# theiler, l_min, v_min and the outputs counts, measures, hist of the tda_recurrence_* entry points
_RQ = [_I, _I, _I, c_vp, c_vp, c_vp]
SYMBOLS = {
    "tda_version": (_I, []),
    "tda_ctx_create": (_I, [_I, C.POINTER(c_vp)]),
    "tda_ctx_destroy": (None, [c_vp]),
    "tda_last_error": (C.c_size_t, [c_vp, C.c_char_p, C.c_size_t]),
    "tda_set_class_words": (_I, [c_vp, _I, _I]),
    "tda_corr_dist_batch_dev": (_I, [c_vp, c_vp, _I, _I, _I, c_vp, c_vp, c_vp]),
    "tda_corr_dist_batch": (_I, [c_vp, c_vp, _I, _I, _I, c_vp, c_vp]),
    "tda_corr_dist_sliding_dev": (_I, [c_vp, c_vp, _I, _I, _I, _I, c_vp, c_vp, c_vp, c_vp]),
    "tda_corr_dist_sliding": (_I, [c_vp, c_vp, _I, _I, _I, _I, c_vp, c_vp, c_vp]),
    "tda_corr_to_dist_batch_dev": (_I, [c_vp, c_vp, _I, _I, _I, c_vp, c_vp]),
    "tda_corr_to_dist_batch": (_I, [c_vp, c_vp, _I, _I, _I, c_vp]),
    "tda_rips_dm_batch_dev": (_I, [c_vp, c_vp, _I, _I, _D, _I, c_vp, _I, c_vp, c_vp, _I, c_vp, c_vp, c_vp]),
    "tda_eeg_window_batch_dev": (_I, [c_vp, c_vp, _I, _I, _I, _D, c_vp, c_vp, c_vp, _I, c_vp, c_vp, _I, c_vp, c_vp, c_vp]),
    "tda_eeg_window_sliding_dev": (_I, [c_vp, c_vp, _I, _I, _I, _I, _I, c_vp, _I, _D, c_vp, c_vp, c_vp, _I, c_vp, c_vp, _I,
                                        c_vp, c_vp, c_vp, c_vp]),
    "tda_rips_dm_batch": (_I, [c_vp, c_vp, _I, _I, _D, _I, c_vp, _I, c_vp, c_vp, _I, c_vp, c_vp]),
    "tda_takens_rips_batch_dev": (_I, [c_vp, c_vp, c_vp, _I, _I, _I, _I, _D, c_vp, _I, c_vp, c_vp, _I, c_vp,
                                       c_vp, c_vp, c_vp]),
    "tda_takens_rips_batch": (_I, [c_vp, c_vp, c_vp, _I, _I, _I, _I, _D, c_vp, _I, c_vp, c_vp, _I, c_vp,
                                   c_vp, c_vp]),
    "tda_cloud_rips_batch_dev": (_I, [c_vp, c_vp, c_vp, _I, _I, _I, _I, _D, c_vp, _I, c_vp, c_vp, _I, c_vp,
                                      c_vp, c_vp]),
    "tda_cloud_rips_batch": (_I, [c_vp, c_vp, c_vp, _I, _I, _I, _I, _D, c_vp, _I, c_vp, c_vp, _I, c_vp, c_vp]),
    "tda_sosfiltfilt_dev": (_I, [c_vp, c_vp, _I, _I, c_vp, c_vp, _I, _I, c_vp, c_vp, c_vp]),
    "tda_sosfiltfilt": (_I, [c_vp, c_vp, _I, _I, c_vp, c_vp, _I, _I, c_vp]),
    "tda_filtfilt_dev": (_I, [c_vp, c_vp, _I, _I, c_vp, c_vp, c_vp, _I, _I, c_vp, c_vp, c_vp]),
    "tda_filtfilt": (_I, [c_vp, c_vp, _I, _I, c_vp, c_vp, c_vp, _I, _I, c_vp]),
    "tda_sosfiltfilt_bank_dev": (_I, [c_vp, c_vp, _I, _I, c_vp, c_vp, _I, _I, _I, c_vp, c_vp, c_vp]),
    "tda_filtfilt_bank_dev": (_I, [c_vp, c_vp, _I, _I, c_vp, c_vp, c_vp, _I, _I, _I, c_vp, c_vp, c_vp]),
    "tda_sosfiltfilt_bank_ragged_dev": (_I, [c_vp, c_vp, _I, _I, c_vp, c_vp, c_vp, c_vp, c_vp, _I, _I, _I, c_vp, c_vp, c_vp]),
    "tda_filtfilt_bank_ragged_dev": (_I, [c_vp, c_vp, _I, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, _I, _I, _I, c_vp, c_vp, c_vp]),
    "tda_gather_windows_dev": (_I, [c_vp, c_vp, c_vp, _I, _I, c_vp, c_vp]),
    "tda_eeg_window_ragged_dev": (_I, [c_vp, c_vp, c_vp, c_vp, _I, _I, _I, _D, c_vp, c_vp, c_vp, _I, c_vp, c_vp, _I, c_vp,
                                       c_vp, c_vp]),
    "tda_upfirdn_dev": (_I, [c_vp, c_vp, C.c_longlong, c_vp, _I, _I, _I, C.c_longlong, C.c_longlong, c_vp, c_vp]),
    "tda_upfirdn": (_I, [c_vp, c_vp, C.c_longlong, c_vp, _I, _I, _I, C.c_longlong, C.c_longlong, c_vp]),
    "tda_hilbert_envelope_dev": (_I, [c_vp, c_vp, _I, c_vp, c_vp, c_vp]),
    "tda_hilbert_envelope": (_I, [c_vp, c_vp, _I, c_vp, c_vp]),
    "tda_resample_poly_ragged_dev": (_I, [c_vp, c_vp, _I, c_vp, c_vp, c_vp, c_vp, c_vp, _I, _I, _I, _I, c_vp, c_vp]),
    "tda_hilbert_envelope_ragged_dev": (_I, [c_vp, c_vp, _I, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "tda_tau_batch_dev": (_I, [c_vp, c_vp, _I, _I, _I, c_vp, c_vp]),
    "tda_tau_segments_dev": (_I, [c_vp, c_vp, c_vp, _I, _I, _I, c_vp, c_vp, c_vp]),
    "tda_ami_batch_dev": (_I, [c_vp, c_vp, _I, _I, _I, _I, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "tda_ami_batch": (_I, [c_vp, c_vp, _I, _I, _I, _I, c_vp, c_vp, c_vp, c_vp]),
    "tda_ami_segments_dev": (_I, [c_vp, c_vp, c_vp, _I, _I, _I, _I, c_vp, c_vp, c_vp]),
    "tda_fnn_batch_dev": (_I, [c_vp, c_vp, c_vp, _I, _I, _I, _I, _D, _D, _D, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "tda_fnn_batch": (_I, [c_vp, c_vp, c_vp, _I, _I, _I, _I, _D, _D, _D, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "tda_recording_rows_dev": (_I, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, _I, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "tda_set_retry_policy": (_I, [c_vp, _I]),
    "tda_set_retry_counter": (_I, [c_vp, c_vp]),
    "tda_set_h1_order": (_I, [c_vp, _I]),
    "tda_set_launch_scheme": (_I, [c_vp, _I]),
    "tda_set_wasserstein_pruning": (_I, [c_vp, _I]),
    "tda_set_wasserstein_counter": (_I, [c_vp, c_vp]),
    "tda_diagram_finish_dev": (_I, [c_vp, c_vp, _I, _I, c_vp]),
    "tda_tau_batch": (_I, [c_vp, c_vp, _I, _I, _I, c_vp]),
    "tda_features_batch_dev": (_I, [c_vp, c_vp, c_vp, _I, _I, c_vp, c_vp]),
    "tda_features_batch": (_I, [c_vp, c_vp, c_vp, _I, _I, c_vp]),
    "tda_aggregate_batch_dev": (_I, [c_vp, c_vp, c_vp, c_vp, _I, c_vp, c_vp]),
    "tda_aggregate_batch": (_I, [c_vp, c_vp, c_vp, c_vp, _I, _I, c_vp]),
    "tda_segment_nanmean_dev": (_I, [c_vp, c_vp, c_vp, _I, c_vp, c_vp]),
    "tda_segment_nanmean": (_I, [c_vp, c_vp, c_vp, _I, _I, c_vp]),
    "tda_spearman_batch_dev": (_I, [c_vp, c_vp, c_vp, _I, c_vp, _I, c_vp, _I, c_vp, c_vp]),
    "tda_spearman_batch": (_I, [c_vp, c_vp, c_vp, _I, _I, c_vp, _I, c_vp, _I, c_vp]),
    "tda_temporal_corr_dev": (_I, [c_vp, c_vp, c_vp, _I, c_vp, _I, c_vp, _I, c_vp, c_vp, c_vp]),
    "tda_temporal_corr_batch": (_I, [c_vp, c_vp, c_vp, _I, _I, c_vp, _I, c_vp, _I, c_vp, c_vp]),
    "tda_wasserstein_batch_dev": (_I, [c_vp, c_vp, c_vp, _I, c_vp, c_vp, _I, c_vp, c_vp, _I, c_vp, c_vp, c_vp]),
    "tda_wasserstein_cross_dev": (_I, [c_vp, c_vp, c_vp, _I, _I, c_vp, c_vp, _I, c_vp, c_vp, _I, _I, c_vp, _I, c_vp, c_vp,
                                       c_vp, c_vp, c_vp]),
    "tda_cross_rows_dev": (_I, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, _I, c_vp, c_vp, c_vp, c_vp]),
    "tda_wasserstein_matrix_dev": (_I, [c_vp, c_vp, c_vp, _I, _I, c_vp, _I, c_vp, c_vp, c_vp, _I, _I, c_vp, _I, _I, c_vp,
                                        c_vp, c_vp, c_vp, c_vp]),
    "tda_match_rows_dev": (_I, [c_vp, c_vp, c_vp, c_vp, _I, _I, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "tda_wasserstein_batch": (_I, [c_vp, c_vp, c_vp, _I, _I, c_vp, c_vp, _I, _I, c_vp, c_vp, _I, c_vp, c_vp]),
    "tda_bottleneck_batch_dev": (_I, [c_vp, c_vp, c_vp, _I, c_vp, c_vp, _I, c_vp, c_vp, _I, c_vp, c_vp, c_vp]),
    "tda_bottleneck_batch": (_I, [c_vp, c_vp, c_vp, _I, _I, c_vp, c_vp, _I, _I, c_vp, c_vp, _I, c_vp, c_vp]),
    "tda_wasserstein_q_batch_dev": (_I, [c_vp, c_vp, c_vp, _I, c_vp, c_vp, _I, c_vp, c_vp, _I, _I, _I, c_vp, c_vp, c_vp]),
    "tda_wasserstein_q_batch": (_I, [c_vp, c_vp, c_vp, _I, _I, c_vp, c_vp, _I, _I, c_vp, c_vp, _I, _I, _I, c_vp, c_vp]),
    "tda_sliced_wasserstein_batch_dev": (_I, [c_vp, c_vp, c_vp, _I, c_vp, c_vp, _I, c_vp, c_vp, _I, c_vp, _I, c_vp, c_vp,
                                              c_vp]),
    "tda_sliced_wasserstein_batch": (_I, [c_vp, c_vp, c_vp, _I, _I, c_vp, c_vp, _I, _I, c_vp, c_vp, _I, c_vp, _I, c_vp,
                                          c_vp]),
    "tda_sliced_prepare_dev": (_I, [c_vp, c_vp, c_vp, _I, _I, c_vp, _I, c_vp, c_vp, C.c_longlong, c_vp, c_vp]),
    "tda_sliced_prepared_pairs_dev": (_I, [c_vp, c_vp, c_vp, c_vp, _I, c_vp, c_vp, c_vp, _I, c_vp, c_vp, _I, _I, c_vp, c_vp,
                                           c_vp]),
    "tda_sliced_matrix_dev": (_I, [c_vp, c_vp, c_vp, c_vp, _I, c_vp, _I, c_vp, c_vp, c_vp, c_vp, _I, c_vp, _I, _I, c_vp, _I,
                                   c_vp, c_vp, c_vp, c_vp]),
    "tda_landscape_mean_dev": (_I, [c_vp, c_vp, c_vp, _I, _I, c_vp, _I, c_vp, _I, c_vp, _I, _I, c_vp, c_vp]),
    "tda_landscape_batch": (_I, [c_vp, c_vp, c_vp, _I, _I, c_vp, _I, _I, c_vp]),
    "tda_euler_dm_batch_dev": (_I, [c_vp, c_vp, _I, _I, _D, _I, c_vp, _I, _I, c_vp, c_vp, c_vp]),
    "tda_euler_dm_batch": (_I, [c_vp, c_vp, _I, _I, _D, _I, c_vp, _I, _I, c_vp, c_vp]),
    "tda_euler_cloud_batch_dev": (_I, [c_vp, c_vp, c_vp, _I, _I, _I, _I, _D, c_vp, _I, _I, c_vp, c_vp, c_vp]),
    "tda_euler_cloud_batch": (_I, [c_vp, c_vp, c_vp, _I, _I, _I, _I, _D, c_vp, _I, _I, c_vp, c_vp]),
    "tda_euler_takens_batch_dev": (_I, [c_vp, c_vp, c_vp, _I, _I, _I, _I, _D, c_vp, _I, _I, c_vp, c_vp, c_vp, c_vp]),
    "tda_euler_takens_batch": (_I, [c_vp, c_vp, c_vp, _I, _I, _I, _I, _D, c_vp, _I, _I, c_vp, c_vp, c_vp]),
    "tda_euler_mean_dev": (_I, [c_vp, c_vp, _I, _I, _I, c_vp, _I, c_vp, _I, c_vp, c_vp]),
    "tda_euler_mean": (_I, [c_vp, c_vp, _I, _I, _I, c_vp, _I, c_vp, _I, c_vp]),
    "tda_network_dm_batch_dev": (_I, [c_vp, c_vp, _I, _I, _D, _I, c_vp, _I, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "tda_network_dm_batch": (_I, [c_vp, c_vp, _I, _I, _D, _I, c_vp, _I, c_vp, c_vp, c_vp, c_vp]),
    "tda_network_cloud_batch_dev": (_I, [c_vp, c_vp, c_vp, _I, _I, _I, _I, _D, c_vp, _I, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "tda_network_cloud_batch": (_I, [c_vp, c_vp, c_vp, _I, _I, _I, _I, _D, c_vp, _I, c_vp, c_vp, c_vp, c_vp]),
    "tda_network_takens_batch_dev": (_I, [c_vp, c_vp, c_vp, _I, _I, _I, _I, _D, c_vp, _I, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "tda_network_takens_batch": (_I, [c_vp, c_vp, c_vp, _I, _I, _I, _I, _D, c_vp, _I, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "tda_network_mean_dev": (_I, [c_vp, c_vp, c_vp, c_vp, _I, _I, _I, c_vp, _I, c_vp, _I, c_vp, c_vp, c_vp, c_vp]),
    "tda_network_mean": (_I, [c_vp, c_vp, c_vp, c_vp, _I, _I, _I, c_vp, _I, c_vp, _I, c_vp, c_vp, c_vp]),
    "tda_recurrence_dm_batch_dev": (_I, [c_vp, c_vp, _I, _I, _D, _I, c_vp, _I] + _RQ + [c_vp, c_vp]),
    "tda_recurrence_dm_batch": (_I, [c_vp, c_vp, _I, _I, _D, _I, c_vp, _I] + _RQ + [c_vp]),
    "tda_recurrence_cloud_batch_dev": (_I, [c_vp, c_vp, c_vp, _I, _I, _I, _I, _D, c_vp, _I] + _RQ + [c_vp, c_vp]),
    "tda_recurrence_cloud_batch": (_I, [c_vp, c_vp, c_vp, _I, _I, _I, _I, _D, c_vp, _I] + _RQ + [c_vp]),
    "tda_recurrence_takens_batch_dev": (_I, [c_vp, c_vp, c_vp, _I, _I, _I, _I, _D, c_vp, _I] + _RQ + [c_vp, c_vp, c_vp]),
    "tda_recurrence_takens_batch": (_I, [c_vp, c_vp, c_vp, _I, _I, _I, _I, _D, c_vp, _I] + _RQ + [c_vp, c_vp]),
    "tda_recurrence_mean_dev": (_I, [c_vp, c_vp, c_vp, c_vp, _I, _I, _I, c_vp, _I, c_vp, _I, c_vp, c_vp, c_vp, c_vp]),
    "tda_recurrence_mean": (_I, [c_vp, c_vp, c_vp, c_vp, _I, _I, _I, c_vp, _I, c_vp, _I, c_vp, c_vp, c_vp]),
    "tda_generators_dm_batch_dev": (_I, [c_vp, c_vp, _I, _I, _D, _I] + _GEN + [c_vp, c_vp]),
    "tda_generators_dm_batch": (_I, [c_vp, c_vp, _I, _I, _D, _I] + _GEN + [c_vp]),
    "tda_generators_cloud_batch_dev": (_I, [c_vp, c_vp, c_vp, _I, _I, _I, _I, _D] + _GEN + [c_vp, c_vp]),
    "tda_generators_cloud_batch": (_I, [c_vp, c_vp, c_vp, _I, _I, _I, _I, _D] + _GEN + [c_vp]),
    "tda_generators_takens_batch_dev": (_I, [c_vp, c_vp, c_vp, _I, _I, _I, _I, _D] + _GEN + [c_vp, c_vp, c_vp]),
    "tda_generators_takens_batch": (_I, [c_vp, c_vp, c_vp, _I, _I, _I, _I, _D] + _GEN + [c_vp, c_vp]),
    "tda_generators_mean_dev": (_I, [c_vp, c_vp, _I, _I, c_vp, _I, c_vp, _I, c_vp, c_vp]),
    "tda_generators_mean": (_I, [c_vp, c_vp, _I, _I, c_vp, _I, c_vp, _I, c_vp]),
    "tda_image_mean_dev": (_I, [c_vp, c_vp, c_vp, _I, _I, c_vp, _I, c_vp, _I, c_vp, _I, c_vp, _I, _D, _I, c_vp, c_vp]),
    "tda_image_batch": (_I, [c_vp, c_vp, c_vp, _I, _I, c_vp, _I, c_vp, _I, _D, _I, c_vp]),
    "tda_frechet_mean_dev": (_I, [c_vp, c_vp, c_vp, _I, _I, c_vp, _I, c_vp, _I, _I, c_vp, c_vp, _I, c_vp, c_vp, c_vp, c_vp]),
    "tda_frechet_mean_batch": (_I, [c_vp, c_vp, c_vp, _I, _I, c_vp, _I, c_vp, _I, _I, c_vp, c_vp, _I, c_vp, c_vp, c_vp]),
    "tda_diagram_kernel_pairs_dev": (_I, [c_vp, c_vp, c_vp, _I, _I, c_vp, c_vp, _I, _I, c_vp, c_vp, _I, _D, _I, _D, _I, _D, c_vp,
                                          c_vp, c_vp, c_vp]),
    "tda_diagram_kernel_pairs": (_I, [c_vp, c_vp, c_vp, _I, _I, c_vp, c_vp, _I, _I, c_vp, c_vp, _I, _D, _I, _D, _I, _D, c_vp, c_vp,
                                      c_vp]),
    "tda_diagram_kernel_gram_dev": (_I, [c_vp, c_vp, c_vp, _I, _I, c_vp, _I, c_vp, c_vp, c_vp, _I, _I, c_vp, _I, c_vp, _I, _D, _I,
                                         _D, _I, _D, c_vp, c_vp]),
    "tda_diagram_kernel_gram": (_I, [c_vp, c_vp, c_vp, _I, _I, c_vp, _I, c_vp, c_vp, c_vp, _I, _I, c_vp, _I, c_vp, _I, _D, _I, _D,
                                     _I, _D, c_vp]),
    "tda_persistence_fisher_batch_dev": (_I, [c_vp, c_vp, c_vp, _I, _I, c_vp, c_vp, _I, _I, c_vp, c_vp, _I, _D, c_vp, c_vp, c_vp]),
    "tda_persistence_fisher_batch": (_I, [c_vp, c_vp, c_vp, _I, _I, c_vp, c_vp, _I, _I, c_vp, c_vp, _I, _D, c_vp, c_vp]),
    "tda_takens_landmarks_dev": (_I, [c_vp, c_vp, c_vp, _I, _I, _I, _I, _I, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "tda_takens_landmarks": (_I, [c_vp, c_vp, c_vp, _I, _I, _I, _I, _I, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "tda_cloud_landmarks_dev": (_I, [c_vp, c_vp, c_vp, _I, _I, _I, _I, _I, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "tda_cloud_landmarks": (_I, [c_vp, c_vp, c_vp, _I, _I, _I, _I, _I, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "tda_takens_rips_landmarks_dev": (_I, [c_vp, c_vp, c_vp, _I, _I, _I, _I, _I, _D, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                           c_vp, _I, c_vp, c_vp, _I, c_vp, c_vp, c_vp, c_vp]),
    "tda_takens_rips_landmarks": (_I, [c_vp, c_vp, c_vp, _I, _I, _I, _I, _I, _D, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                       c_vp, _I, c_vp, c_vp, _I, c_vp, c_vp, c_vp]),
    "tda_sublevel_batch_dev": (_I, [c_vp, c_vp, c_vp, c_vp, _I, _I, _I, c_vp, _I, c_vp, c_vp, c_vp, c_vp]),
    "tda_sublevel_batch": (_I, [c_vp, c_vp, c_vp, c_vp, _I, _I, _I, c_vp, _I, c_vp, c_vp, c_vp]),
    "tda_plv_dist_batch_dev": (_I, [c_vp, c_vp, c_vp, c_vp, _I, _I, _I, c_vp, _I, c_vp, c_vp, c_vp, c_vp]),
    "tda_plv_dist_batch": (_I, [c_vp, c_vp, c_vp, c_vp, _I, _I, _I, c_vp, _I, c_vp, c_vp, c_vp]),
    "tda_connectivity_dist_batch_dev": (_I, [c_vp, c_vp, c_vp, c_vp, _I, _I, _I, c_vp, _I, _I, c_vp, c_vp, c_vp, c_vp]),
    "tda_connectivity_dist_batch": (_I, [c_vp, c_vp, c_vp, c_vp, _I, _I, _I, c_vp, _I, _I, c_vp, c_vp, c_vp]),
    "tda_perm_sums_batch_dev": (_I, [c_vp, c_vp, _I, _I, _I, c_vp, _I, c_vp, C.c_longlong, c_vp, c_vp, c_vp]),
    "tda_perm_sums_batch": (_I, [c_vp, c_vp, _I, _I, _I, c_vp, _I, c_vp, c_vp]),
    "tda_event_create": (_I, [c_vp, C.POINTER(c_vp)]),
    "tda_event_record": (_I, [c_vp, c_vp, c_vp]),
    "tda_event_elapsed_ms": (_I, [c_vp, c_vp, c_vp, C.POINTER(C.c_float)]),
    "tda_event_destroy": (_I, [c_vp, c_vp]),
    "tda_set_kernel_probe": (_I, [c_vp, _I, c_vp, c_vp, c_vp]),
    "tda_stream_sync": (_I, [c_vp, c_vp]),
}

class DiagramSet(C.Structure):
    """tda_diagram_set of include/tdaeeg.h."""
    _fields_ = [("rows", c_vp), ("cnt", c_vp), ("cap", _I), ("order", _I), ("feat", c_vp)]


_lib = None


class TdaError(RuntimeError):
    pass


def load():
    """dlopen libtdaeeg.so.  torch (if importable) is imported first so that both share ONE HIP
    runtime (both link libamdhip64.so.7; the first one loaded wins)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise TdaError(
            f"{LIB_PATH} is missing: build the HIP extension first "
            "(python -c 'import __graft_entry__ as g; g.build()').  There is no CPU fallback.")
    try:
        import torch  # noqa: F401  (loads torch's bundled HIP runtime first)
    except Exception:
        pass
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)   # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


class Context:
    """One per process and GPU (tda_ctx)."""

    def __init__(self, device=0):
        self.lib = load()
        h = c_vp()
        rc = self.lib.tda_ctx_create(int(device), C.byref(h))
        if rc != 0:
            buf = C.create_string_buffer(512)
            self.lib.tda_last_error(None, buf, 512)
            raise TdaError(f"tda_ctx_create(device={device}) failed ({rc}): {buf.value.decode()} "
                           "-- the HIP path needs a visible MI355X; there is no CPU fallback")
        self.h = h
        self.device = int(device)
        # first-pass class capacity (x64 bits) of the Rips kernels, e.g. TDA_CLASS_WORDS=1,1 (dm, cloud)
        cw = os.environ.get("TDA_CLASS_WORDS")
        if cw:
            dm, cloud = (int(x) for x in cw.split(","))
            self.set_class_words(dm, cloud)

    def check(self, rc):
        if rc != 0:
            buf = C.create_string_buffer(1024)
            self.lib.tda_last_error(self.h, buf, 1024)
            raise TdaError(f"libtdaeeg error {rc}: {buf.value.decode()}")

    def set_class_words(self, words_dm=2, words_cloud=1):
        self.check(self.lib.tda_set_class_words(self.h, words_dm, words_cloud))

    RETRY_AUTO, RETRY_FIRST_PASS, RETRY_ONLY, RETRY_ONE_STEP, RETRY_LAST_RUNG = 0, 1, 2, 3, 4

    retry_policy = 0          # the policy last set here (RETRY_AUTO is the library's default): callers save and put it back

    def set_retry_policy(self, policy):
        self.check(self.lib.tda_set_retry_policy(self.h, int(policy)))
        self.retry_policy = int(policy)

    ORDER_IN_CALL, ORDER_DEFERRED = 0, 1

    def set_h1_order(self, policy):
        self.check(self.lib.tda_set_h1_order(self.h, int(policy)))

    @contextlib.contextmanager
    def deferred(self, retry="auto"):
        """The policies of a batched step for the Rips calls inside the block: ORDER_DEFERRED (the caller runs ONE finishing
        pass afterwards) and, for retry="first" / "one", RETRY_FIRST_PASS / RETRY_ONE_STEP (pipeline.run_step).  ORDER_IN_CALL
        and RETRY_AUTO are back when the block is left, also by an exception."""
        if retry != "auto":
            self.set_retry_policy(self.RETRY_FIRST_PASS if retry == "first" else self.RETRY_ONE_STEP)
        self.set_h1_order(self.ORDER_DEFERRED)
        try:
            yield self
        finally:
            self.set_h1_order(self.ORDER_IN_CALL)
            if retry != "auto":
                self.set_retry_policy(self.RETRY_AUTO)

    SCHEME_LISTS, SCHEME_GRID, SCHEME_ONE = 0, 1, 2

    def set_launch_scheme(self, scheme):
        """How the finishing pass and the Wasserstein launches split their work (include/tdaeeg.h); results do not change."""
        self.check(self.lib.tda_set_launch_scheme(self.h, int(scheme)))

    def set_wasserstein_pruning(self, on=True):
        """Leave out the Wasserstein work whose result is known in advance (include/tdaeeg.h); results do not change."""
        self.check(self.lib.tda_set_wasserstein_pruning(self.h, 1 if on else 0))

    def set_wasserstein_counter(self, dev_ptr):
        """dev_ptr: device address of a zeroed u64[3] (or None): short cuts, rows + columns trimmed, pairs solved."""
        self.check(self.lib.tda_set_wasserstein_counter(self.h, c_vp(dev_ptr) if dev_ptr else None))

    def set_retry_counter(self, dev_ptr):
        """dev_ptr: device address of a zeroed u64[4] (or None): windows redone by the widening passes."""
        self.check(self.lib.tda_set_retry_counter(self.h, c_vp(dev_ptr) if dev_ptr else None))

    # ---- one-shot kernel probe (bench.py roofline): HIP events around ONE first-pass kernel ----
    PROBES = {"rips_audio": 1, "rips_eeg": 2, "corr_dist": 3}

    def new_event(self):
        ev = c_vp()
        self.check(self.lib.tda_event_create(self.h, C.byref(ev)))
        return ev

    def arm_probe(self, stage, ev_start=None, ev_stop=None, dev_span=None):
        """dev_span: optional device pointer (int) to a zeroed u64[4] (rips_audio only): the kernel
        accumulates its own duration there (see include/tdaeeg.h); events may be omitted then."""
        self.check(self.lib.tda_set_kernel_probe(self.h, self.PROBES[stage], ev_start, ev_stop,
                                                 c_vp(dev_span) if dev_span else None))

    def elapsed_ms(self, ev_start, ev_stop):
        ms = C.c_float()
        self.check(self.lib.tda_event_elapsed_ms(self.h, ev_start, ev_stop, C.byref(ms)))
        return float(ms.value)

    def close(self):
        if getattr(self, "h", None):
            self.lib.tda_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_ctx = {}


def get_ctx(device=None):
    if device is None:
        device = int(os.environ.get("TDA_DEVICE", os.environ.get("LOCAL_RANK", "0")))
        try:
            import torch
            if torch.cuda.is_available():
                device = torch.cuda.current_device()
        except Exception:
            pass
    if device not in _ctx:
        _ctx[device] = Context(device)
    return _ctx[device]


def ptr(a):
    """void* of a C-contiguous numpy array (or None)."""
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(c_vp)


def f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)
