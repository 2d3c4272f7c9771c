/*
 * tdaeeg.h -- C ABI of libtdaeeg.so: the MI355X (gfx950) persistent-homology
 * feature engine for the per-window hot path of Ignaciagothe/tda-eeg-audio.
 *
 * The reference has no FFI: its boundary is the Python call level (SURVEY.md
 * section 8b).  Each entry point below names the reference call it replaces
 * (paths relative to the reference tree; notebooks cited by raw .ipynb JSON line).
 *
 * Conventions
 *   * Plain C, no torch / HIP types in signatures.  `stream` is a hipStream_t
 *     passed as void* (NULL = the default stream).
 *   * `*_dev` entry points take DEVICE pointers, enqueue on `stream` and return
 *     without synchronising (safe to capture in a hipGraph).  The un-suffixed
 *     twins take HOST pointers, stage through the context's device workspace and
 *     synchronise before returning.
 *   * Every function returns a tda_status (0 = ok); nothing throws or aborts.
 *     Per-window problems are reported in the `status` arrays (bit flags below),
 *     never silently.
 *   * The library keeps no pointer after a call returns and never writes inputs.
 *   * Persistence diagrams are rows of (birth, death) float64 holding float32-exact
 *     values (what ripser returns), +inf for essential classes.
 *       H0: finite rows in ascending death order, then one (0,+inf) per component.
 *       H1: rows in descending birth order (ripser's column order).
 */
#ifndef TDAEEG_H
#define TDAEEG_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tda_ctx tda_ctx;

typedef enum {
    TDA_OK = 0,
    TDA_ERR_INVALID = 1,      /* bad argument (null pointer, size out of range) */
    TDA_ERR_HIP = 2,          /* a HIP runtime call failed; see tda_last_error */
    TDA_ERR_UNSUPPORTED = 3,  /* size outside what the kernels implement        */
    TDA_ERR_NOMEM = 4
} tda_status;

/* per-window status bits written by the kernels */
#define TDA_WIN_OK            0
#define TDA_WIN_H1_TRUNCATED  1   /* more H1 rows than h1_cap; count holds the true number    */
#define TDA_WIN_CLASS_OVERFLOW 2  /* more simultaneously alive H1 classes than the kernel's
                                     class capacity (tda_set_class_words); diagrams invalid   */
#define TDA_WIN_DEGENERATE    4   /* point cloud with < 3 points: diagrams are [[0,0]],[[0,0]]
                                     exactly as scripts/utils.py:125-126                      */
#define TDA_WIN_NOT_CONVERGED 8   /* assignment solver hit its iteration bound (-> NaN)        */
#define TDA_WIN_TOO_LARGE     16  /* more than TDA_MAX_POINTS points (tau < 1?): no diagram    */
#define TDA_WIN_NO_PAIR       32  /* tda_wasserstein_cross_dev: this diagram has no partner at
                                     its position (mvm:89); the distance is NaN and is no member of the group's mean */
#define TDA_WIN_NOT_FINITE    64  /* tda_sublevel_batch: the signal has a sample that is not finite; count 0, no rows
                                     tda_plv_dist_batch, tda_connectivity_dist_batch: the same for a window; its plv / value
                                     and dist blocks are NaN */

#define TDA_N_FEATURES 11         /* scripts/utils.py:166-177 key order */
#define TDA_MAX_POINTS 128        /* vertices per Rips complex (reference needs <= 124)        */
#define TDA_MAX_DIM    4          /* Takens embedding dimension (reference uses 3)             */

int  tda_version(void);

/* Context: owns the HIP device binding, a stream-ordered workspace and the error
 * string.  One per process and GPU (the reference's joblib workers, v2:569-572,
 * become one process per GPU). */
tda_status tda_ctx_create(int device_id, tda_ctx** out);
void       tda_ctx_destroy(tda_ctx* ctx);
/* Copies the last error message of this context (or of the failed create when
 * ctx == NULL) into buf; returns its length. */
size_t     tda_last_error(const tda_ctx* ctx, char* buf, size_t cap);
/* First-pass capacity for simultaneously alive H1 classes.  words_dm in {0,1,2,4}: 64 * words bits for distance-matrix
 * input; 0 = 32 bits, honoured by the fused EEG window kernel only (tda_rips_dm_batch treats it as 1).  words_cloud in
 * {1,2}: 32 or 64 bits for point clouds.  Defaults: 2 and 1.  Windows that need more are redone by the widening passes
 * (tda_set_retry_policy), so the setting changes speed, never results. */
tda_status tda_set_class_words(tda_ctx* ctx, int words_dm, int words_cloud);
/* How the Rips entry points treat windows that run out of class bits (TDA_WIN_CLASS_OVERFLOW).
 * AUTO (default): every call launches its widening passes after the first pass; they redo only the flagged
 *   windows, but each is a launch that needs (large) CU resources even when nothing is flagged.
 * FIRST_PASS: only the first pass is launched; flagged windows keep the status bit and invalid rows.  A
 *   streaming caller checks the statuses once they have reached the host and, if any is set, calls the same
 *   entry point again on the same buffers under RETRY_ONLY (then recomputes what depends on the diagrams).
 * RETRY_ONLY: only the widening passes (and the row ordering) are launched.
 * ONE_STEP: the first pass and ONE widening pass (the next rung of the ladder: 128 bits for matrices, 64 for
 *   clouds), which catches nearly every flagged window and still fits beside the other kernels of a busy GPU; the
 *   wide rungs (up to 95 KB of LDS and 256 VGPRs per workgroup, which wait for a nearly empty CU even when they have
 *   nothing to redo) are left to a later RETRY_ONLY call for the batches whose statuses still carry the bit.
 * The ladders end in a pass that keeps the class vectors in HBM and has no capacity limit (8,192 classes cover every
 * complex on 128 points): under AUTO and RETRY_ONLY no window keeps TDA_WIN_CLASS_OVERFLOW, as ripser never refuses an
 * input.  LAST_RUNG launches only that pass (on the flagged windows). */
#define TDA_RETRY_AUTO       0
#define TDA_RETRY_FIRST_PASS 1
#define TDA_RETRY_ONLY       2
#define TDA_RETRY_ONE_STEP   3
#define TDA_RETRY_LAST_RUNG  4   /* only the last rung (class vectors in HBM) on the flagged windows: for tests */
tda_status tda_set_retry_policy(tda_ctx* ctx, int policy);
/* Optional accounting of the widening passes: dev_counters = DEVICE u64[4] (or NULL to stop).  Every window a
 * widening pass redoes adds one to [0] (distance-matrix input, tda_rips_dm_batch) or [1] (point clouds,
 * tda_takens_rips_batch / tda_cloud_rips_batch); a window that climbs two rungs of the ladder counts twice; [2] counts
 * the windows redone by the last rung (class vectors in HBM, no capacity limit).
 * The reference has no counterpart (ripser's columns grow on the heap); bench.py reports it as windows_repaired. */
tda_status tda_set_retry_counter(tda_ctx* ctx, void* dev_counters);

/* ---- corr -> distance ------------------------------------------------------
 * replaces compute_correlation_matrix + correlation_to_distance(method="euclidean")
 * (notebooks/2_graph_construction.ipynb:86-122) and the per-window loop of
 * process_file_graphs (nb2:198-207).
 * win  : (n_win, n_ch, n_t) float64, C order   (preprocessed/<cond>/<rec>/<band>.npy)
 * dist : (n_win, n_ch, n_ch) float64           (<band>_distances.npy)
 * corr : same shape or NULL                    (<band>_correlations.npy)            */
tda_status tda_corr_dist_batch_dev(tda_ctx* ctx, const double* win, int n_win, int n_ch, int n_t,
                                   double* dist, double* corr, void* stream);
tda_status tda_corr_dist_batch(tda_ctx* ctx, const double* win, int n_win, int n_ch, int n_t,
                               double* dist, double* corr);

/* Sliding windows fused in: create_sliding_windows (notebooks/1_preprocesamiento.ipynb:314-381;
 * window w = samples [w*step, w*step+win_len), n_win = (n_samples-win_len)/step+1) followed by the
 * per-window corr->dist above, reading the overlapping windows straight from ONE band-passed
 * recording sig (n_ch, n_samples) float64 -- the (n_win, n_ch, win_len) stack (4x the bytes at 75 %
 * overlap) is never materialised.  dist/corr: (n_win, n_ch, n_ch); n_win (out, nullable).      */
tda_status tda_corr_dist_sliding_dev(tda_ctx* ctx, const double* sig, int n_ch, int n_samples,
                                     int win_len, int step, double* dist, double* corr, int* n_win,
                                     void* stream);
tda_status tda_corr_dist_sliding(tda_ctx* ctx, const double* sig, int n_ch, int n_samples,
                                 int win_len, int step, double* dist, double* corr, int* n_win);

/* correlation_to_distance (nb2:100-122) alone, on stored correlation matrices.
 * method: 0 "euclidean" (the only one the reference calls, nb2:227,304,312), 1 "abs",
 *         2 "standard", 3 "sqrt" (nb2:109-116).  corr, dist: (n_win, n, n) float64.          */
tda_status tda_corr_to_dist_batch_dev(tda_ctx* ctx, const double* corr, int n_win, int n, int method,
                                      double* dist, void* stream);
tda_status tda_corr_to_dist_batch(tda_ctx* ctx, const double* corr, int n_win, int n, int method,
                                  double* dist);

/* ---- Vietoris-Rips H0/H1 from distance matrices -----------------------------
 * replaces compute_eeg_persistence (scripts/utils.py:135-141) ==
 * compute_persistence_diagram (scripts/tda_eeg_classification_v2.py:143-176):
 * ripser(dm, maxdim=1, thresh, distance_matrix=True)["dgms"].
 * dm        : (n_win, n, n) float64, n <= TDA_MAX_POINTS
 * symmetrise: 1 = apply (D+D^T)/2, diag 0, max(.,0) first (utils.py:137-139);
 *             0 = use entries (i,j), i<j, as ripser.py does on a raw matrix
 * h0        : (n_win, h0_cap, 2) float64, h0_cap >= n;   h0_cnt: (n_win) int32
 * h1        : (n_win, h1_cap, 2) float64;                h1_cnt: (n_win) int32
 * status    : (n_win) int32 bit flags (TDA_WIN_*)                                    */
tda_status tda_rips_dm_batch_dev(tda_ctx* ctx, const double* dm, int n_win, int n, double thresh,
                                 int symmetrise, double* h0, int h0_cap, int* h0_cnt,
                                 double* h1, int h1_cap, int* h1_cnt, int* status, void* stream);
tda_status tda_rips_dm_batch(tda_ctx* ctx, const double* dm, int n_win, int n, double thresh,
                             int symmetrise, double* h0, int h0_cap, int* h0_cnt,
                             double* h1, int h1_cap, int* h1_cnt, int* status);

/* ---- fused EEG window: samples -> correlation -> distance -> Rips H0/H1 in ONE launch -------------
 * replaces, per window, compute_correlation_matrix + correlation_to_distance (nb2:86-122; the loop of
 * process_file_graphs, nb2:198-207) followed by compute_eeg_persistence (scripts/utils.py:135-141): the distance
 * matrix stays in LDS, 95.1 KB of HBM traffic per window instead of 129.4.  Same arithmetic, operation for
 * operation, as tda_corr_dist_batch_dev + tda_rips_dm_batch_dev(symmetrise = 1): identical diagrams.  Its ladder of
 * class widths (32 / 64 -> 128 -> 512 bits in LDS) ends, like that of tda_rips_dm_batch_dev, in a pass without a
 * capacity limit (class vectors in HBM): 512 bits hold the 506 classes that 47 channels can have alive at once, not
 * the 529 of 48.  TDA_RETRY_LAST_RUNG runs that pass alone on the windows whose status carries
 * TDA_WIN_CLASS_OVERFLOW.
 * win: (n_win, n_ch, n_t) float64, 33 <= n_ch <= 48 (the reference has 47), 2 <= n_t <= 256 (250).
 * dist / corr (nullable; corr needs dist): the matrices as tda_corr_dist_batch writes them, for callers that also
 * want the graphs/<cond>/<rec>/<band>_distances.npy hand-off file.  Device pointers only. */
tda_status tda_eeg_window_batch_dev(tda_ctx* ctx, const double* win, int n_win, int n_ch, int n_t, double thresh,
                                    double* dist, double* corr, double* h0, int h0_cap, int* h0_cnt,
                                    double* h1, int h1_cap, int* h1_cnt, int* status, void* stream);

/* The same kernel on windows read IN PLACE from band-passed recordings of equal length (recordings of different
 * lengths: tda_eeg_window_ragged_dev below), sig: (n_rec, n_ch,
 * n_samples) float64 -- create_sliding_windows (notebooks/1_preprocesamiento.ipynb:314-381: window k of a recording =
 * samples [k*step, k*step + win_len), n_win_per_rec = (n_samples - win_len) / step + 1) + process_file_graphs
 * (nb2:198-207) + compute_eeg_persistence (utils.py:135-141) without ever materialising the (n_win, n_ch, win_len)
 * stack (4x the bytes at 75 % overlap; 43 GB for the corpus) or the matrices.  sel (nullable, n_sel entries): the
 * windows to process, as r * n_win_per_rec + k -- the drivers' window selection (v2:394-398, cmp:77-80); outputs
 * have n_sel rows then, otherwise n_rec * n_win_per_rec (recording-major).  n_win_per_rec (out, nullable, host). */
tda_status tda_eeg_window_sliding_dev(tda_ctx* ctx, const double* sig, int n_rec, int n_ch, int n_samples,
                                      int win_len, int step, const int* sel, int n_sel, double thresh,
                                      double* dist, double* corr, double* h0, int h0_cap, int* h0_cnt,
                                      double* h1, int h1_cap, int* h1_cnt, int* status, int* n_win_per_rec,
                                      void* stream);

/* The same kernel on windows of RAGGED recordings, read in place from a window table: recordings of different lengths
 * L_r are packed back to back (recording r is an (n_ch, L_r) row-major block at element n_ch * off[r], off the
 * exclusive prefix sum of L); output window w starts at element win_start[w] of sig and its rows are win_ld[w] = L_r
 * apart.  win_start / win_ld: device int64 (n_win), built once on the host -- create_sliding_windows
 * (notebooks/1_preprocesamiento.ipynb:314-381) of each recording at its own length + the window selection (cmp:77-80) +
 * nb2:198-207 + utils.py:135-141.  Diagrams identical to tda_eeg_window_batch_dev on the same windows stacked. */
tda_status tda_eeg_window_ragged_dev(tda_ctx* ctx, const double* sig, const long long* win_start,
                                     const long long* win_ld, int n_win, int n_ch, int win_len, double thresh,
                                     double* dist, double* corr, double* h0, int h0_cap, int* h0_cnt, double* h1,
                                     int h1_cap, int* h1_cnt, int* status, void* stream);

/* ---- Takens embedding + Rips (audio branch) ---------------------------------
 * replaces takens_embedding (scripts/utils.py:107-116) followed by
 * compute_audio_persistence (utils.py:123-132): per-column min-max to [0,1],
 * ripser(pc_norm, maxdim=1, thresh) whose point-cloud path is
 * sklearn.metrics.pairwise_distances -> float32.
 * win  : (n_win, n_t) float64 audio windows;  tau: (n_win) int32 delays
 * n_points (out, nullable): points per window, P = ceil((n_t-(dim-1)tau)/subsample)
 * Windows with P < 3 get [[0,0]],[[0,0]] and TDA_WIN_DEGENERATE (utils.py:125-126).  */
tda_status tda_takens_rips_batch_dev(tda_ctx* ctx, const double* win, const int* tau, int n_win,
                                     int n_t, int dim, int subsample, double thresh,
                                     double* h0, int h0_cap, int* h0_cnt,
                                     double* h1, int h1_cap, int* h1_cnt,
                                     int* n_points, int* status, void* stream);
tda_status tda_takens_rips_batch(tda_ctx* ctx, const double* win, const int* tau, int n_win,
                                 int n_t, int dim, int subsample, double thresh,
                                 double* h0, int h0_cap, int* h0_cnt,
                                 double* h1, int h1_cap, int* h1_cnt,
                                 int* n_points, int* status);

/* ---- Rips from explicit point clouds ----------------------------------------
 * replaces compute_audio_persistence(point_cloud) (utils.py:123-132) when the caller
 * already holds the (P, dim) cloud.  pc: (n_win, p_cap, dim) float64; n_pts: (n_win). */
tda_status tda_cloud_rips_batch_dev(tda_ctx* ctx, const double* pc, const int* n_pts, int n_win,
                                    int p_cap, int dim, int normalise, double thresh,
                                    double* h0, int h0_cap, int* h0_cnt,
                                    double* h1, int h1_cap, int* h1_cnt, int* status, void* stream);
tda_status tda_cloud_rips_batch(tda_ctx* ctx, const double* pc, const int* n_pts, int n_win,
                                int p_cap, int dim, int normalise, double thresh,
                                double* h0, int h0_cap, int* h0_cnt,
                                double* h1, int h1_cap, int* h1_cnt, int* status);

/* ---- zero-phase IIR filtering (front ends) ----------------------------
 * tda_sosfiltfilt replaces scipy.signal.sosfiltfilt(sos, x) as apply_bandpass_filter calls it per
 * EEG channel (notebooks/1_preprocesamiento.ipynb:236-263); tda_filtfilt replaces
 * scipy.signal.filtfilt(b, a, s) of bandpass_filter (scripts/utils.py:66-74).  Same algorithm as
 * scipy (odd extension by `edge`, forward from zi*x[0], backward from zi*y[-1], trim), same
 * operation order: bit-identical float64 results.  Filter design stays on the host:
 *   sos (n_sections,6) from scipy.signal.butter(..., output="sos"), zi (n_sections,2) from sosfilt_zi,
 *   edge = 3*(2*n_sections+1 - min(#b2==0, #a2==0));   b, a (ntaps), zi (ntaps-1) from lfilter_zi,
 *   edge = 3*ntaps.
 * x, y: (n_sig, n_samples) float64; work (device, *_dev only): (n_sig, n_samples + 2*edge).
 * sos / zi / b / a are HOST pointers in both forms (they travel as kernel arguments).           */
tda_status tda_sosfiltfilt_dev(tda_ctx* ctx, const double* x, int n_sig, int n_samples, const double* sos,
                               const double* zi, int n_sections, int edge, double* y, double* work,
                               void* stream);
tda_status tda_sosfiltfilt(tda_ctx* ctx, const double* x, int n_sig, int n_samples, const double* sos,
                           const double* zi, int n_sections, int edge, double* y);
tda_status tda_filtfilt_dev(tda_ctx* ctx, const double* x, int n_sig, int n_samples, const double* b,
                            const double* a, const double* zi, int ntaps, int edge, double* y, double* work,
                            void* stream);
tda_status tda_filtfilt(tda_ctx* ctx, const double* x, int n_sig, int n_samples, const double* b,
                        const double* a, const double* zi, int ntaps, int edge, double* y);

/* Filter BANKS: the same n_sig signals through n_filters filters of equal structure in ONE launch -- the five frequency
 * bands of apply_bandpass_filter (nb1:236-263, one call per band in preprocess_file nb1:388-494) and of bandpass_filter
 * (utils.py:66-74, one call per band in process_recording, cmp:63-64).  sos (n_filters, n_sections, 6), zi (n_filters,
 * n_sections, 2) / b, a (n_filters, ntaps), zi (n_filters, ntaps-1): HOST pointers; y (n_filters, n_sig, n_samples),
 * work (n_filters, n_sig, n_samples + 2*edge): device.  n_filters <= 5.  Bit-identical to the single-filter calls. */
tda_status tda_sosfiltfilt_bank_dev(tda_ctx* ctx, const double* x, int n_sig, int n_samples, const double* sos,
                                    const double* zi, int n_filters, int n_sections, int edge, double* y, double* work,
                                    void* stream);
tda_status tda_filtfilt_bank_dev(tda_ctx* ctx, const double* x, int n_sig, int n_samples, const double* b,
                                 const double* a, const double* zi, int n_filters, int ntaps, int edge, double* y,
                                 double* work, void* stream);

/* RAGGED filter banks: signals of different lengths, packed back to back, each filtered over its own length with its
 * own odd extension and trim -- scipy.signal.sosfiltfilt / filtfilt on every signal alone, bit-identical.
 * tda_sosfiltfilt_bank_ragged_dev replaces apply_bandpass_filter (nb1:236-263) for the EEG of n_rec recordings of
 * lengths len[r]: recording r is an (n_ch, len[r]) block of x at element n_ch * off[r] (off: exclusive prefix sum of
 * len, n_rec + 1 entries); y (n_filters, n_ch * off[n_rec]) in the same layout per filter; work (n_filters, n_ch *
 * (off[n_rec] + 2*edge*n_rec)), recording r at n_ch * (off[r] + 2*edge*r).
 * tda_filtfilt_bank_ragged_dev replaces bandpass_filter (utils.py:66-74, cmp:63-64) for n_sig envelopes of lengths
 * len[s] (one channel each): signal s at element off[s]; y (n_filters, off[n_sig]); work (n_filters, off[n_sig] +
 * 2*edge*n_sig), signal s at off[s] + 2*edge*s; ntaps <= 9.
 * len, off: device int64 tables; len_host: the same lengths on the host -- a length <= edge is TDA_ERR_INVALID (scipy
 * raises too).  sos / zi / b / a: host, as in the equal-length banks. */
tda_status tda_sosfiltfilt_bank_ragged_dev(tda_ctx* ctx, const double* x, int n_rec, int n_ch, const long long* len,
                                           const long long* off, const long long* len_host, const double* sos,
                                           const double* zi, int n_filters, int n_sections, int edge, double* y,
                                           double* work, void* stream);
tda_status tda_filtfilt_bank_ragged_dev(tda_ctx* ctx, const double* x, int n_sig, const long long* len,
                                        const long long* off, const long long* len_host, const double* b,
                                        const double* a, const double* zi, int n_filters, int ntaps, int edge,
                                        double* y, double* work, void* stream);
/* Selected windows of packed signals into a stack: out[w, t] = src[start[w] + t], t < win_len (start: device int64,
 * n_win) -- create_windows + the np.linspace selection (cmp:65,77-80) of the band-passed envelopes of ragged
 * recordings, for the tau / Takens kernels. */
tda_status tda_gather_windows_dev(tda_ctx* ctx, const double* src, const long long* start, int n_win, int win_len,
                                  double* out, void* stream);

/* Audio front end.  tda_upfirdn replaces scipy.signal.resample_poly(audio, 250, 44100) (scripts/utils.py:77-79):
 * h (len_h, host-designed exactly as scipy does, incl. its zero padding and the factor `up`),
 *   y[j] = sum_i x[i] * h[(j + n_pre_remove)*down - i*up],  j < n_out.
 * tda_hilbert_envelope replaces np.abs(scipy.signal.hilbert(s)) (utils.py:58-59):
 *   env[n] = sqrt(x[n]^2 + (sum_m x[m] g[(n-m) mod N])^2),  g = imag(ifft(h_hilbert)) tabulated by the host.
 * float64, agreement with scipy to rounding (1e-12 relative), not bit-identical.  *_dev: all pointers device. */
tda_status tda_upfirdn_dev(tda_ctx* ctx, const double* x, long long n_in, const double* h, int len_h, int up,
                           int down, long long n_pre_remove, long long n_out, double* y, void* stream);
tda_status tda_upfirdn(tda_ctx* ctx, const double* x, long long n_in, const double* h, int len_h, int up,
                       int down, long long n_pre_remove, long long n_out, double* y);
tda_status tda_hilbert_envelope_dev(tda_ctx* ctx, const double* x, int n, const double* g, double* env,
                                    void* stream);
tda_status tda_hilbert_envelope(tda_ctx* ctx, const double* x, int n, const double* g, double* env);
/* Audio front end for RAGGED signals: every signal of a shard in one launch, signals packed back to back (signal s has
 * len[s] samples at element off[s], off the exclusive prefix sum of len; len, off: device int64; len_host: the same
 * lengths on the host, checked here).  float64, agreement with scipy to rounding, not bit-identical.
 * tda_resample_poly_ragged_dev replaces scipy.signal.resample_poly(audio, up, down) of resample_audio
 * (scripts/utils.py:77-79) for every signal: hp (up, n_phase_taps) device, the polyphase table hp[p][q] = h[p + up*q] of
 * the host-designed filter (as for tda_upfirdn; zero past the end of h -- one table serves every length, see
 * preprocess.AudioPlan); signal s gives ceil(len[s]*up/down) outputs at y + out_off[s] (out_off: device int64).
 * up <= 8.  Geometry that makes no sense (up, down, n_phase_taps < 1, n_pre_remove < 0, a length < 1) is
 * TDA_ERR_INVALID.
 * tda_hilbert_envelope_ragged_dev replaces np.abs(scipy.signal.hilbert(s)) (utils.py:58-59) for every signal: g
 * device, the table g_N = imag(ifft(h_hilbert)) of signal s's length at g + g_off[s] (g_off: device int64; signals of
 * one length may share a table); env in the layout of x.  Lengths in [1, 8192]. */
tda_status tda_resample_poly_ragged_dev(tda_ctx* ctx, const double* x, int n_sig, const long long* len,
                                        const long long* off, const long long* len_host, const long long* out_off,
                                        const double* hp, int n_phase_taps, int up, int down, int n_pre_remove,
                                        double* y, void* stream);
tda_status tda_hilbert_envelope_ragged_dev(tda_ctx* ctx, const double* x, int n_sig, const long long* len,
                                           const long long* off, const long long* len_host, const double* g,
                                           const long long* g_off, double* env, void* stream);

/* ---- delay from the first zero crossing of the autocorrelation ---------------
 * replaces compute_tau (scripts/utils.py:92-104). max_lag < 0 = None (len/4).
 * n_t: 2 <= n_t <= 8192 (the centred window is held in LDS, 8 n_t bytes); anything else is
 * TDA_ERR_UNSUPPORTED.  max_lag: any value; as in the reference it is cut to n_t - 1.  The same
 * limits hold for tda_tau_segments_dev.                                                */
tda_status tda_tau_batch_dev(tda_ctx* ctx, const double* win, int n_win, int n_t, int max_lag,
                             int* tau, void* stream);
tda_status tda_tau_batch(tda_ctx* ctx, const double* win, int n_win, int n_t, int max_lag, int* tau);
/* The driver's use of it (scripts/tda_eeg_audio_comparison.py:83, scripts/matched_vs_mismatched.py:56): one tau per
 * (recording, band) group, from the FIRST window of the group (window seg_off[g] of win).  tau_seg: (n_seg);
 * tau_win (nullable): (n_total) receives the group's value for each of its windows, the per-window array
 * tda_takens_rips_batch takes.  Device pointers only (a stage of the batched driver). */
tda_status tda_tau_segments_dev(tda_ctx* ctx, const double* win, const int* seg_off, int n_seg, int n_t,
                                int max_lag, int* tau_seg, int* tau_win, void* stream);

/* ---- Delay and dimension selection: mutual information and false nearest neighbours ------
 * The two parameters of a delay embedding as the nonlinear time-series literature picks them: the delay tau at the first
 * minimum of the average mutual information of the signal with its own past (Fraser & Swinney 1986), the dimension as the
 * smallest one at which the false nearest neighbours vanish (Kennel, Brown & Abarbanel 1992).  compute_tau above is the
 * linear counterpart of the first; the Takens entry points take what these produce (a per-window tau, dim <= TDA_MAX_DIM).
 * The contract is this text; tests/embedding_ref.py evaluates it twice.  Every float64 operation below is one IEEE
 * operation, no contraction.
 *
 * Average mutual information: tda_ami_batch[_dev], tda_ami_segments_dev.
 *   Inputs.     win (n_win, n_t) float64, 4 <= n_t <= TDA_AMI_MAX_SAMPLES.  max_lag < 0 means n_t / 4; max_lag is then cut
 *               to n_t - 2.  n_bins in [2, TDA_AMI_MAX_BINS].
 *   Bins.       lo, hi: the exact minimum and maximum of the window, w = hi - lo.
 *               b_i = min(n_bins - 1, (int)(((x_i - lo) / w) * (double)n_bins)); a sample equal to hi lands in the last bin.
 *   Joint counts.  For L = 0..max_lag, N = n_t - L: J_L[p][q] = #{ i in [0, N) : b_i = p, b_(i+L) = q },
 *               r_p = sum_q J_L[p][q], s_q = sum_p J_L[p][q].
 *   AMI, nats.  I(L) = sum over the cells with J > 0 of ((double)J / (double)N) * log((double)(J * N) / (double)(r_p * s_q)),
 *               J = J_L[p][q]; the integer products are exact (below 2^27).
 *   ami         (n_win, max_lag + 1) float64, the I(L), with max_lag as resolved above.
 *   tau         (n_win) int32: the smallest L in [1, max_lag - 1] with I(L) < I(L-1) and I(L) <= I(L+1), compared on the
 *               doubles that ami holds, so tau is a byte-exact function of the returned row; 0 without such an L.
 *   joint       (nullable) (n_win, max_lag + 1, n_bins, n_bins) int32, the J_L.  A NULL joint changes no other byte.
 *   status      (n_win) int32.  TDA_WIN_NOT_FINITE: a sample is not finite; ami NaN, tau 0, joint 0.
 *               TDA_WIN_DEGENERATE: hi == lo; ami 0.0, tau 0, joint 0.  Otherwise 0.
 *   Segments.   tda_ami_segments_dev is to tda_ami_batch_dev what tda_tau_segments_dev is to tda_tau_batch_dev: group g
 *               takes its delay from its FIRST window (window seg_off[g] of win); tau_seg (n_seg) and, when it is given,
 *               tau_win (n_total: every window of the group) receive it.  Where the rule gives 0 (no minimum, a refused
 *               window) both receive compute_tau's fallback max(max_lag / 10, 1) with the resolved max_lag, so tau_win goes
 *               straight into the Takens entry points.  An empty group has tau_seg 0.  Device pointers only.
 *   Determinism.  joint and the bins are bytes of this text.  ami holds the rounding of log and of the sum, which the kernel
 *               adds in one fixed order of its own (DESIGN.md 3.26 has the measured bar against the numpy statement).  A
 *               window alone and inside a batch, and one run and the next, give the same bytes.  The only atomics are
 *               integer additions to a wave's own histogram in LDS, which commute; no float atomics, no global atomics, no
 *               polls; every loop is bounded before it starts by n_t, max_lag or n_bins.
 *
 * False nearest neighbours: tda_fnn_batch[_dev].
 *   Inputs.     win (n_win, n_t) float64, 4 <= n_t <= TDA_FNN_MAX_SAMPLES.  tau (n_win) int32, the delay of every window.
 *               d_max in [1, TDA_FNN_MAX_DIM], theiler in [1, n_t], r_tol > 0, a_tol > 0, frac_tol in [0, 1].
 *   Definition, for d = 1..d_max.  M_d = n_t - d tau, the points i = 0..M_d - 1 of the d-dimensional embedding that have a
 *               (d+1)-th coordinate.  M_d < 2: the rows of this dimension are zero (nn: -1).
 *               D2_d(i, j): s = 0.0; for k = 0..d-1 ascending: e = x[i + k tau] - x[j + k tau]; s = s + e * e.
 *               Neighbour j*(i): the j in [0, M_d) with |i - j| >= theiler and the smallest D2_d(i, j), ties to the smallest
 *               j; -1 without a candidate.  With D2 = D2_d(i, j*), e = x[i + d tau] - x[j* + d tau], e2 = e * e:
 *                 criterion 1 (distance)  D2 > 0 ? e2 > (r_tol * r_tol) * D2 : e2 > 0.0
 *                 criterion 2 (size)      (D2 + e2) > R2, R2 = (a_tol * a_tol) * var; m: the sequential sum of the window
 *                                         divided by (double)n_t (as tda_tau_batch takes its mean), var: the sequential
 *                                         sum of (x - m) * (x - m) divided by (double)n_t
 *   counts      (n_win, d_max, TDA_FNN_COLS) int32, the columns
 *                 0 valid           points with a neighbour
 *                 1 false_distance  of those, false by criterion 1
 *                 2 false_size      false by criterion 2
 *                 3 false_either    false by either
 *   frac        (n_win, d_max) float64: valid ? (double)false_either / (double)valid : 0.0
 *   dim         (n_win) int32: the smallest d with valid > 0 and (double)false_either <= frac_tol * (double)valid; 0
 *               without one.
 *   nn          (nullable) (n_win, d_max, n_t) int32: nn[., d - 1, i] = j*(i), -1 wherever there is none (i >= M_d, no
 *               candidate, a refused window).  A NULL nn changes no other byte.
 *   status      (n_win) int32.  TDA_WIN_NOT_FINITE: a sample is not finite.  TDA_WIN_TOO_LARGE: tau < 1, as the Takens
 *               entry points refuse it.  TDA_WIN_DEGENERATE: M_1 < 2.  In all three counts, frac and dim are zero and nn
 *               is -1.  Otherwise 0.
 *   Determinism.  Every output is bytes of this text.  No atomics, no polls; every loop is bounded before it starts by n_t
 *               or d_max.
 *
 * Limits.  Anything outside the ranges above is TDA_ERR_INVALID with a message in tda_last_error; nothing is launched or
 * written.  The _dev forms only enqueue on `stream` and allocate nothing.  The host forms stage every buffer. */
#define TDA_AMI_MAX_SAMPLES 8192
#define TDA_AMI_MAX_BINS    32
#define TDA_FNN_MAX_SAMPLES 2048
#define TDA_FNN_MAX_DIM     8
#define TDA_FNN_COLS        4
tda_status tda_ami_batch_dev(tda_ctx* ctx, const double* win, int n_win, int n_t, int max_lag, int n_bins, double* ami,
                             int* tau, int* joint, int* status, void* stream);
tda_status tda_ami_batch(tda_ctx* ctx, const double* win, int n_win, int n_t, int max_lag, int n_bins, double* ami,
                         int* tau, int* joint, int* status);
tda_status tda_ami_segments_dev(tda_ctx* ctx, const double* win, const int* seg_off, int n_seg, int n_t, int max_lag,
                                int n_bins, int* tau_seg, int* tau_win, void* stream);
tda_status tda_fnn_batch_dev(tda_ctx* ctx, const double* win, const int* tau, int n_win, int n_t, int d_max, int theiler,
                             double r_tol, double a_tol, double frac_tol, int* counts, double* frac, int* dim, int* nn,
                             int* status, void* stream);
tda_status tda_fnn_batch(tda_ctx* ctx, const double* win, const int* tau, int n_win, int n_t, int d_max, int theiler,
                         double r_tol, double a_tol, double frac_tol, int* counts, double* frac, int* dim, int* nn,
                         int* status);

/* ---- 11 scalar features per diagram ------------------------------------------
 * replaces extract_features (scripts/utils.py:144-177) ==
 * extract_persistence_features (tda_eeg_classification_v2.py:179-250).
 * dgm: (n_dgm, cap, 2) float64; cnt: (n_dgm); feat: (n_dgm, 11) float64.             */
tda_status tda_features_batch_dev(tda_ctx* ctx, const double* dgm, const int* cnt, int n_dgm,
                                  int cap, double* feat, void* stream);
tda_status tda_features_batch(tda_ctx* ctx, const double* dgm, const int* cnt, int n_dgm,
                              int cap, double* feat);

/* ---- finishing pass over the diagrams of a batch ---------------------------------
 * Up to four diagram sets in ONE call (a launch for the diagrams of up to 64 rows and, where a set has room for more, one
 * for the larger ones: tda_set_launch_scheme): for sets with order != 0 the H1 rows are put
 * into ripser's order in place, and where feat != NULL the 11 scalars of extract_features are written -- what
 * tda_features_batch_dev does for one set.  The driver of a whole step runs the Rips entry points under
 * TDA_ORDER_DEFERRED and finishes the EEG H0 / EEG H1 / audio H1 diagrams of the batch with one call
 * (scripts/tda_eeg_audio_comparison.py:92-99; scripts/tda_eeg_classification_v2.py:410-416).  `sets` is a host array
 * of descriptors; the pointers inside are device pointers. */
typedef struct {
    double* rows;      /* (n_dgm, cap, 2) float64 */
    const int* cnt;    /* (n_dgm) */
    int cap;
    int order;         /* 1: rows are H1 rows in emission order -> descending birth (ripser's order) */
    double* feat;      /* (n_dgm, 11) float64 or NULL */
} tda_diagram_set;
tda_status tda_diagram_finish_dev(tda_ctx* ctx, const tda_diagram_set* sets, int n_sets, int n_dgm, void* stream);
/* IN_CALL (default): every Rips entry point returns H1 rows in ripser's order (it launches the finishing pass for
 * its own diagrams).  DEFERRED: rows stay in emission order until the caller's tda_diagram_finish_dev. */
#define TDA_ORDER_IN_CALL  0
#define TDA_ORDER_DEFERRED 1
tda_status tda_set_h1_order(tda_ctx* ctx, int policy);
/* How tda_diagram_finish_dev (and the finishing pass inside the Rips entry points) and the Wasserstein entry points
 * split their work over launches when the diagram buffers have room for more rows than the diagrams usually have.  The
 * results do not depend on it, bit for bit; it exists so that one process can run the schemes against each other.
 * LISTS (default): diagrams of up to 64 rows are finished by the packed kernel (eight lanes per diagram), pairs of up
 *   to 64 x 64 points solved by the small launch; what they leave goes onto a per-stream list, and the launch sized by
 *   the capacities runs over that list on a small fixed grid.
 * GRID: the small launch has one wavefront per diagram, and the launch sized by the capacities starts a wavefront for
 *   every diagram / pair of the batch (those that are not its own leave after one load).
 * ONE: the launch sized by the capacities alone (what the environment variables TDA_FINISH_ONE_LAUNCH /
 *   TDA_WS_ONE_LAUNCH select for their kernel, whatever is set here). */
#define TDA_SCHEME_LISTS 0
#define TDA_SCHEME_GRID  1
#define TDA_SCHEME_ONE   2
tda_status tda_set_launch_scheme(tda_ctx* ctx, int scheme);
/* The Wasserstein entry points leave out work whose result is known before it is done: in a pair of diagrams with one
 * common birth (two H0 diagrams) the points too short or too long to be matched with any point of the other diagram,
 * and the whole assignment of a pair in which every point is nearer to the diagonal than to the other diagram.  The
 * results do not depend on it, bit for bit; on = 0 runs the full computation, so that one process can hold the two
 * against each other.  Default: on. */
tda_status tda_set_wasserstein_pruning(tda_ctx* ctx, int on);
/* dev_counters: NULL (default: nothing is counted) or a device u64[3] that the caller zeroes; every solved pair adds
 * [0] 1 if it took the all-diagonal short cut, [1] the rows plus columns trimmed off its equal-birth recurrence,
 * [2] 1.  Both stay 0 while pruning is off. */
tda_status tda_set_wasserstein_counter(tda_ctx* ctx, unsigned long long* dev_counters);

/* ---- per-recording aggregation -------------------------------------------------
 * replaces the mean/std over windows of process_file_features
 * (tda_eeg_classification_v2.py:429-436).
 * feat_h0, feat_h1 : (n_total, 11) float64 features of the used windows, grouped
 * seg_off          : (n_seg+1) int32 offsets of each (recording, band) group
 * out              : (n_seg, 44) float64 in the column order of features/feature_names.txt
 *                    within one band: per feature {h0 mean, h0 std, h1 mean, h1 std}.  */
tda_status tda_aggregate_batch_dev(tda_ctx* ctx, const double* feat_h0, const double* feat_h1,
                                   const int* seg_off, int n_seg, double* out, void* stream);
tda_status tda_aggregate_batch(tda_ctx* ctx, const double* feat_h0, const double* feat_h1,
                               const int* seg_off, int n_seg, int n_total, double* out);

/* ---- np.nanmean over the windows of each (recording, band) group ----------------
 * replaces np.nanmean(wass_h0) / np.nanmean(vals) (scripts/tda_eeg_audio_comparison.py:117-118,
 * scripts/matched_vs_mismatched.py:95).  x: (n_total) float64; seg_off: (n_seg+1) int32.
 * Empty or all-NaN groups give NaN.                                                    */
tda_status tda_segment_nanmean_dev(tda_ctx* ctx, const double* x, const int* seg_off, int n_seg,
                                   double* out, void* stream);
tda_status tda_segment_nanmean(tda_ctx* ctx, const double* x, const int* seg_off, int n_seg,
                               int n_total, double* out);

/* ---- one result row per (recording, band) group ---------------------------------------
 * out: (n_seg, 48) float64 = [ nanmean of w_h0 (cmp:117), nanmean of w_h1 (cmp:118), tau (cmp:83), number of
 * windows, the 44 values of tda_aggregate_batch (v2:429-436) ] -- tda_segment_nanmean x 2 + tda_aggregate_batch
 * + the row assembly in ONE launch; the rows are what the GPUs of a node exchange.  Device pointers only.
 * status_a / status_b / seg_flags (all nullable): per-window status arrays of the two Rips calls and an
 * (n_seg) int32 output that receives, per group, the OR of their status words without TDA_WIN_DEGENERATE (a result,
 * not a condition) -- what a caller running under TDA_RETRY_FIRST_PASS / ONE_STEP copies to the host: bit
 * TDA_WIN_CLASS_OVERFLOW asks for the rest of the ladder, any other bit means rows the reference would not give. */
tda_status tda_recording_rows_dev(tda_ctx* ctx, const double* w_h0, const double* w_h1, const int* tau_seg,
                                  const double* feat_h0, const double* feat_h1, const int* seg_off,
                                  int n_seg, double* out, const int* status_a, const int* status_b,
                                  int* seg_flags, void* stream);

/* ---- Spearman correlation of feature time series ------------------------------------
 * replaces the spearmanr(a_ts, e_ts) loop of process_recording
 * (scripts/tda_eeg_audio_comparison.py:104-114): per (recording, band) group and per selected
 * feature column, the Pearson correlation of the average ranks of the audio and EEG series;
 * r = 0 when the group has < 5 windows or a series has np.std <= 1e-10 (the reference's rule,
 * which then reports p = 1).  x, y: (n_total, ld) float64; cols: (n_cols) column indices;
 * r: (n_seg, n_cols).  The p-value is a function of (r, n) only (Student t) and is left to the host. */
tda_status tda_spearman_batch_dev(tda_ctx* ctx, const double* x, const double* y, int ld, const int* cols,
                                  int n_cols, const int* seg_off, int n_seg, double* r, void* stream);
tda_status tda_spearman_batch(tda_ctx* ctx, const double* x, const double* y, int n_total, int ld,
                              const int* cols, int n_cols, const int* seg_off, int n_seg, double* r);

/* ---- temporal correlation of the H1 feature time series of a step ---------------------
 * replaces the window filter and the spearmanr(a_ts, e_ts) loop of process_recording
 * (scripts/tda_eeg_audio_comparison.py:90-91,104-114) on the per-window feature matrices of a step, r AND p:
 * fa, fe: (n_total, ld) float64, the audio H1 and EEG H1 features of every window; cols: (n_cols) column indices
 * (each < ld); seg_off: (n_seg+1) int32; status_b (nullable): (n_total) status words of the audio Rips call.
 * The survivors of a group are its windows with (status_b & (TDA_WIN_DEGENERATE | TDA_WIN_TOO_LARGE)) == 0, in
 * their order (cmp:90-91, the rule of tda_recording_rows_dev); m is their number.  Per group and column:
 *   m == 0                              r = p = NaN   (the reference drops the band, cmp:101-102)
 *   m < 5 or np.std of a series <= 1e-10  r = 0, p = 1  (cmp:110-114)
 *   otherwise  r = Pearson correlation of the average ranks, the bits of tda_spearman_batch on the survivors;
 *              p = I_{1-r^2}((m-2)/2, 1/2), the two-sided Student-t p-value scipy.stats.spearmanr reports (0 at r = +-1)
 * out: (n_seg, 2 * n_cols) float64, [r, p] per column.  Any m.  The _dev call only enqueues one fixed-size launch
 * (no allocation, no host synchronisation): it may be captured into a graph.  The host twin also checks the tables. */
tda_status tda_temporal_corr_dev(tda_ctx* ctx, const double* fa, const double* fe, int ld, const int* cols,
                                 int n_cols, const int* seg_off, int n_seg, const int* status_b, double* out,
                                 void* stream);
tda_status tda_temporal_corr_batch(tda_ctx* ctx, const double* fa, const double* fe, int n_total, int ld,
                                   const int* cols, int n_cols, const int* seg_off, int n_seg, const int* status_b,
                                   double* out);

/* ---- Wasserstein distance between diagrams ------------------------------------
 * replaces safe_wasserstein (scripts/utils.py:180-191) -> persim.wasserstein
 * (order 1, Euclidean ground metric, diagonal cost (d-b)/sqrt 2).
 * dgm_a: (n_a, cap_a, 2), cnt_a: (n_a);  dgm_b likewise.
 * idx_a, idx_b: (n_pairs) int32 diagram indices to pair (NULL = identity).
 * Rows with a non-finite entry are ignored and an empty diagram becomes {(0,0)}
 * (utils.py:182-187).  out: (n_pairs) float64, NaN where status != 0.                 */
tda_status tda_wasserstein_batch_dev(tda_ctx* ctx, const double* dgm_a, const int* cnt_a, int cap_a,
                                     const double* dgm_b, const int* cnt_b, int cap_b,
                                     const int* idx_a, const int* idx_b, int n_pairs,
                                     double* out, int* status, void* stream);
tda_status tda_wasserstein_batch(tda_ctx* ctx, const double* dgm_a, const int* cnt_a, int n_a, int cap_a,
                                 const double* dgm_b, const int* cnt_b, int n_b, int cap_b,
                                 const int* idx_a, const int* idx_b, int n_pairs,
                                 double* out, int* status);

/* ---- Bottleneck distance between diagrams ---------------------------------------
 * The largest matched cost under the best matching (the definition of Hera, GUDHI and persim.bottleneck).  The
 * diagrams are cleaned as for the Wasserstein distance: rows with a non-finite entry are ignored and an empty diagram
 * becomes {(0,0)} (utils.py:182-187).  Ground cost between points: L-infinity,
 *     C_ij = fmax(fabs(a_b - b_b), fabs(a_d - b_d));
 * a point may go to the diagonal at cost 0.5 * (d - b); diagonal to diagonal is free.  The result is the minimum over
 * matchings of the largest matched cost.  Every cost is one correctly rounded float64 operation on the inputs and the
 * result is one of them, chosen by comparisons only: it equals a CPU evaluation of this definition bit for bit.
 * d >= b is assumed for every finite row (Rips never emits another one).
 * Arguments as tda_wasserstein_batch[_dev].  out: (n_pairs) float64, NaN where status != 0; status: (n_pairs) int32.
 * A pair with a diagram of more than 512 finite rows is TDA_WIN_NOT_CONVERGED (the buffers may be larger than that), as
 * is a pair whose solver hit one of its loop bounds.  The _dev form only enqueues on `stream` and allocates nothing. */
tda_status tda_bottleneck_batch_dev(tda_ctx* ctx, const double* dgm_a, const int* cnt_a, int cap_a,
                                    const double* dgm_b, const int* cnt_b, int cap_b,
                                    const int* idx_a, const int* idx_b, int n_pairs,
                                    double* out, int* status, void* stream);
tda_status tda_bottleneck_batch(tda_ctx* ctx, const double* dgm_a, const int* cnt_a, int n_a, int cap_a,
                                const double* dgm_b, const int* cnt_b, int n_b, int cap_b,
                                const int* idx_a, const int* idx_b, int n_pairs,
                                double* out, int* status);

/* ---- Wasserstein distances of order 1 and 2, L2 or L-infinity ground metric ---------
 * What Hera, GUDHI and giotto-tda call wasserstein_distance: order 2 (the metric of Frechet means on diagram space) and
 * the L-infinity ground metric with (d - b) / 2 to the diagonal (the convention of the bottleneck distance above), beside
 * persim's L2 with (d - b) / sqrt 2.
 *   Arguments.   As tda_wasserstein_batch[_dev].
 *   Parameters.  order is 1 or 2; ground is TDA_GROUND_L2 or TDA_GROUND_LINF.  Anything else is TDA_ERR_INVALID and
 *                nothing is launched.  All four combinations are accepted.
 *   Cleaning.    As for the Wasserstein distance: rows with a non-finite entry are ignored, an empty diagram becomes
 *                {(0,0)}.
 *   Costs.       Every line is one correctly rounded float64 operation; there is no multiply-add.
 *                  dx = fabs(a_b - b_b), dy = fabs(a_d - b_d), p = d - b.
 *                  L2:         e = (dx * dx) + (dy * dy).
 *                    order 1:  point cost sqrt(e), diagonal cost p * 0.7071067811865476.
 *                    order 2:  point cost e (no root), diagonal cost 0.5 * (p * p).
 *                  L-infinity: m = fmax(dx, dy), h = 0.5 * p.
 *                    order 1:  point cost m, diagonal cost h.
 *                    order 2:  point cost m * m, diagonal cost h * h.
 *   Value.       V is the minimum over partial matchings of the sum of the matched point costs plus the diagonal costs of
 *                every unmatched point of both diagrams; diagonal to diagonal is free.  The result is V for order 1 and
 *                sqrt(V), correctly rounded, for order 2.
 *   Exactness.   Every cost is the same float64 on the GPU and in a CPU evaluation of this text.  The result differs from
 *                such an evaluation only by the order of the additions and by which of several equally good matchings was
 *                summed.  Two diagrams whose points all share one birth are summed as (all diagonal costs) + (the gains
 *                C - s - t of the matched pairs); a V that comes out below 0 there is returned as 0.  d >= b is assumed
 *                for every finite row.  A pair alone and the same pair inside a batch give the same bytes.
 *   Status.      A pair with a diagram of more than 512 finite rows is TDA_WIN_NOT_CONVERGED with NaN (the buffers may be
 *                larger than that), as is a pair whose solver hit one of its loop bounds.  No other status occurs.
 *   The _dev form only enqueues on `stream` and allocates nothing.  tda_set_wasserstein_pruning and
 *   tda_set_wasserstein_counter apply as they do to tda_wasserstein_batch: the short cuts never change a byte.
 * Relation to tda_wasserstein_batch.  (order 1, TDA_GROUND_L2) is the same mathematical quantity, not the same float:
 * that entry follows sklearn's |x|^2 - 2 x.y + |y|^2 expansion, whose error is bounded at 7.3e-8 X per point cost (X the
 * largest |coordinate| of the pair; csrc/wasserstein.hip), so the two may differ by up to about min(M, N) times that.
 * tda_wasserstein_batch stays the drop-in for the reference; this entry is not a replacement for it. */
#define TDA_GROUND_L2   0
#define TDA_GROUND_LINF 1
tda_status tda_wasserstein_q_batch_dev(tda_ctx* ctx, const double* dgm_a, const int* cnt_a, int cap_a,
                                       const double* dgm_b, const int* cnt_b, int cap_b,
                                       const int* idx_a, const int* idx_b, int n_pairs,
                                       int order, int ground, double* out, int* status, void* stream);
tda_status tda_wasserstein_q_batch(tda_ctx* ctx, const double* dgm_a, const int* cnt_a, int n_a, int cap_a,
                                   const double* dgm_b, const int* cnt_b, int n_b, int cap_b,
                                   const int* idx_a, const int* idx_b, int n_pairs,
                                   int order, int ground, double* out, int* status);

/* ---- Sliced Wasserstein distance between diagrams ---------------------------------
 * Carriere, Cuturi, Oudot 2017 (what persim.sliced_wasserstein computes): project both diagrams onto a handful of
 * directions, sort each projection, take the L1 difference of the sorted lists, average over the directions.  persim is
 * not installed anywhere this project runs, so no parity with it is claimed.  The contract is this text.
 *   Cleaning.     As for the Wasserstein distance: rows with a non-finite entry are ignored, an empty diagram becomes
 *                 {(0,0)}.  A has m rows (b, d) after cleaning, B has n, and N = m + n.
 *   Images.       For a row, h = 0.5 * (b + d) (one addition, one exact multiplication); its image is the point (h, h).
 *   Lists.        A' is the rows of A followed by the images of the rows of B; B' is the rows of B followed by the images
 *                 of the rows of A.  Both have N points.
 *   Directions.   dirs is an (n_dirs, 2) float64 table (c_k, s_k) passed by the caller.  The kernel never evaluates a
 *                 trigonometric function and never normalises a direction.
 *   Projection.   For every point (x, y) of A' and B', the images included: p = (c * x) + (s * y) -- two rounded
 *                 multiplications and one rounded addition, no multiply-add.  The same formula applies to the images; it
 *                 is not (c + s) * h.
 *   Per direction. u is the N projections of A' in ascending order, v those of B'; t_i = fabs(u_i - v_i), i < N; L_k is
 *                 the sum of the t_i.  Sorting is an order-free selection: ties and -0.0 do not change any t_i.
 *   Result.       SW = (sum over k of L_k) / n_dirs.
 * Order of additions.  Every t_i is the same float64 on the GPU and in a CPU evaluation of this text.  Every term is
 * non-negative, so the order of the additions is not part of the contract.  It is deterministic: no atomics; the order
 * depends only on the rank index i and the direction index k; a pair alone and the same pair inside a batch give the same
 * bytes; SW(A, B) and SW(B, A) give the same bytes.
 * Tolerance.  Any two summation orders of n non-negative terms agree within 2 (n - 1) 2^-53 relative, to first order;
 * applied to the inner and the outer sum, the GPU value agrees with any CPU evaluation of this text within
 * (N + n_dirs + 1) * 2^-52 * value, and exactly where the value is 0.
 * Limits: 1 <= n_dirs <= TDA_MAX_DIRECTIONS and cap >= 1; anything else is TDA_ERR_INVALID and nothing is launched.  A pair
 * with N > TDA_SW_MAX_POINTS gets NaN and TDA_WIN_TOO_LARGE.  The host form also rejects directions that are not finite; the
 * _dev form cannot see them and applies the formula as written.
 * Arguments as tda_wasserstein_batch[_dev] (idx_a / idx_b NULL = identity), plus dirs.  out: (n_pairs) float64, NaN where
 * status != 0; status: (n_pairs) int32.  The _dev form only enqueues on `stream` and allocates nothing. */
#define TDA_MAX_DIRECTIONS 128
#define TDA_SW_MAX_POINTS  512
tda_status tda_sliced_wasserstein_batch_dev(tda_ctx* ctx, const double* dgm_a, const int* cnt_a, int cap_a,
                                            const double* dgm_b, const int* cnt_b, int cap_b,
                                            const int* idx_a, const int* idx_b, int n_pairs,
                                            const double* dirs, int n_dirs, double* out, int* status, void* stream);
tda_status tda_sliced_wasserstein_batch(tda_ctx* ctx, const double* dgm_a, const int* cnt_a, int n_a, int cap_a,
                                        const double* dgm_b, const int* cnt_b, int n_b, int cap_b,
                                        const int* idx_a, const int* idx_b, int n_pairs,
                                        const double* dirs, int n_dirs, double* out, int* status);

/* ---- Persistence landscapes and Betti curves, averaged per group ------------------
 * A diagram has rows (b_i, d_i), i < min(cnt, cap), float64.  F is the set of rows with both values finite (the mask of
 * tda_features_batch).  The grid is n_grid float64 values t_j, passed as an array: the caller computes them, the kernel
 * never does.  There is no multiply-add anywhere in the definition.
 *   tent_i(t)   = min(t - b_i, d_i - t), replaced by 0.0 where it is not > 0; each difference is one IEEE subtraction.
 *   lambda_k(t), k = 1..K: the k-th largest value of the multiset {tent_i(t) : i in F} padded with K zeros.
 *   beta(t)     = the number of rows i < min(cnt, cap) with b_i <= t < d_i, as float64; rows with d_i = +inf count.
 *   V           = [lambda_1, ..., lambda_K, beta], shape (K + 1, n_grid): the vector of a diagram.
 * Group mean, for the diagrams seg_off[g] <= w < seg_off[g + 1] in buffer order: diagrams whose status word has a bit of
 * skip_mask are left out; s = V(first kept), then s = s + V(next kept) and so on, elementwise in that order; the result
 * is s / n_kept, and NaN in every element when n_kept = 0.  This is np.mean(np.stack(kept), axis=0) (a plain sequential
 * sum).  A group of one diagram is that diagram's own vector (x / 1): with seg_off = NULL every diagram is its own group
 * and n_seg must be n_dgm.  The result does not depend on the order of the rows of a diagram.
 * Limits: 1 <= n_levels <= TDA_MAX_LANDSCAPES, 1 <= n_grid <= TDA_MAX_GRID, cap >= 1; anything else is TDA_ERR_INVALID
 * and nothing is launched.  Every operation is one correctly rounded float64 operation or an order-free selection: the
 * output equals a CPU evaluation of this definition bit for bit.
 * out: (n_seg, n_levels + 1, n_grid) float64.  The _dev form only enqueues on `stream` and allocates nothing. */
#define TDA_MAX_LANDSCAPES 8
#define TDA_MAX_GRID       256
tda_status tda_landscape_mean_dev(tda_ctx* ctx, const double* dgm, const int* cnt, int cap, int n_dgm,
                                  const int* seg_off, int n_seg, const int* status, int skip_mask,
                                  const double* grid, int n_grid, int n_levels, double* out, void* stream);
tda_status tda_landscape_batch(tda_ctx* ctx, const double* dgm, const int* cnt, int n_dgm, int cap,
                               const double* grid, int n_grid, int n_levels, double* out);

/* ---- Euler characteristic curves and simplex-count curves of Rips complexes ------------
 * The Euler characteristic of the clique (Vietoris-Rips) complex of a window as the scale sweeps a grid, and the simplex
 * counts it is made of: the summary of Santos et al. (2019) for functional brain networks, and the Euler characteristic
 * curve of Dlotko and Gurnari.  It is the one output here that looks above the triangles (K = 3: tetrahedra).  The
 * contract is this text; tests/euler_ref.py evaluates it.
 *   Keys.       A window has n vertices and float32 keys k[a][b], a > b: THE KEYS THE RIPS ENTRY POINTS USE for the same
 *               input, so curve and diagram describe one complex.
 *                 Distance matrices (n_win, n, n) float64, 1 <= n <= TDA_MAX_POINTS.  symmetrise = 1:
 *                   v = (D[a][b] + D[b][a]) / 2; if v < 0 then v = 0; k = (float)v.  symmetrise = 0: k = (float)D[b][a],
 *                   the entry (i, j) with i < j, as tda_rips_dm_batch words it.
 *                 Point clouds, in the two forms of the cloud Rips entry points: explicit (n_win, p_cap, dim) clouds with
 *                   n_pts and normalise (tda_cloud_rips_batch), or Takens windows with tau, dim <= TDA_MAX_DIM and
 *                   subsample (tda_takens_rips_batch: always normalised).  Per-column min-max (scripts/utils.py:127-130,
 *                   range 0 -> 1), then sklearn's distance: d2 = -2 x.y (x.y = fma(x2, y2, fma(x1, y1, x0 * y0)) and so
 *                   on), d2 += |x|^2, d2 += |y|^2 with x the point of larger index, d2 = 0 unless d2 > 0, sqrt, (float).
 *   Grid.       t[g], g < n_grid: float64, 1 <= n_grid <= TDA_MAX_GRID, any values in any order.
 *   Presence.   Edge {a, b} is present at g iff k <= (float)thresh and (double)k <= t[g]: plain IEEE comparisons, so a NaN
 *               key or a NaN grid point makes the edge absent; inclusive, so a grid point equal to a key has the edge.
 *   Counts.     f_j(g), j = 0..K: the number of (j + 1)-subsets of the vertices whose pairs are all present at g;
 *               f_0 = n.  K = max_dim, 1 <= K <= TDA_EC_MAX_DIM.  chi(g) = sum_j (-1)^j f_j(g): the Euler characteristic
 *               of the K-skeleton of the Rips complex at scale min(t[g], thresh).
 *   Outputs.    counts (n_win, K + 2, n_grid) int32: rows f_0 .. f_K, then chi (C(128, 4) = 10,668,000 fits).
 *               status (n_win) int32: 0 for distance matrices; the cloud forms write TDA_WIN_DEGENERATE (fewer than 3
 *               points) or TDA_WIN_TOO_LARGE (more than min(p_cap, TDA_MAX_POINTS) points, or tau < 1) exactly where the
 *               cloud Rips entry points do, and such a window's block of counts is all zeros.  n_points (nullable): as
 *               tda_takens_rips_batch.
 *   Means.      tda_euler_mean: mean (n_seg, K + 2, n_grid) float64.  Over the windows seg_off[g] <= w < seg_off[g + 1]
 *               whose status_in word has no bit of skip_mask (status_in may be NULL), every entry is
 *               (double)S / (double)m, S the exact int64 sum of the kept windows' int32 values and m their number; m = 0
 *               gives NaN.  seg_off = NULL: every window is its own group and n_seg must be n_win.  The byte pattern of
 *               np.mean(stack, axis=0) on the integer rows.
 *   Limits.     n, p_cap (>= 1), n_t (>= 1), dim, n_grid or max_dim out of range, or n_seg != n_win without a table, is
 *               TDA_ERR_INVALID with a message in tda_last_error; nothing is launched or written.
 *   Determinism.  The outputs are the integers of this text.  A window alone and inside a batch give the same bytes.  Every
 *               loop bound is known before the loop starts (n, n_grid, a popcount); no polls, no atomics.
 * The _dev forms only enqueue on `stream` and allocate nothing.  The host forms stage every buffer. */
#define TDA_EC_MAX_DIM 3
tda_status tda_euler_dm_batch_dev(tda_ctx* ctx, const double* dm, int n_win, int n, double thresh, int symmetrise,
                                  const double* grid, int n_grid, int max_dim, int* counts, int* status, void* stream);
tda_status tda_euler_dm_batch(tda_ctx* ctx, const double* dm, int n_win, int n, double thresh, int symmetrise,
                              const double* grid, int n_grid, int max_dim, int* counts, int* status);
tda_status tda_euler_cloud_batch_dev(tda_ctx* ctx, const double* pc, const int* n_pts, int n_win, int p_cap, int dim,
                                     int normalise, double thresh, const double* grid, int n_grid, int max_dim,
                                     int* counts, int* status, void* stream);
tda_status tda_euler_cloud_batch(tda_ctx* ctx, const double* pc, const int* n_pts, int n_win, int p_cap, int dim,
                                 int normalise, double thresh, const double* grid, int n_grid, int max_dim,
                                 int* counts, int* status);
tda_status tda_euler_takens_batch_dev(tda_ctx* ctx, const double* win, const int* tau, int n_win, int n_t, int dim,
                                      int subsample, double thresh, const double* grid, int n_grid, int max_dim,
                                      int* counts, int* n_points, int* status, void* stream);
tda_status tda_euler_takens_batch(tda_ctx* ctx, const double* win, const int* tau, int n_win, int n_t, int dim,
                                  int subsample, double thresh, const double* grid, int n_grid, int max_dim,
                                  int* counts, int* n_points, int* status);
tda_status tda_euler_mean_dev(tda_ctx* ctx, const int* counts, int n_win, int max_dim, int n_grid, const int* seg_off,
                              int n_seg, const int* status_in, int skip_mask, double* mean, void* stream);
tda_status tda_euler_mean(tda_ctx* ctx, const int* counts, int n_win, int max_dim, int n_grid, const int* seg_off,
                          int n_seg, const int* status_in, int skip_mask, double* mean);

/* ---- Network curves: graph measures of the thresholded graphs ----------------------------
 * The conventional graph measures of the functional-connectivity literature -- degree, clustering coefficient and
 * transitivity, characteristic path length, global efficiency, number and size of the components -- of the graph G_g of a
 * window at every point g of a grid of scales: the baseline beside the topological summaries of the same filtration.  The
 * contract is this text; tests/network_ref.py evaluates it twice.
 *   Inputs.     The input forms, keys k[a][b], grid t[g], presence rule, refusals and status words are those of "Euler
 *               characteristic curves" above, word for word: G_g has the vertices 0..n-1 and the edge {a, b} exactly when
 *               k <= (float)thresh and (double)k <= t[g].  Curve, Euler curve and diagram describe one filtration.
 *   Notation.   deg(v), N(v): degree and neighbours of v in G_g.  h(u, v): the number of edges of a shortest path, undefined
 *               when u and v are not connected.  tri(v): the number of pairs {u, w} within N(v) whose edge is present.
 *               p_d: the number of unordered pairs {u, v} with h(u, v) = d.  C(m, 2) = m (m - 1) / 2.
 *   counts      (n_win, TDA_NET_ROWS, n_grid) int32, the rows
 *                 0 edges       number of edges
 *                 1 isolated    number of v with deg(v) = 0
 *                 2 max_degree  largest degree
 *                 3 wedges      sum_v C(deg(v), 2)                                   (at most 128 C(127, 2) = 1,024,128)
 *                 4 triangles   (sum_v tri(v)) / 3
 *                 5 components  number of connected components
 *                 6 largest     size of the largest component
 *                 7 pairs       unordered connected pairs u != v, sum_d p_d
 *                 8 hops        sum over those pairs of h          (at most (n - 1) n (n + 1) / 6 = 349,504 at n = 128)
 *                 9 diameter    largest h; 0 without a pair
 *   measures    (n_win, TDA_NET_MEASURES, n_grid) float64.  Each value is a function of the integers in one order of IEEE
 *               operations (no contraction):
 *                 0 transitivity  wedges ? (double)(3 * triangles) / (double)wedges : 0.0
 *                 1 clustering    Watts-Strogatz mean local clustering: c_v = deg(v) < 2 ? 0.0 :
 *                                 (double)tri(v) / (double)C(deg(v), 2); S = 0.0; S += c_0; S += c_1; ... in ascending v;
 *                                 the value is S / (double)n
 *                 2 efficiency    Latora-Marchiori global efficiency: n < 2 ? 0.0 :
 *                                 (sum_{d = 1, 2, ...} (double)p_d / (double)d) / (double)C(n, 2), d ascending, the sum
 *                                 starting from 0.0 (terms past the diameter are +0.0)
 *                 3 path_length   characteristic path length over the connected pairs: pairs ? (double)hops /
 *                                 (double)pairs : 0.0
 *   nodal       (nullable) (n_win, TDA_NET_NODAL, n_grid, n_node) int32, n_node = n (matrices), p_cap (clouds),
 *               TDA_MAX_POINTS (Takens): the `part` convention of the generators.  The rows: 0 degree deg(v), 1 triangles
 *               tri(v), 2 reach (the vertices u != v connected to v), 3 farness sum_u h(v, u), 4 eccentricity max_u h(v, u)
 *               (0 when there is none).  Entries with v >= n are 0.  A NULL nodal changes no byte of the other outputs.
 *   status, n_points  as the Euler entry points.  A refused window (TDA_WIN_DEGENERATE, TDA_WIN_TOO_LARGE, tau < 1) has
 *               all-zero blocks, 0.0 in measures.
 *   Means.      tda_network_mean: mean_counts (n_seg, TDA_NET_ROWS, n_grid), mean_measures (n_seg, TDA_NET_MEASURES,
 *               n_grid), mean_nodal (n_seg, TDA_NET_NODAL, n_grid, n_node), all float64; each input is nullable together
 *               with its mean.  Groups, status_in, skip_mask and seg_off = NULL as tda_euler_mean.  The integer blocks:
 *               (double)S / (double)m with S the exact int64 sum of the kept windows.  measures: S = 0.0, then S += the
 *               kept windows' values in ascending window order, S / (double)m.  m = 0 gives NaN.
 *   Limits.     Those of the Euler entry points, without max_dim; for the means n_seg != n_win without a table, an input
 *               without its mean or the reverse, or n_node < 1 with nodal: TDA_ERR_INVALID with a message in
 *               tda_last_error; nothing is launched or written.
 *   Determinism.  A window alone and inside a batch give the same bytes.  No atomics, no polls.  Every loop is bounded
 *               before it starts by n, n_grid, n_node or a popcount; the level loop of the search by n - 1.
 * The _dev forms only enqueue on `stream` and allocate nothing.  The host forms stage every buffer. */
#define TDA_NET_ROWS     10
#define TDA_NET_MEASURES 4
#define TDA_NET_NODAL    5
tda_status tda_network_dm_batch_dev(tda_ctx* ctx, const double* dm, int n_win, int n, double thresh, int symmetrise,
                                    const double* grid, int n_grid, int* counts, double* measures, int* nodal, int* status,
                                    void* stream);
tda_status tda_network_dm_batch(tda_ctx* ctx, const double* dm, int n_win, int n, double thresh, int symmetrise,
                                const double* grid, int n_grid, int* counts, double* measures, int* nodal, int* status);
tda_status tda_network_cloud_batch_dev(tda_ctx* ctx, const double* pc, const int* n_pts, int n_win, int p_cap, int dim,
                                       int normalise, double thresh, const double* grid, int n_grid, int* counts,
                                       double* measures, int* nodal, int* status, void* stream);
tda_status tda_network_cloud_batch(tda_ctx* ctx, const double* pc, const int* n_pts, int n_win, int p_cap, int dim,
                                   int normalise, double thresh, const double* grid, int n_grid, int* counts,
                                   double* measures, int* nodal, int* status);
tda_status tda_network_takens_batch_dev(tda_ctx* ctx, const double* win, const int* tau, int n_win, int n_t, int dim,
                                        int subsample, double thresh, const double* grid, int n_grid, int* counts,
                                        double* measures, int* nodal, int* n_points, int* status, void* stream);
tda_status tda_network_takens_batch(tda_ctx* ctx, const double* win, const int* tau, int n_win, int n_t, int dim,
                                    int subsample, double thresh, const double* grid, int n_grid, int* counts,
                                    double* measures, int* nodal, int* n_points, int* status);
tda_status tda_network_mean_dev(tda_ctx* ctx, const int* counts, const double* measures, const int* nodal, int n_win,
                                int n_grid, int n_node, const int* seg_off, int n_seg, const int* status_in, int skip_mask,
                                double* mean_counts, double* mean_measures, double* mean_nodal, void* stream);
tda_status tda_network_mean(tda_ctx* ctx, const int* counts, const double* measures, const int* nodal, int n_win,
                            int n_grid, int n_node, const int* seg_off, int n_seg, const int* status_in, int skip_mask,
                            double* mean_counts, double* mean_measures, double* mean_nodal);

/* ---- Recurrence curves: recurrence quantification of the windows in time order ------------
 * Recurrence quantification analysis (Zbilut & Webber 1992; Marwan et al. 2007) of a window at every point g of a grid of
 * scales: the conventional baseline beside the topological summaries of a delay embedding.  The recurrence plot at scale
 * t[g] is the adjacency matrix of the 1-skeleton of the Rips complex at t[g] on the vertices in time order; the network
 * curves forget that order, these curves read it.  The contract is this text; tests/recurrence_ref.py evaluates it twice.
 *   Inputs.     The input forms, keys k[a][b], grid t[g], presence rule, refusals and status words are those of "Euler
 *               characteristic curves" above, word for word.  Three further parameters: theiler, l_min, v_min.
 *               For a window with n points R_g[i][j] = 1 iff i != j, |i - j| >= theiler and the edge {i, j} is present at
 *               g: k <= (float)thresh and (double)k <= t[g].  R_g is symmetric with a zero band of half-width theiler - 1
 *               around the diagonal; theiler = 1 removes the main diagonal only.  The vertex index is the time index: the
 *               row of a cloud, point i of a Takens window (with subsample = s one step is s samples).
 *   Lines.      A diagonal line of length l is a maximal run R[i+m][j+m] = 1, m = 0..l-1, on one diagonal j - i = const,
 *               counted over the whole matrix: both triangles contribute, every line above the diagonal has its mirror
 *               below.  A vertical line is a maximal run of consecutive i with R[i][j] = 1 in one column j; the zero band
 *               interrupts it.  HD(l), HV(l): the numbers of such lines of length exactly l >= 1.
 *   counts      (n_win, TDA_RQA_ROWS, n_grid) int32, the rows
 *                 0 recurrences   sum R                                                        (at most 128 * 127)
 *                 1 diag_lines    sum_{l >= l_min} HD(l)
 *                 2 diag_points   sum_{l >= l_min} l HD(l)
 *                 3 diag_longest  largest l with HD(l) > 0, whatever l_min; 0 without one
 *                 4 vert_lines    sum_{l >= v_min} HV(l)
 *                 5 vert_points   sum_{l >= v_min} l HV(l)
 *                 6 vert_longest  largest l with HV(l) > 0, whatever v_min; 0 without one
 *   measures    (n_win, TDA_RQA_MEASURES, n_grid) float64.  Each value is a function of the integers in one order of IEEE
 *               operations (no contraction):
 *                 0 recurrence_rate  N ? (double)recurrences / (double)N : 0.0, N = theiler <= n ?
 *                                    (n - theiler)(n - theiler + 1) : 0, the ordered pairs outside the band
 *                 1 determinism      recurrences ? (double)diag_points / (double)recurrences : 0.0
 *                 2 diag_mean        diag_lines ? (double)diag_points / (double)diag_lines : 0.0
 *                 3 diag_entropy     S = 0.0; for l = l_min, l_min + 1, ... ascending with HD(l) > 0:
 *                                    p = (double)HD(l) / (double)diag_lines; S = S - p * log(p).  The value is S; 0.0
 *                                    without lines
 *                 4 laminarity       recurrences ? (double)vert_points / (double)recurrences : 0.0
 *                 5 trapping_time    vert_lines ? (double)vert_points / (double)vert_lines : 0.0
 *                 6 vert_entropy     as row 3, with HV, v_min and vert_lines
 *   hist        (nullable) (n_win, 2, n_grid, n_hist) int32, n_hist = n (matrices), p_cap (clouds), TDA_MAX_POINTS
 *               (Takens): the `nodal` convention of the network curves.  hist[., 0, ., l - 1] = HD(l),
 *               hist[., 1, ., l - 1] = HV(l); zeros past the window's own n.  A NULL hist changes no byte of the other
 *               outputs.
 *   status, n_points  as the Euler entry points.  A refused window (TDA_WIN_DEGENERATE, TDA_WIN_TOO_LARGE, tau < 1) has
 *               all-zero blocks, 0.0 in measures.
 *   Means.      tda_recurrence_mean: mean_counts (n_seg, TDA_RQA_ROWS, n_grid), mean_measures (n_seg, TDA_RQA_MEASURES,
 *               n_grid), mean_hist (n_seg, 2, n_grid, n_hist), all float64; each input is nullable together with its
 *               mean.  The rules are those of tda_network_mean: groups, status_in, skip_mask and seg_off = NULL as there;
 *               the integer blocks (double)S / (double)m with S the exact int64 sum of the m kept windows; measures
 *               S = 0.0, then S += the kept windows' values in ascending window order, S / (double)m.  m = 0 gives NaN.
 *   Limits.     Those of the Euler entry points, without max_dim; theiler, l_min and v_min in [1, TDA_MAX_POINTS]; for the
 *               means those of tda_network_mean with n_hist for n_node.  Anything else: TDA_ERR_INVALID with a message in
 *               tda_last_error; nothing is launched or written.
 *   Determinism.  Everything but rows 3 and 6 of measures is bytes; those two agree with the written sum to the rounding
 *               of log (DESIGN.md 3.25 has the measured bar), and a histogram with a single non-zero bin gives exactly
 *               0.0.  A window alone and inside a batch give the same bytes.  No atomics, no polls.  Every loop is bounded
 *               before it starts by n, n_grid, n_hist or a popcount.
 * The _dev forms only enqueue on `stream` and allocate nothing.  The host forms stage every buffer. */
#define TDA_RQA_ROWS     7
#define TDA_RQA_MEASURES 7
tda_status tda_recurrence_dm_batch_dev(tda_ctx* ctx, const double* dm, int n_win, int n, double thresh, int symmetrise,
                                       const double* grid, int n_grid, int theiler, int l_min, int v_min, int* counts,
                                       double* measures, int* hist, int* status, void* stream);
tda_status tda_recurrence_dm_batch(tda_ctx* ctx, const double* dm, int n_win, int n, double thresh, int symmetrise,
                                   const double* grid, int n_grid, int theiler, int l_min, int v_min, int* counts,
                                   double* measures, int* hist, int* status);
tda_status tda_recurrence_cloud_batch_dev(tda_ctx* ctx, const double* pc, const int* n_pts, int n_win, int p_cap, int dim,
                                          int normalise, double thresh, const double* grid, int n_grid, int theiler,
                                          int l_min, int v_min, int* counts, double* measures, int* hist, int* status,
                                          void* stream);
tda_status tda_recurrence_cloud_batch(tda_ctx* ctx, const double* pc, const int* n_pts, int n_win, int p_cap, int dim,
                                      int normalise, double thresh, const double* grid, int n_grid, int theiler, int l_min,
                                      int v_min, int* counts, double* measures, int* hist, int* status);
tda_status tda_recurrence_takens_batch_dev(tda_ctx* ctx, const double* win, const int* tau, int n_win, int n_t, int dim,
                                           int subsample, double thresh, const double* grid, int n_grid, int theiler,
                                           int l_min, int v_min, int* counts, double* measures, int* hist, int* n_points,
                                           int* status, void* stream);
tda_status tda_recurrence_takens_batch(tda_ctx* ctx, const double* win, const int* tau, int n_win, int n_t, int dim,
                                       int subsample, double thresh, const double* grid, int n_grid, int theiler, int l_min,
                                       int v_min, int* counts, double* measures, int* hist, int* n_points, int* status);
tda_status tda_recurrence_mean_dev(tda_ctx* ctx, const int* counts, const double* measures, const int* hist, int n_win,
                                   int n_grid, int n_hist, const int* seg_off, int n_seg, const int* status_in,
                                   int skip_mask, double* mean_counts, double* mean_measures, double* mean_hist,
                                   void* stream);
tda_status tda_recurrence_mean(tda_ctx* ctx, const int* counts, const double* measures, const int* hist, int n_win,
                               int n_grid, int n_hist, const int* seg_off, int n_seg, const int* status_in, int skip_mask,
                               double* mean_counts, double* mean_measures, double* mean_hist);

/* ---- Generators and representative cycles of Rips persistence pairs ---------------------
 * Which simplices stand behind a row of a diagram, and a cycle that represents every H1 row: the counterpart of
 * ripser(..., do_cocycles=True) and of GUDHI's flag_persistence_generators, for the question "which channels carry the
 * loop".  The Rips kernels are not asked: the simplices are recovered afterwards from the keys and the rows they wrote,
 * by a local rule.  The contract is this text; tests/generators_ref.py evaluates it three times.
 *   Keys.       k[a][b], a > b: the float32 keys of the Rips entry points for the same input, as "Euler characteristic
 *               curves" above words them (distance matrices with symmetrise; clouds with n_pts and normalise; Takens
 *               windows with tau, dim, subsample).  The edges are the pairs with k <= (float)thresh (a NaN key is no
 *               edge), ordered by (key, a, b): among equal keys by the flat index a (a - 1) / 2 + b.
 *   Kinds.      G_e is the graph of the edges that precede e = (a, b) in that order.  cn(e): some vertex v has both (a, v)
 *               and (b, v) in G_e.  conn(e): a and b are connected in G_e.  Forest edges F = {e : !conn(e)} (Kruskal's
 *               edges under that order), birth edges B = {e : conn(e) and !cn(e)}, death edges K = {e : cn(e)}.
 *               An edge of K is the youngest edge of a triangle that enters with it and is paired at zero persistence, so
 *               every H1 row (b, d), d > b, has its birth edge in B with key b and the youngest edge of its killing
 *               triangle in K with key d; the finite H0 rows pair, in ascending death order, with the edges of F of
 *               non-zero key (DESIGN.md 3.22 has the proofs).
 *   Rows in.    The diagrams of the same windows as the Rips entry points wrote them: h0 (n_win, h0_cap, 2) with h0_cnt
 *               (both nullable when h0_edge is NULL), h1 (n_win, h1_cap, 2) with h1_cnt, h1_cap >= 1.  The rows looked at
 *               are the first min(count, cap).  rips_status (nullable): a window whose word has a bit of skip_mask gets the
 *               fill values only.
 *   h1_gen      (n_win, h1_cap, 4) int16 [birth_a, birth_b, death_a, death_b], a > b.  A maximal run of consecutive rows
 *               with equal birth x takes the edges of B with (double)k == x in order, one per row.  The death edge of a
 *               row with d != +inf is the first edge of K with (double)k == d; a row with d = +inf has -1, -1.
 *   h1_flag     (n_win, h1_cap) int32.  TDA_GEN_BIRTH_TIED: the run has a different number of candidates in B than rows.
 *               TDA_GEN_DEATH_TIED: more than one candidate in K.  TDA_GEN_NO_EDGE: the row's place in its run is past the
 *               candidates of B, or d != +inf has no candidate in K -- the diagram is not this input's; the row's edges
 *               and cycle are -1, its length 0, and it carries no TDA_GEN_CYCLE_TRUNCATED.  TDA_GEN_CYCLE_TRUNCATED: the
 *               cycle is longer than cyc_cap; cyc holds its first cyc_cap vertices and cyc_len the true length.
 *   cyc, cyc_len  (n_win, h1_cap, cyc_cap) int16 (nullable: then part must be NULL too; lengths and flags are written as
 *               if it were there) and (n_win, h1_cap) int32, 4 <= cyc_cap <= TDA_MAX_POINTS.  Breadth-first
 *               search from birth_b in G_e in level sets; the parent of a vertex is the lowest-numbered adjacent vertex of
 *               the previous level.  The cycle is birth_a, parent(birth_a), ..., birth_b: with e it is a closed walk whose
 *               youngest edge is e, so it is born at b and becomes a boundary-equivalent of older cycles exactly at d.
 *               At least 4 vertices (!cn(e) rules out 3).  -1 fills the rest of the row.
 *   part        (nullable) (n_win, n_part) float64, n_part = n (matrices), p_cap (clouds), TDA_MAX_POINTS (Takens).
 *               part[v] = +0.0, then in row order += d - b for every row with a finite d, flag 0 and v on its cycle.
 *               Entries at and above the window's vertex count are 0.
 *   h0_edge     (nullable) (n_win, h0_cap, 2) int16 [a, b], a > b.  A maximal run of consecutive H0 rows with equal death x
 *               takes the edges of F with (double)k == x in order, one per row; a row past the candidates, and every row
 *               with death +inf, has -1, -1.  On the rows of this input the counts agree: exact under ties as well.
 *   Fill.       Rows at and above min(count, cap), and every row of a skipped window or of one whose status is not 0:
 *               h1_gen, cyc, h0_edge -1; h1_flag, cyc_len 0; part 0.
 *   work        (nullable) (n_win, 4, 2) int32: per wave of the window's workgroup, the searches it ran and their levels
 *               (for tools/generators_bench.py; no part of the contract beyond "searches <= |F| + |B|").
 *   status      (n_win) int32: 0 for matrices; TDA_WIN_DEGENERATE / TDA_WIN_TOO_LARGE exactly where the Euler entry points
 *               set them.  n_points (nullable): as tda_takens_rips_batch.
 *   Means.      tda_generators_mean: mean (n_seg, n) float64 of part (n_win, n).  Per group and vertex S = +0.0, then
 *               S += part[w][v] for the windows seg_off[g] <= w < seg_off[g + 1] in order whose status_in word (nullable)
 *               has no bit of skip_mask; S / (double)m, NaN for m = 0.  seg_off = NULL: n_seg must be n_win.
 *   Limits.     n in [1, TDA_MAX_POINTS], p_cap, n_t >= 1, dim in [1, TDA_MAX_DIM], cyc_cap in [4, TDA_MAX_POINTS],
 *               h1_cap >= 1, h0_edge without h0 / h0_cnt / h0_cap >= 1, part without cyc, n < 1 or n_seg != n_win without a table for the
 *               means: TDA_ERR_INVALID with a message in tda_last_error; nothing is launched or written.
 *   Determinism.  The outputs are the integers (and the ordered float64 sums) of this text.  A window alone and inside a
 *               batch give the same bytes.  Every loop bound is known before the loop starts; no polls, no atomics.
 * The _dev forms only enqueue on `stream` and allocate nothing.  The host forms stage every buffer. */
#define TDA_GEN_BIRTH_TIED      1
#define TDA_GEN_DEATH_TIED      2
#define TDA_GEN_CYCLE_TRUNCATED 4
#define TDA_GEN_NO_EDGE         8
tda_status tda_generators_dm_batch_dev(tda_ctx* ctx, const double* dm, int n_win, int n, double thresh, int symmetrise,
                                       const double* h0, int h0_cap, const int* h0_cnt,
                                       const double* h1, int h1_cap, const int* h1_cnt, const int* rips_status,
                                       int skip_mask, int cyc_cap, short* h1_gen, int* h1_flag, short* cyc, int* cyc_len,
                                       double* part, short* h0_edge, int* work, int* status, void* stream);
tda_status tda_generators_dm_batch(tda_ctx* ctx, const double* dm, int n_win, int n, double thresh, int symmetrise,
                                   const double* h0, int h0_cap, const int* h0_cnt,
                                   const double* h1, int h1_cap, const int* h1_cnt, const int* rips_status,
                                   int skip_mask, int cyc_cap, short* h1_gen, int* h1_flag, short* cyc, int* cyc_len,
                                   double* part, short* h0_edge, int* work, int* status);
tda_status tda_generators_cloud_batch_dev(tda_ctx* ctx, const double* pc, const int* n_pts, int n_win, int p_cap, int dim,
                                          int normalise, double thresh,
                                          const double* h0, int h0_cap, const int* h0_cnt,
                                          const double* h1, int h1_cap, const int* h1_cnt, const int* rips_status,
                                          int skip_mask, int cyc_cap, short* h1_gen, int* h1_flag, short* cyc, int* cyc_len,
                                          double* part, short* h0_edge, int* work, int* status, void* stream);
tda_status tda_generators_cloud_batch(tda_ctx* ctx, const double* pc, const int* n_pts, int n_win, int p_cap, int dim,
                                      int normalise, double thresh,
                                      const double* h0, int h0_cap, const int* h0_cnt,
                                      const double* h1, int h1_cap, const int* h1_cnt, const int* rips_status,
                                      int skip_mask, int cyc_cap, short* h1_gen, int* h1_flag, short* cyc, int* cyc_len,
                                      double* part, short* h0_edge, int* work, int* status);
tda_status tda_generators_takens_batch_dev(tda_ctx* ctx, const double* win, const int* tau, int n_win, int n_t, int dim,
                                           int subsample, double thresh,
                                           const double* h0, int h0_cap, const int* h0_cnt,
                                           const double* h1, int h1_cap, const int* h1_cnt, const int* rips_status,
                                           int skip_mask, int cyc_cap, short* h1_gen, int* h1_flag, short* cyc, int* cyc_len,
                                           double* part, short* h0_edge, int* work, int* n_points, int* status,
                                           void* stream);
tda_status tda_generators_takens_batch(tda_ctx* ctx, const double* win, const int* tau, int n_win, int n_t, int dim,
                                       int subsample, double thresh,
                                       const double* h0, int h0_cap, const int* h0_cnt,
                                       const double* h1, int h1_cap, const int* h1_cnt, const int* rips_status,
                                       int skip_mask, int cyc_cap, short* h1_gen, int* h1_flag, short* cyc, int* cyc_len,
                                       double* part, short* h0_edge, int* work, int* n_points, int* status);
tda_status tda_generators_mean_dev(tda_ctx* ctx, const double* part, int n_win, int n, const int* seg_off, int n_seg,
                                   const int* status_in, int skip_mask, double* mean, void* stream);
tda_status tda_generators_mean(tda_ctx* ctx, const double* part, int n_win, int n, const int* seg_off, int n_seg,
                               const int* status_in, int skip_mask, double* mean);

/* ---- Frechet means of diagrams, per group ---------------------------------------------
 * The mean diagram of a group in the order-2 Wasserstein metric and the group's variance around it: the algorithm of
 * Turner, Mileyko, Mukherjee and Harer (2014), with the update rule of GUDHI's lagrangian_barycenter.  The contract is this
 * text; tests/frechet_ref.py evaluates it on the CPU.
 *   Input.    A group is the diagrams seg_off[g] <= w < seg_off[g + 1], in buffer order.  Diagrams whose status_in word has
 *             a bit of skip_mask are left out, as in tda_landscape_mean_dev (status_in may be NULL).  The kept ones are
 *             X_1 .. X_m, in buffer order.  Of every diagram only the rows i < min(cnt, cap) with both values finite
 *             count, in row order.  An empty diagram stays empty: it is not replaced by {(0,0)}.  The two are equivalent
 *             for this cost (a point on the diagonal has diagonal cost 0 and no negative gain), so nothing is lost.
 *   Costs.    Those of tda_wasserstein_q_batch with order 2 and TDA_GROUND_L2, operation for operation, no multiply-add:
 *               dx = fabs(y_b - x_b), dy = fabs(y_d - x_d), C = (dx * dx) + (dy * dy);
 *               diagonal cost 0.5 * (p * p) with p = d - b;
 *               gain g = min(0, (C - s) - t), where s is the diagonal cost of the point of the diagram with FEWER rows
 *               (the row role; Y on a tie) and t that of the other point.
 *             A matched cell is a real match iff its computed gain is < 0.
 *   Start.    Y^0 is the finite rows of X_1, in row order.
 *   One iteration on Y = Y^t with n rows:
 *     1. For i = 1..m an optimal partial matching of Y and X_i (the minimum of the summed gains; with n = 0 or X_i empty
 *        nothing is matched).  V_i is its value from the original costs: a term per row j of Y (C of its real match, else
 *        its diagonal cost) and a term per row of X_i without a real match (its diagonal cost).  The terms are added into
 *        64 partial sums -- the Y terms to sum (j mod 64) in ascending j, then the X terms to sum (row mod 64) in
 *        ascending row -- and the 64 sums are folded pairwise at distances 32, 16, 8, 4, 2, 1 (a[l] + a[l xor distance]).
 *        F_t = V_1 + V_2 + ... in the order of i, starting from 0.
 *     2. For every row j of Y: k_j is the number of i in which j has a real match, sb_j and sd_j the sums of the matched
 *        births and deaths, added in ascending i, starting from 0.
 *     3. A row with k_j = 0 is dropped.  Otherwise wb = sb / k, wd = sd / k; if k = m the new row is (wb, wd), else
 *        h = 0.5 * (wb + wd) and the new row is (((k * wb) + ((m - k) * h)) / m, ((k * wd) + ((m - k) * h)) / m).
 *     4. Every row x of every X_i without a real match spawns one row by the same formula with k = 1, wb = x_b, wd = x_d.
 *     5. Y^{t+1} is the surviving rows in the order of j, then the spawned rows in the order (i, row).
 *   Stop.     Converged at t if Y^{t+1} has the row count and the bytes of Y^t (the new rows depend only on the matchings
 *             and the X_i, so an unchanged matching gives unchanged bytes).  The loop runs for t = 0 .. max_iter - 1,
 *             1 <= max_iter <= TDA_FM_MAX_ITER.  The output is always the last iterate that was matched, Y^t with its own
 *             energy, never an unmatched Y^{t+1}.  Without convergence within the bound the group carries
 *             TDA_WIN_NOT_CONVERGED and keeps its output.
 *   Outputs per group.  mean (cap_out, 2): the rows of Y^t (rows beyond the count are not written); mean_cnt: the true
 *             row count; var = F_t / m, the Frechet variance of the output; iters = t + 1; status.
 *   Limits.   m = 0: count 0, var NaN, iters 0, status 0.  m > 64, a diagram with more than TDA_FM_MAX_POINTS finite rows,
 *             or a Y^{t+1} formed with more than TDA_FM_MAX_POINTS rows (in the last iteration too): TDA_WIN_TOO_LARGE,
 *             count 0, var NaN.  A solver loop bound hit: TDA_WIN_NOT_CONVERGED, count 0, var NaN.  count > cap_out:
 *             TDA_WIN_H1_TRUNCATED, the true count, the first cap_out rows, var and iters valid.
 *             cap >= 1, cap_out >= 1, 1 <= max_iter <= TDA_FM_MAX_ITER, and n_seg = n_dgm when seg_off is NULL; anything
 *             else is TDA_ERR_INVALID and nothing is launched.  Table entries are clamped to [0, n_dgm].
 *   Bounds.   Every loop of the kernel has a bound known before it starts: max_iter, the group's size, the row limits and
 *             the solver's own bounds.  Nothing can spin.
 *   Exactness.  Every cost and every update is one correctly rounded float64 operation of this text and the sums run in
 *             the stated orders.  Where every optimal matching met along the way is unique, the output equals a CPU
 *             evaluation of this text bit for bit; otherwise both are valid runs of the same algorithm.
 *   Determinism.  No atomics on floating point.  A group alone and the same group inside a batch give the same bytes.  With
 *             seg_off = NULL every diagram is its own group; the mean of a diagram whose rows all have d > b is then its
 *             finite rows, with var 0 and iters 1.
 * The _dev form only enqueues on `stream` and allocates nothing.  mean (n_seg, cap_out, 2) float64; mean_cnt, iters, status
 * (n_seg) int32; var (n_seg) float64. */
#define TDA_FM_MAX_ITER   64
#define TDA_FM_MAX_POINTS 512
tda_status tda_frechet_mean_dev(tda_ctx* ctx, const double* dgm, const int* cnt, int cap, int n_dgm,
                                const int* seg_off, int n_seg, const int* status_in, int skip_mask, int max_iter,
                                double* mean, int* mean_cnt, int cap_out, double* var, int* iters, int* status,
                                void* stream);
tda_status tda_frechet_mean_batch(tda_ctx* ctx, const double* dgm, const int* cnt, int n_dgm, int cap,
                                  const int* seg_off, int n_seg, const int* status_in, int skip_mask, int max_iter,
                                  double* mean, int* mean_cnt, int cap_out, double* var, int* iters, int* status);

/* ---- Persistence images, averaged per group -----------------------------------------
 * The image of a diagram is the bivariate normal density with covariance sigma^2 I, placed on every point of the diagram in
 * birth/persistence coordinates, weighted by a power of the persistence and integrated over every pixel of a grid.  This
 * is how persim's PersistenceImager is understood; persim is not installed anywhere this project runs, so no parity with
 * it is claimed.  The contract is this text.
 * A diagram has rows (b_i, d_i), i < min(cnt, cap), float64.
 *   Rows used.    F is the set of rows with both values finite (the mask of tda_features_batch).  Essential classes never
 *                 enter an image.
 *   Coordinates.  A point sits at (b_i, p_i) with p_i = d_i - b_i, one IEEE subtraction.
 *   Edges.        xe holds n_x + 1 birth edges and ye holds n_y + 1 persistence edges, float64 arrays passed by the
 *                 caller.  The kernel never computes an edge.
 *   Width.        sigma is a float64 > 0.  s = sigma * 1.4142135623730951, one multiplication.
 *   Weight.       power is in {0, 1, 2}.  The weight w_i is 1.0, p_i or p_i * p_i.
 *   CDF.          Phi(e, c) = 0.5 * erfc(-((e - c) / s)).
 *   Factors.      fx_i[c] = Phi(xe[c+1], b_i) - Phi(xe[c], b_i)
 *                 fy_i[r] = Phi(ye[r+1], p_i) - Phi(ye[r], p_i)
 *   Image.        I[r, c] = sum over i in F of (w_i * fy_i[r]) * fx_i[c], shape (n_y, n_x).  Row r is the persistence
 *                 axis.  An empty F gives all zeros.
 * Group mean, for the diagrams seg_off[g] <= w < seg_off[g + 1]: diagrams whose status word has a bit of skip_mask are
 * left out; the result is (sum of the kept diagrams' images) / n_kept, and NaN in every element when n_kept = 0.  With
 * seg_off = NULL every diagram is its own group and n_seg must be n_dgm.  Table entries are clamped to [0, n_dgm], as in
 * tda_landscape_mean_dev.
 * Order of additions.  d >= b holds for Rips rows, so every term is non-negative and the order of the additions is not
 * part of the contract.  It is deterministic: no atomics; the additions that make a pixel depend only on the group's own
 * diagrams and the parameters, not on the launch shape or on the other groups.  A recording alone and the same recording
 * inside a shard give the same bytes.
 * erfc is the device library's: the result agrees with a CPU evaluation of this text to rounding, not bit for bit.
 * Limits: 1 <= n_x, n_y <= TDA_MAX_IMAGE_SIDE; sigma finite and > 0; power in {0, 1, 2}; cap >= 1; anything else is
 * TDA_ERR_INVALID and nothing is launched.  The host form also rejects edges that are not finite and strictly ascending;
 * the _dev form cannot see the edges and applies the formula as written.
 * out: (n_seg, n_y, n_x) float64.  The _dev form only enqueues on `stream` and allocates nothing. */
#define TDA_MAX_IMAGE_SIDE 32
tda_status tda_image_mean_dev(tda_ctx* ctx, const double* dgm, const int* cnt, int cap, int n_dgm,
                              const int* seg_off, int n_seg, const int* status, int skip_mask,
                              const double* xe, int n_x, const double* ye, int n_y, double sigma, int power,
                              double* out, void* stream);
tda_status tda_image_batch(tda_ctx* ctx, const double* dgm, const int* cnt, int n_dgm, int cap,
                           const double* xe, int n_x, const double* ye, int n_y, double sigma, int power, double* out);

/* ---- Kernels on diagrams: persistence scale-space and weighted Gaussian ----------------
 * The persistence scale-space kernel (PSSK; Reininghaus, Huber, Bauer, Kwitt 2015; GUDHI's PersistenceScaleSpaceKernel) and
 * the persistence weighted Gaussian kernel (PWGK; Kusano, Fukumizu, Hiraoka 2016; GUDHI's PersistenceWeightedGaussianKernel),
 * between pairs of diagrams and between the mean embeddings of groups of diagrams.  GUDHI is not installed anywhere this
 * project runs, so no parity with it is claimed.  The contract is this text; tests/diagram_kernel_ref.py evaluates it.
 *   Rows.       A diagram has rows (b_i, d_i), i < min(cnt, cap), float64.  F is the set of rows with both values finite:
 *               the (0, inf) row of every H0 diagram never enters.  An empty F is the zero measure; it is NOT replaced by
 *               {(0,0)}.
 *   Parameters. All computed by the caller: ninv finite and < 0; mirror 0 or 1; scale finite; weight TDA_KW_ONE,
 *               TDA_KW_PERS or TDA_KW_ATAN; wc finite, used by TDA_KW_ATAN only.  The device never divides by sigma and
 *               never computes pi.
 *   Weights.    Once per row, never once per pair: p_i = d_i - b_i; w_i = 1.0 (TDA_KW_ONE), p_i (TDA_KW_PERS) or
 *               atan(wc * p_i) (TDA_KW_ATAN).  A weight that is not finite (a persistence that overflows) is outside
 *               the contract.
 *   Terms.      No multiply-add anywhere.  For i in F_A and j in F_B:
 *                 dx = b_i - b_j; dy = d_i - d_j; a1 = (dx * dx + dy * dy) * ninv; E1 = exp(a1)
 *                 ex = b_i - d_j; ey = d_i - b_j; a2 = (ex * ex + ey * ey) * ninv; E2 = exp(a2)      (mirror = 1 only)
 *                 t_ij = (w_i * w_j) * (E1 - E2), or (w_i * w_j) * E1 when mirror is 0.
 *               S(A, B) is the sum of all t_ij and K(A, B) = scale * S(A, B).  a1 and a2 are the same float64 on the GPU
 *               and in a CPU evaluation; only exp, atan and the order of the additions differ.  A row on the diagonal
 *               (b = d) has a1 = a2 bit for bit and adds exactly 0.0 when mirror is 1.
 *   Named.      PSSK(sigma): ninv = -1 / (8 sigma), mirror = 1, scale = 1 / (8 pi sigma), TDA_KW_ONE.
 *               PWGK(sigma, c): ninv = -1 / (2 sigma^2), mirror = 0, scale = 1, TDA_KW_ATAN with wc = c.
 *   Pairs.      k_ab = K(A, B), k_aa = K(A, A), k_bb = K(B, B); s = k_aa + k_bb; t = k_ab + k_ab; d2 = s - t;
 *               out = sqrt(d2 > 0 ? d2 : 0), the distance the kernel induces.  kvals (n_pairs, 3), nullable, receives
 *               [k_ab, k_aa, k_bb].  A pair index outside [0, n_a) or [0, n_b) gives NaN (in kvals too) and
 *               TDA_WIN_NO_PAIR, as tda_sliced_prepared_pairs_dev does; every other pair has status 0.  There is no limit
 *               on the rows of a diagram: the loops run over chunks.
 *   Gram.       The groups of set A are seg_off_a[g] <= w < seg_off_a[g + 1], those of set B likewise; seg_off = NULL makes
 *               every diagram its own group (n_seg must then be the number of diagrams); table entries are clamped to
 *               [0, n].  The kept diagrams of a group are those whose status word has no bit of skip_mask (status may be
 *               NULL); n_g of them.  G[g, h] = (scale * S_gh) / (double)(n_g * n_h), where S_gh runs over all finite rows of
 *               all kept diagrams of g against those of h: the kernel between the groups' mean embeddings.  NaN when n_g or
 *               n_h is 0.  out is (n_seg_a, n_seg_b).  With dgm_b = NULL the second set is the first (the other B arguments
 *               are ignored), out is (n_seg_a, n_seg_a), only the tiles h >= g are computed and G[h, g] is a copy of
 *               G[g, h]: symmetric as bytes.
 *   Determinism.  No atomics.  A pair alone and the same pair inside a batch, a group alone and the same group inside a
 *               batch, give the same bytes.  The order of the additions is not otherwise part of the contract; the terms
 *               are non-negative (d >= b) up to the rounding of exp.
 *   Tolerance.  Against a CPU evaluation of this text, with A = |scale| * sum |w_i w_j| (E1 + mirror * E2) (divided by
 *               n_g n_h for a Gram entry) and N_t the number of terms: DESIGN.md 3.15.
 *   Limits.     A bad ninv, scale, mirror, weight or wc, or cap < 1, is TDA_ERR_INVALID and nothing is launched.
 * The _dev forms only enqueue on `stream` and allocate nothing.  out (n_pairs) float64, status (n_pairs) int32. */
#define TDA_KW_ONE  0
#define TDA_KW_PERS 1
#define TDA_KW_ATAN 2
tda_status tda_diagram_kernel_pairs_dev(tda_ctx* ctx, const double* dgm_a, const int* cnt_a, int n_a, int cap_a,
                                        const double* dgm_b, const int* cnt_b, int n_b, int cap_b,
                                        const int* idx_a, const int* idx_b, int n_pairs,
                                        double ninv, int mirror, double scale, int weight, double wc,
                                        double* out, double* kvals, int* status, void* stream);
tda_status tda_diagram_kernel_pairs(tda_ctx* ctx, const double* dgm_a, const int* cnt_a, int n_a, int cap_a,
                                    const double* dgm_b, const int* cnt_b, int n_b, int cap_b,
                                    const int* idx_a, const int* idx_b, int n_pairs,
                                    double ninv, int mirror, double scale, int weight, double wc,
                                    double* out, double* kvals, int* status);
tda_status tda_diagram_kernel_gram_dev(tda_ctx* ctx, const double* dgm_a, const int* cnt_a, int n_a, int cap_a,
                                       const int* seg_off_a, int n_seg_a, const int* status_a,
                                       const double* dgm_b, const int* cnt_b, int n_b, int cap_b,
                                       const int* seg_off_b, int n_seg_b, const int* status_b, int skip_mask,
                                       double ninv, int mirror, double scale, int weight, double wc,
                                       double* out, void* stream);
tda_status tda_diagram_kernel_gram(tda_ctx* ctx, const double* dgm_a, const int* cnt_a, int n_a, int cap_a,
                                   const int* seg_off_a, int n_seg_a, const int* status_a,
                                   const double* dgm_b, const int* cnt_b, int n_b, int cap_b,
                                   const int* seg_off_b, int n_seg_b, const int* status_b, int skip_mask,
                                   double ninv, int mirror, double scale, int weight, double wc, double* out);

/* ---- Persistence Fisher distance between diagrams ---------------------------------------
 * The Fisher information metric distance between two persistence diagrams (Le and Yamada, NeurIPS 2018; the exact route of
 * GUDHI's PersistenceFisherDistance, without kernel_approx), on which the persistence Fisher kernel exp(-t * out) is built;
 * the kernel is formed by the Python layer, not on the device.  GUDHI is not installed anywhere this project runs, so no
 * parity with it is claimed.  The contract is this text; tests/fisher_ref.py evaluates it.
 *   Inputs.     Rows (b_i, d_i), i < min(max(cnt, 0), cap), float64.  F_A / F_B are the rows of A / B with both values
 *               finite, in their stored order; m = |F_A|, n = |F_B|, N = m + n.  The diagonal image of a row is (h, h)
 *               with h = 0.5 * (b + d), the formula of the sliced Wasserstein text.  The caller passes
 *               ninv = -1 / (2 sigma^2): the device never divides by sigma.
 *   Lists.      P = F_A followed by the images of F_B, N points.  Q = F_B followed by the images of F_A, N points.
 *               Theta = P followed by Q, 2N points with multiplicity.
 *   Values.     For x in Theta and u in a list: dx = x1 - u1; dy = x2 - u2; g = exp((dx * dx + dy * dy) * ninv).  No
 *               multiply-add anywhere.
 *                 r_P(x) = sum over u in P of g;  r_Q(x) likewise over Q
 *                 Z_P = sum over x in Theta of r_P(x);  Z_Q likewise
 *                 a_x = sqrt(r_P(x) / Z_P);  b_x = sqrt(r_Q(x) / Z_Q)
 *                 c2 = sum over x in Theta of (a_x - b_x)^2
 *                 out = 2 * asin(min(0.5 * sqrt(c2), 1))
 *               N = 0 gives out = 0.  The arguments of exp are the same float64 on the GPU and in a CPU evaluation; only
 *               exp, sqrt, asin and the order of the additions differ.
 *   Form.       out is the angle acos(sum over x of sqrt(rho_P(x) rho_Q(x))) of the paper, rho = r / Z, written through the
 *               chord between the unit vectors a and b.  The acos form loses half the digits near 0 and does not return 0
 *               for a diagram against itself; the chord form is well conditioned on all of [0, pi / 2], the range of out.
 *   Status.     N > TDA_PF_MAX_POINTS gives NaN and TDA_WIN_TOO_LARGE.  A pair index outside [0, n_a) or [0, n_b) gives
 *               NaN and TDA_WIN_NO_PAIR.  Every other pair has status 0; out is NaN wherever status is not 0.
 *   Limits.     A ninv that is not finite and < 0, or cap < 1, is TDA_ERR_INVALID and nothing is launched.
 *   Determinism.  No atomics.  The order of the additions is not part of the contract, with two exceptions that are.  A pair
 *               alone and the same pair inside a batch give the same bytes: nothing about the arithmetic depends on
 *               anything but that pair's own m and n.  And r_P and r_Q, and Z_P and Z_Q, are accumulated by the same code
 *               in the same order over their lists: two diagrams with the same finite rows in the same order give
 *               out == 0.0 exactly, wherever their non-finite rows sit.
 *   Tolerance.  Against a CPU evaluation of this text: (C + 8 N) * 2^-53 absolute, DESIGN.md 3.16.
 * The _dev form only enqueues on `stream` and allocates nothing.  out (n_pairs) float64, status (n_pairs) int32. */
#define TDA_PF_MAX_POINTS 512
tda_status tda_persistence_fisher_batch_dev(tda_ctx* ctx, const double* dgm_a, const int* cnt_a, int n_a, int cap_a,
                                            const double* dgm_b, const int* cnt_b, int n_b, int cap_b,
                                            const int* idx_a, const int* idx_b, int n_pairs, double ninv,
                                            double* out, int* status, void* stream);
tda_status tda_persistence_fisher_batch(tda_ctx* ctx, const double* dgm_a, const int* cnt_a, int n_a, int cap_a,
                                        const double* dgm_b, const int* cnt_b, int n_b, int cap_b,
                                        const int* idx_a, const int* idx_b, int n_pairs, double ninv,
                                        double* out, int* status);

/* ---- Landmark Rips: greedy permutation (furthest-point sampling) in front of the cloud Rips ----------------
 * ripser(X, n_perm=k) for clouds above TDA_MAX_POINTS points: k landmarks chosen by the greedy permutation, Rips on the
 * landmarks alone, and the covering radius r_cover.  For each of H0 and H1 the landmark diagram lies within bottleneck
 * distance 2 * r_cover of the diagram of the whole cloud.  The selection is upstream ripser.py's __get_greedy_perm, stated
 * from knowledge of upstream.  The contract is this text; tests/landmark_ref.py evaluates it.
 *   Cloud.      X, P points in dim coordinates.  Takens form: rows s[i * subsample + k * tau], k < dim, with
 *               P = ceil((n_t - (dim - 1) * tau) / subsample) (0 when the numerator is <= 0), as tda_takens_rips_batch
 *               builds it, always normalised.  Cloud form: the first n_pts[w] rows of pc[w], (n_win, p_cap, dim).  With
 *               normalise, X is first min-max normalised per column over the whole cloud: (x - min) / range, range 0
 *               replaced by 1 (utils.py:127-130).
 *   Distance.   To a pivot p, for i != p:
 *                 d(i, p) = sqrt(max(((-2 * dot(x_i, x_p)) + |x_i|^2) + |x_p|^2, 0)),   d(p, p) = 0
 *               with dot = fma(.., fma(.., x0 * y0)), |x|^2 the left-to-right sum of the products without fma, and a
 *               correctly rounded sqrt: column p of the distance matrix the cloud Rips ranks, kept in float64.
 *   Selection.  For P > n_perm:  idx[0] = 0 and ds = d(., 0).  For t = 1 .. n_perm - 1: idx[t] = the LOWEST index at which
 *               ds attains its maximum (values compared after the square root, as np.argmax does);
 *               lambda[t - 1] = ds[idx[t]];  ds = min(ds, d(., idx[t])).  Last, lambda[n_perm - 1] = max(ds) = r_cover.
 *               n_lm = n_perm.  The text is followed literally: once every point is covered at distance 0, index 0 is
 *               picked again and the landmark cloud has duplicate rows.
 *   Identity.   For P <= n_perm nothing is selected: idx = 0 .. P - 1, n_lm = P, lambda[0 .. P - 1] = 0, r_cover = 0.
 *   Outputs.    lm (n_win, n_perm, dim) float64: the landmark rows X[idx[t]] (normalised when X is), in selection order;
 *               lm_idx (n_win, n_perm) int32;  lm_lambda (n_win, n_perm) float64, may be null;  r_cover (n_win) float64;
 *               n_lm (n_win) int32;  n_full (n_win) int32 = P.  Rows and entries from n_lm on are left untouched.
 *   Refused windows.  tau < 1 in the Takens form, or P > TDA_LM_MAX_POINTS (cloud form: P > min(p_cap,
 *               TDA_LM_MAX_POINTS)): n_lm = TDA_MAX_POINTS + 1 -- a count no landmark set can have --, r_cover = NaN,
 *               n_full = P, nothing else written.  A negative n_pts counts as 0.
 *   Diagrams.   tda_takens_rips_landmarks runs the selection into the caller's landmark buffers and then
 *               tda_cloud_rips_batch on (lm, n_lm) with normalise = 0: its diagrams ARE the diagrams of the cloud path on
 *               the landmark rows, by composition; retry policy and widening ladder apply to that second stage unchanged.
 *               P < 3 ends as TDA_WIN_DEGENERATE with [[0,0]],[[0,0]], a refused window as TDA_WIN_TOO_LARGE with counts
 *               0 (the cloud stage flags the count above TDA_MAX_POINTS itself).  n_points (nullable) receives n_lm.
 *               h0_cap >= n_perm.
 *   Limits.     3 <= n_perm <= TDA_MAX_POINTS, 1 <= dim <= TDA_MAX_DIM, subsample >= 1, 1 <= n_t <= TDA_LM_MAX_SAMPLES,
 *               1 <= p_cap <= TDA_LM_MAX_POINTS; anything else is TDA_ERR_INVALID and nothing is launched.
 *   Non-finite samples give unspecified landmarks (indices stay inside the cloud, the loop has a fixed trip count).
 *   Determinism.  No atomics; a window alone and inside a batch give the same bytes.
 * The _dev forms only enqueue on `stream` and allocate nothing.  The host forms stage the output buffers in both
 * directions, so "left untouched" holds for them too. */
#define TDA_LM_MAX_POINTS 1024
#define TDA_LM_MAX_SAMPLES 4096
tda_status tda_takens_landmarks_dev(tda_ctx* ctx, const double* win, const int* tau, int n_win, int n_t, int dim,
                                    int subsample, int n_perm, double* lm, int* lm_idx, double* lm_lambda,
                                    double* r_cover, int* n_lm, int* n_full, void* stream);
tda_status tda_takens_landmarks(tda_ctx* ctx, const double* win, const int* tau, int n_win, int n_t, int dim,
                                int subsample, int n_perm, double* lm, int* lm_idx, double* lm_lambda,
                                double* r_cover, int* n_lm, int* n_full);
tda_status tda_cloud_landmarks_dev(tda_ctx* ctx, const double* pc, const int* n_pts, int n_win, int p_cap, int dim,
                                   int normalise, int n_perm, double* lm, int* lm_idx, double* lm_lambda,
                                   double* r_cover, int* n_lm, int* n_full, void* stream);
tda_status tda_cloud_landmarks(tda_ctx* ctx, const double* pc, const int* n_pts, int n_win, int p_cap, int dim,
                               int normalise, int n_perm, double* lm, int* lm_idx, double* lm_lambda,
                               double* r_cover, int* n_lm, int* n_full);
tda_status tda_takens_rips_landmarks_dev(tda_ctx* ctx, const double* win, const int* tau, int n_win, int n_t, int dim,
                                         int subsample, int n_perm, double thresh, double* lm, int* lm_idx,
                                         double* lm_lambda, double* r_cover, int* n_lm, int* n_full,
                                         double* h0, int h0_cap, int* h0_cnt, double* h1, int h1_cap, int* h1_cnt,
                                         int* n_points, int* status, void* stream);
tda_status tda_takens_rips_landmarks(tda_ctx* ctx, const double* win, const int* tau, int n_win, int n_t, int dim,
                                     int subsample, int n_perm, double thresh, double* lm, int* lm_idx,
                                     double* lm_lambda, double* r_cover, int* n_lm, int* n_full,
                                     double* h0, int h0_cap, int* h0_cnt, double* h1, int h1_cap, int* h1_cnt,
                                     int* n_points, int* status);

/* ---- Sublevel-set persistence of time series: H0 of the lower-star filtration of a 1-D signal ----------------
 * What ripser's lower_star example, a cubical complex on a 1-D array and persistence-based peak detection compute: every
 * local minimum paired with the local maximum at which its basin merges into a deeper one.  Superlevel sets: pass -x.
 * None of those libraries is installed where this project runs, so no parity with them is claimed.  The contract is this
 * text; tests/sublevel_ref.py evaluates it.
 *   Signal.     x[0 .. n_t - 1], float64, all finite.  Vertices are totally ordered by (x[i], i).  Vertex i enters the
 *               filtration at x[i], edge (i, i + 1) at the later of its ends.
 *   Rows.       The vertices are processed in that order with union-find.  When two components meet at vertex v, the one
 *               whose minimum is larger in the total order dies (elder rule): the row (birth, death) =
 *               (x[min of the dying component], x[v]) with indices (argmin, v).  Rows with birth == death are dropped.  The
 *               component of the global minimum g gives the last row, (x[g], +inf), indices (g, -1).
 *   Order.      The finite rows ascend in (death, birth, death index): ripser's H0 order.  At most
 *               TDA_SL_ROWS(n_t) = (n_t + 1) / 2 rows.  Births and deaths are input values, copied bit for bit.
 *   Equivalent form, the one the kernel evaluates (no sequential sweep; tests/test_sublevel_model.py holds the two
 *               together).  Each interior vertex p above both neighbours in the total order gives one row.  ml is the
 *               minimum, in the total order, of the maximal run of vertices left of p that are below p, mr the same to the
 *               right, y the larger of ml and mr: the row is (x[y], x[p], y, p).  Every maximum is independent of the others.
 *   Addressing. Signal s = w * n_ch + c starts at element win_start[w] + c * win_ld[w] of sig, the tables of
 *               tda_eeg_window_ragged_dev (device int64, n_win entries each).  Both NULL: the windows are stacked,
 *               (n_win, n_ch, n_t).  One of them NULL is TDA_ERR_INVALID.
 *   Outputs.    dgm (n_win * n_ch, cap, 2) float64;  cnt and status (n_win * n_ch) int32;  idx nullable,
 *               (n_win * n_ch, cap, 2) int32.  Only rows [0, cnt) of a signal's own block are written.
 *   Status.     A signal with a sample that is not finite has cnt = 0 and TDA_WIN_NOT_FINITE, and no row of it is written;
 *               the other signals of the batch are unaffected.  Every other signal has status 0.
 *   Limits.     1 <= n_t <= TDA_SL_MAX_SAMPLES, n_ch >= 1, cap >= TDA_SL_ROWS(n_t); anything else is TDA_ERR_INVALID and
 *               nothing is launched.
 *   Determinism.  No atomics; a signal alone and inside a batch give the same bytes.
 * The _dev form only enqueues on `stream` and allocates nothing.  The host form stages the output buffers in both
 * directions, so "only rows [0, cnt)" holds for it too; its tables are host arrays. */
#define TDA_SL_MAX_SAMPLES 4096
#define TDA_SL_ROWS(n) (((n) + 1) / 2)
tda_status tda_sublevel_batch_dev(tda_ctx* ctx, const double* sig, const long long* win_start, const long long* win_ld,
                                  int n_win, int n_ch, int n_t, double* dgm, int cap, int* cnt, int* idx, int* status,
                                  void* stream);
tda_status tda_sublevel_batch(tda_ctx* ctx, const double* sig, const long long* win_start, const long long* win_ld,
                              int n_win, int n_ch, int n_t, double* dgm, int cap, int* cnt, int* idx, int* status);

/* ---- Phase-locking value: phase synchrony of the channels of a window, and its distance matrix ----------------
 * The PLV of Lachaux et al. (1999): the length of the mean phasor of the phase difference of two channels over the window;
 * it ignores amplitude.  The second connectivity beside Pearson correlation (tda_corr_dist_batch); Rips on the result is
 * tda_rips_dm_batch[_dev].  The contract is this text; tests/plv_ref.py evaluates it.
 *   Window.     x[c][t], float64, c < n_ch, t < n_t.
 *   Analytic signal.  h[c][t] = sum_m x[c][m] * g[(t - m) mod n_t], g = imag(ifft(h_hilbert)) of length n_t, tabulated by
 *               the host as scipy.signal.hilbert builds its multiplier (preprocess._hilbert_g); z = x + i h is
 *               scipy.signal.hilbert(x, axis=-1) of the WINDOW ITSELF.  Phases taken from a Hilbert transform of the whole
 *               recording are out of scope: transform the recording first and this call has nothing to offer.
 *   Unit phasor.  m = sqrt(x*x + h*h), u = (x / m, h / m); where the computed m is 0, u = (1, 0) (np.angle(0) is 0).
 *   PLV.        plv[i][j] = sqrt(R*R + I*I) / n_t, R + iI = sum_t u_i[t] * conj(u_j[t]), for i != j; plv[i][i] = 1.0
 *               exactly.  Pair (i, j), i < j, is computed once and stored at both places: symmetric as bytes.
 *   Distance.   dist = correlation_to_distance(plv, method), the four methods of tda_corr_to_dist_batch (clip, formula,
 *               clamp at 0); method 0, sqrt(2 (1 - p)), keeps the meaning of the Rips threshold of the EEG step.  The
 *               diagonal is exactly 0, the matrix symmetric as bytes.
 *   Sums.       float64 fused multiply-adds in an order that is the kernel's, not the contract's: agreement with the
 *               definition is to rounding (tests/plv_ref.py: PLV_BAR), not bit for bit.
 *   Status.     A window with a sample that is not finite gets TDA_WIN_NOT_FINITE and its plv and dist blocks are NaN; the
 *               other windows are unaffected.  Every other window has status 0.
 *   Addressing. As tda_sublevel_batch_dev: row c of window w starts at element win_start[w] + c * win_ld[w] of sig (device
 *               int64 tables, n_win entries each).  Both NULL: stacked windows (n_win, n_ch, n_t).  One NULL is
 *               TDA_ERR_INVALID.
 *   Outputs.    dist (n_win, n_ch, n_ch) float64; plv the same, nullable (nothing of it is touched then); status (n_win).
 *   Limits.     2 <= n_ch <= TDA_PLV_MAX_CHANNELS, 2 <= n_t <= TDA_PLV_MAX_SAMPLES (the window, the table and a tile of at
 *               least 16 samples' phasors share the 160 KiB of LDS of a CU), method in 0..3; anything else is
 *               TDA_ERR_INVALID and nothing is launched.
 *   Determinism.  No atomics; a window alone and inside a batch give the same bytes.
 * The _dev form only enqueues on `stream` and allocates nothing (g: device, n_t doubles).  The host form stages every
 * buffer; its tables and g are host arrays. */
#define TDA_PLV_MAX_CHANNELS 64
#define TDA_PLV_MAX_SAMPLES 256
tda_status tda_plv_dist_batch_dev(tda_ctx* ctx, const double* sig, const long long* win_start, const long long* win_ld,
                                  int n_win, int n_ch, int n_t, const double* g, int method, double* dist, double* plv,
                                  int* status, void* stream);
tda_status tda_plv_dist_batch(tda_ctx* ctx, const double* sig, const long long* win_start, const long long* win_ld,
                              int n_win, int n_ch, int n_t, const double* g, int method, double* dist, double* plv,
                              int* status);

/* ---- Analytic-signal connectivity: wPLI, imaginary coherency, coherence, envelope correlation, and their distances ----
 * Correlation and the PLV are inflated by volume conduction: one source seen at zero lag by many electrodes gives values
 * near 1.  The measures that answer it, and the amplitude counterpart: the weighted phase-lag index (Vinck et al. 2011), the
 * imaginary part of coherency (Nolte et al. 2004), coherence (the full magnitude beside it) and the correlation of the
 * amplitude envelopes (AEC).  Rips on the result is tda_rips_dm_batch[_dev].  The contract is this text;
 * tests/connectivity_ref.py evaluates it.
 *   Window.     x[c][t], float64, c < n_ch, t < n_t.
 *   Analytic signal.  That of the phase-locking value: h[c][t] = sum_m x[c][m] * g[(t - m) mod n_t], g the host table
 *               (preprocess._hilbert_g), z = x + i h: scipy.signal.hilbert of the WINDOW ITSELF.
 *   Sums.       For i < j:  s[t] = h_i[t] x_j[t] - x_i[t] h_j[t] = Im(z_i conj z_j) (in the kernel two rounded products and
 *               their difference, so identical channels have s = 0 exactly);  r[t] = x_i x_j + h_i h_j;
 *               S = sum s, A = sum |s|, R = sum r;  P_c = sum (x_c^2 + h_c^2);  a_c[t] = sqrt(x_c^2 + h_c^2).
 *   Measures.   TAU = TDA_CONN_TAU = 2^-40.  For i != j:
 *               TDA_CONN_WPLI  (0, "wpli")   abs(S) / A, and exactly 0.0 where A <= TAU * sqrt(P_i P_j): the pair is in phase
 *                              or antiphase to rounding, no lag information exists
 *               TDA_CONN_IMCOH (1, "imcoh")  abs(S) / sqrt(P_i P_j), 0.0 where P_i P_j == 0
 *               TDA_CONN_COH   (2, "coh")    sqrt(S*S + R*R) / sqrt(P_i P_j), 0.0 where P_i P_j == 0
 *               TDA_CONN_AEC   (3, "aec")    the Pearson correlation of a_i and a_j in centred form (mean first, then products
 *                              of deviations), and 0.0 where either envelope is flat: sum (a_c - mean_c)^2 <=
 *                              n_t * (TAU * mean_c)^2 (the reference's NaN -> 0 rule for zero-variance channels)
 *               The threshold rules are part of the definition, not a tolerance: they make the duplicated, rescaled, zero
 *               and constant channels deterministic instead of a quotient of rounding noise.  value[i][i] = 1.0 exactly.
 *               Pair (i, j), i < j, is computed once and stored at both places: symmetric as bytes.
 *   Distance.   dist = correlation_to_distance(value, method), the four methods of tda_corr_to_dist_batch (clip, formula,
 *               clamp at 0).  The diagonal is exactly 0, the matrix symmetric as bytes.
 *   Order.      float64 in an order that is the kernel's, not the contract's (aec: one pass, the deviations taken from the
 *               mean of the first block of samples, which leaves a covariance what it is): agreement with the definition is
 *               to rounding (tests/connectivity_ref.py: BAR), not bit for bit.
 *   Status.     A window with a sample that is not finite gets TDA_WIN_NOT_FINITE and its value and dist blocks are NaN; the
 *               other windows are unaffected.  Every other window has status 0.
 *   Addressing. As tda_plv_dist_batch_dev: win_start / win_ld (device int64 tables) or both NULL for stacked windows; one
 *               NULL is TDA_ERR_INVALID.
 *   Outputs.    dist (n_win, n_ch, n_ch) float64; value the same, nullable (nothing of it is touched then); status (n_win).
 *   Limits.     Those of the PLV: 2 <= n_ch <= TDA_PLV_MAX_CHANNELS, 2 <= n_t <= TDA_PLV_MAX_SAMPLES; measure in 0..3, method
 *               in 0..3; anything else is TDA_ERR_INVALID and nothing is launched.
 *   Determinism.  No atomics, no scratch; a window alone, inside a batch and through a window table gives the same bytes.
 * The _dev form only enqueues on `stream` and allocates nothing (g: device, n_t doubles).  The host form stages every
 * buffer; its tables and g are host arrays. */
#define TDA_CONN_TAU 0x1p-40
#define TDA_CONN_WPLI 0
#define TDA_CONN_IMCOH 1
#define TDA_CONN_COH 2
#define TDA_CONN_AEC 3
tda_status tda_connectivity_dist_batch_dev(tda_ctx* ctx, const double* sig, const long long* win_start,
                                           const long long* win_ld, int n_win, int n_ch, int n_t, const double* g,
                                           int measure, int method, double* dist, double* value, int* status, void* stream);
tda_status tda_connectivity_dist_batch(tda_ctx* ctx, const double* sig, const long long* win_start, const long long* win_ld,
                                       int n_win, int n_ch, int n_t, const double* g, int measure, int method, double* dist,
                                       double* value, int* status);

/* ---- Two-sample permutation sums: within- and between-group sums of a matrix under many relabellings ----------------
 * The arithmetic of the permutation test of Robinson and Turner (2017, "Hypothesis testing for topological data analysis")
 * on a distance matrix between diagrams, and of its kernel twin, the MMD / energy two-sample test on a Gram matrix: the
 * sums of the matrix over the pairs inside group 0, inside group 1 and between the groups, for every relabelling of a
 * batch at once.  The statistics and p-values made of them are the host's (utils.two_sample_statistic).  The reference
 * compares groups with a random forest on scalars and has no counterpart.  The contract is this text;
 * tests/permutation_ref.py evaluates it literally.
 *   Matrices.   D (n_mat, n, ld) float64, ld >= n: entry (i, j) of matrix m is D[(m * n + i) * ld + j].  Only entries with
 *               i < j are read; the diagonal, the lower triangle and the columns from n on are never touched.
 *   Labels.     lab (TDA_PT_WORDS(n_perm), n) uint64: bit (p % 64) of lab[p / 64][j] is the label, 0 or 1, of item j under
 *               relabelling p (engine.pack_labels).  The bits of the last word past n_perm are ignored.
 *   Row sums.   For relabelling p and row i:  same = +0.0, diff = +0.0;  for j = i + 1, ..., n - 1 in this order:
 *               same = same + D[i][j] if label[j] == label[i], else diff = diff + D[i][j].  An entry is added to one of the
 *               two and not at all to the other.
 *   Blocks.     Rows are taken in blocks of TDA_PT_ROW_BLOCK: block b = rows [b R, min((b + 1) R, n)), TDA_PT_BLOCKS(n)
 *               of them.  Per block p00 = p11 = p01 = +0.0;  for i ascending in the block:
 *               (label[i] == 0 ? p00 : p11) += same_i;  p01 += diff_i.
 *   Sums.       S00 = S11 = S01 = +0.0;  for b ascending:  S00 += p00_b;  S11 += p11_b;  S01 += p01_b.
 *               So S00 (S11) is the sum of D[i][j], i < j, over the pairs with both labels 0 (1), S01 over the pairs with
 *               different labels, each in one written order that is a function of n alone: it does not depend on n_perm, on
 *               the place of a relabelling in the batch, on n_mat or on how the work is launched.  The order treats the two
 *               classes alike: S00 under a labelling has the bytes of S11 under its complement, and S01 the same bytes
 *               under both.  No partial sum is ever -0.0 (they start at +0.0), so adding an empty row or block changes
 *               nothing.
 *   Non-finite entries follow IEEE: an Inf or NaN at (i, j), i < j, reaches exactly the one sum whose class holds the pair.
 *   Outputs.    out (n_mat, 3, n_perm) float64: S00, S11, S01.  n1 (n_perm) int32, nullable: the number of items labelled 1.
 *   Work.       work: device, at least TDA_PT_WORK_DOUBLES(n_mat, n, n_perm) doubles, the block partials; the call reads
 *               nothing it has not written there.
 *   Limits.     2 <= n <= TDA_PT_MAX_ITEMS, 1 <= n_perm <= TDA_PT_MAX_PERM, 0 <= n_mat <= TDA_PT_MAX_MATRICES, ld >= n;
 *               anything else is TDA_ERR_INVALID with a message in tda_last_error, and nothing is launched or written.
 *   Determinism.  No atomics; one lane per relabelling; results are the bytes of the definition.
 * The _dev form only enqueues on `stream` (two launches) and allocates nothing.  The host form stages every buffer and
 * takes its work space from the context. */
#define TDA_PT_ROW_BLOCK 64
#define TDA_PT_MAX_ITEMS 4096
#define TDA_PT_MAX_PERM 1048576
#define TDA_PT_MAX_MATRICES 4096
#define TDA_PT_WORDS(n_perm) (((n_perm) + 63) / 64)
#define TDA_PT_BLOCKS(n) (((n) + TDA_PT_ROW_BLOCK - 1) / TDA_PT_ROW_BLOCK)
#define TDA_PT_WORK_DOUBLES(n_mat, n, n_perm) \
    ((long long)(n_mat) * TDA_PT_BLOCKS(n) * 3 * 64 * TDA_PT_WORDS(n_perm))
tda_status tda_perm_sums_batch_dev(tda_ctx* ctx, const double* D, int n_mat, int n, int ld, const unsigned long long* lab,
                                   int n_perm, double* work, long long work_doubles, double* out, int* n1, void* stream);
tda_status tda_perm_sums_batch(tda_ctx* ctx, const double* D, int n_mat, int n, int ld, const unsigned long long* lab,
                               int n_perm, double* out, int* n1);

/* ---- Wasserstein distances between GROUPED diagrams, paired by position -------------
 * replaces compute_cross_wasserstein (scripts/matched_vs_mismatched.py:86-95) for every (recording, band) at once:
 * the diagrams of A group g are paired, position by position, with those of B group partner_seg[g] (mvm:89:
 * n = min(len(eeg), len(audio)); matched: the recording's own audio, mvm:136-137; mismatched: the audio of the first
 * file of the other condition, mvm:113-118,139-141).
 * A side: dgm_a (n_a, cap_a, 2), cnt_a (n_a), seg_off_a (n_seg_a + 1) int32, grp_a (n_a) int32 = the group of every
 * diagram.  B side: dgm_b (n_b, cap_b, 2), cnt_b, seg_off_b (n_seg_b + 1), status_b (n_b) = the status words of the
 * Rips call that made the B diagrams.  partner_seg: (n_seg_a) int32, the B group of each A group or -1.
 * A diagram w at position i of group g, p = partner_seg[g], has a pair iff p >= 0, i < seg_off_b[p+1] - seg_off_b[p]
 * and status_b[seg_off_b[p] + i] does not carry TDA_WIN_DEGENERATE (mvm:60: a cloud with < 3 points gives no diagram).
 * With a pair, out[w] / status[w] are what tda_wasserstein_batch_dev gives for it (the same solver); without one,
 * out[w] = NaN and status[w] = TDA_WIN_NO_PAIR, and the workgroup leaves before the solver.  Table entries that point
 * outside the tables count as "no pair".  out: (n_a) float64, status: (n_a) int32.  Device pointers only,
 * enqueue-only, no allocation.                                                             */
tda_status tda_wasserstein_cross_dev(tda_ctx* ctx, const double* dgm_a, const int* cnt_a, int cap_a, int n_a,
                                     const int* grp_a, const int* seg_off_a, int n_seg_a,
                                     const double* dgm_b, const int* cnt_b, int cap_b, int n_b,
                                     const int* seg_off_b, int n_seg_b, const int* status_b,
                                     const int* partner_seg, double* out, int* status, void* stream);

/* ---- one row of the control experiment per (recording, band) group ---------------------
 * out: (n_seg, 4) float64 = [ nanmean of the matched distances (mvm:137), nanmean of the mismatched ones (mvm:141),
 * number of matched pairs, number of mismatched pairs ] from the out / status arrays of two
 * tda_wasserstein_cross_dev calls over the same A side.  The pairs of a group are its first n entries (mvm:89); the
 * mean is np.nanmean over exactly those n values (mvm:95), numpy's pairwise tree; a pair whose solver status is set
 * counts as NaN; no pair (mvm:90) or only NaN: NaN.
 * status_a / seg_flags (nullable): the status words of the Rips call that made the A diagrams, and an (n_seg) int32
 * output that receives, per group, the OR of status_a and of the two solver status arrays without TDA_WIN_NO_PAIR and
 * TDA_WIN_DEGENERATE -- as tda_recording_rows_dev: any bit means a row the reference would not give.        */
tda_status tda_cross_rows_dev(tda_ctx* ctx, const double* w_matched, const int* status_matched,
                              const double* w_mismatched, const int* status_mismatched, const int* seg_off_a,
                              int n_seg, double* out, const int* status_a, int* seg_flags, void* stream);

/* ---- the match-mismatch matrix: every A group against every candidate column ------------
 * compute_cross_wasserstein (mvm:86-95) of the EEG diagrams of every (recording, band) group against the audio diagrams
 * of EVERY candidate recording, not only the own audio and one mismatched partner (mvm:134-145): the matched distance,
 * the reference's mismatched column, a null distribution per recording and the rank of the true audio all come from
 * this one matrix.
 * A side: dgm_a (n_a, cap_a, 2), cnt_a (n_a), seg_off_a (n_seg_a + 1) int32, cls_a (n_seg_a) int32 = the class (band) of
 * every group, 0 .. n_cls - 1; a group with another value has no entry anywhere (NaN, 0 pairs).  B side: dgm_b
 * (n_b, cap_b, 2), cnt_b, status_b (n_b) and seg_off_b with n_cls * n_col + 1 entries: the B groups class-major, the
 * group of (class k, column c) is k * n_col + c; an empty group is a column without audio.
 * Entry (g, c) is what tda_wasserstein_cross_dev with partner_seg[g] = cls_a[g] * n_col + c followed by
 * tda_cross_rows_dev gives for group g, bit for bit: out[g, c] the mean over the pairs (numpy's pairwise tree, a pair
 * with a solver status counts as NaN; no pair: NaN), pairs[g, c] their number, flags[g, c] the OR of their solver
 * status words without TDA_WIN_NO_PAIR and TDA_WIN_DEGENERATE.  The pairing rules are tda_wasserstein_cross_dev's;
 * table entries that point outside the tables count as "no pair".  A group of more than 64 diagrams gets NaN, 0 pairs
 * and TDA_WIN_TOO_LARGE in every column.
 * out float64, pairs int32, flags int32, each (n_seg_a, n_col) row-major; every word is written by the call (nothing
 * has to be cleared before it).  No per-pair array exists, on the host or the device.  Honours tda_set_launch_scheme
 * as the other Wasserstein entry points.  Device pointers only, enqueue-only, no allocation (TDA_SCHEME_LISTS outside
 * a capture may grow the per-stream lists to 65,536 entries once).                                        */
tda_status tda_wasserstein_matrix_dev(tda_ctx* ctx, const double* dgm_a, const int* cnt_a, int cap_a, int n_a,
                                      const int* seg_off_a, int n_seg_a, const int* cls_a,
                                      const double* dgm_b, const int* cnt_b, int cap_b, int n_b,
                                      const int* seg_off_b, int n_cls, int n_col, const int* status_b,
                                      double* out, int* pairs, int* flags, void* stream);

/* ---- one row of the match-mismatch matrix per (recording, band) group ---------------------
 * rows: (n_seg_a, 6) float64 = [ w_own, n_own_pairs, n_valid, n_less, n_equal, null_mean ] from out / pairs / flags of
 * tda_wasserstein_matrix_dev and own_col (n_seg_a) int32, the column of the group's own audio (mvm:136-137) or -1.
 * w_own = out[g, own_col[g]] and n_own_pairs its pair count.  The others are the columns c != own_col[g] with a finite
 * entry: n_valid their number, n_less / n_equal how many of them are < / == w_own (the midrank of the true audio among
 * n_valid + 1 candidates is 1 + n_less + n_equal / 2), null_mean their mean (NaN without any; a sum of non-negative
 * terms in the kernel's own order: within (n_valid + 1) * 2^-52 relative of numpy's).  Without an own column, or with
 * a NaN there: w_own = NaN, n_less = n_equal = 0, n_valid and null_mean over all finite columns.
 * status_a (nullable, with seg_off_a) / seg_flags (nullable): as tda_cross_rows_dev -- per group the OR of the row's
 * flags and of the group's status_a words without TDA_WIN_NO_PAIR and TDA_WIN_DEGENERATE.                   */
tda_status tda_match_rows_dev(tda_ctx* ctx, const double* out, const int* pairs, const int* flags,
                              int n_seg_a, int n_col, const int* own_col, const int* status_a, const int* seg_off_a,
                              double* rows, int* seg_flags, void* stream);

/* ---- Sliced Wasserstein distance from prepared diagrams: sort once, merge per pair ----
 * The definition is the sliced Wasserstein text above, unchanged.  For a pair (A, B) and a direction, the sorted
 * projections of A' are the merge of two lists that depend on one diagram each: the sorted projections of A's rows and
 * the sorted projections of B's diagonal images.  tda_sliced_prepare_dev makes both lists of every diagram and direction
 * once; the other two entry points merge them per pair.  A merge of two sorted lists is the sorted list of their union,
 * so every u_i, v_i and t_i is the float64 of tda_sliced_wasserstein_batch_dev, and the additions are made in that
 * kernel's order (rank e = 64 r + lane belongs to `lane`; a lane adds its ranks r = 0, 1, .. in turn, only those with
 * e < N; the lanes are combined by the butterfly lane ^ 1, 2, .., 32; one wave adds the L_k as k = lane, lane + 64, the
 * same butterfly, then divides by n_dirs): a prepared pair returns the BYTES tda_sliced_wasserstein_batch_dev returns
 * for the same pair and directions.
 *
 * tda_sliced_prepare_dev.  dgm (n_dgm, cap, 2), cnt (n_dgm), dirs (n_dirs, 2) as above.  Per diagram: cnt is clamped to
 * [0, cap], rows with a non-finite entry are dropped, an empty diagram becomes {(0, 0)}; m rows remain.  For every
 * direction k two ascending lists of m float64 are written: kind 0, the projections (c * b) + (s * d) of the rows; kind 1,
 * the projections (c * h) + (s * h) of the images, h = 0.5 * (b + d) -- the formula of the text above, no multiply-add and
 * not (c + s) * h.
 * Table.  slot_off is (n_dgm + 1) int64, made by the caller, non-decreasing: diagram i owns the slot
 * [slot_off[i], slot_off[i + 1]) of s_i rows.  Its region of `table` starts at double 2 * n_dirs * slot_off[i]; element
 * ((2 k + kind) * s_i + rank) of the region is the value of direction k, kind and rank.  Only the ranks < m are defined;
 * the rest of a region is not written.  `table` holds 2 * n_dirs * table_rows doubles.  All index arithmetic is size_t.
 * m_clean (n_dgm) int32: m for a diagram that was prepared; -1 where m > TDA_SW_MAX_POINTS, m > s_i, slot_off[i + 1] >
 * table_rows or the slot is not a slot (negative start or length): such a diagram writes nothing to the table.
 * Limits: 1 <= n_dirs <= TDA_MAX_DIRECTIONS and cap >= 1; anything else is TDA_ERR_INVALID and nothing is launched.
 *
 * tda_sliced_prepared_pairs_dev.  Two prepared sets (table, slot_off, m_clean, number of diagrams), made with the SAME
 * direction table of n_dirs rows; idx_a / idx_b (n_pairs) int32, NULL = identity.  out (n_pairs) float64, NaN where
 * status != 0; status (n_pairs) int32.  A pair with m_clean < 0 on either side or N = m + n > TDA_SW_MAX_POINTS gets NaN
 * and TDA_WIN_TOO_LARGE.  An index outside [0, n_a) / [0, n_b): tda_sliced_wasserstein_batch_dev does not look at its
 * indices (it is not told n_a and n_b; only the host form rejects them), so such an index is the caller's error there and
 * here.  This entry point knows the sizes and does not read outside the tables for it: the pair gets NaN and
 * TDA_WIN_NO_PAIR.  1 <= n_dirs <= TDA_MAX_DIRECTIONS, or TDA_ERR_INVALID.
 *
 * tda_sliced_matrix_dev.  tda_wasserstein_matrix_dev with the sliced distance in the place of the Wasserstein distance:
 * the same tables (seg_off_a / cls_a over the A diagrams, the B groups class-major in seg_off_b, status_b), the same
 * pairing rules (by position within a group; no pair where the B group is shorter, the B diagram carries
 * TDA_WIN_DEGENERATE, the class is out of range or a table entry points outside its table) and the same entry: out[g, c]
 * the mean over the pairs (numpy's pairwise tree; the pairs of an entry are its first `pairs` positions, a pair with a
 * status counts as NaN; no pair: NaN), pairs[g, c] their number, flags[g, c] the OR of their status words without
 * TDA_WIN_NO_PAIR and TDA_WIN_DEGENERATE.  The value of a pair is tda_sliced_prepared_pairs_dev's, bit for bit.  A group of
 * more than 64 diagrams gets NaN, 0 pairs and TDA_WIN_TOO_LARGE in every column.  out float64, pairs int32, flags int32,
 * each (n_seg_a, n_col) row-major; every word is written by exactly one workgroup of the call, nothing has to be cleared
 * before it, no atomics, no per-pair array.
 * All three: device pointers only, enqueue-only on `stream`, no allocation. */
tda_status tda_sliced_prepare_dev(tda_ctx* ctx, const double* dgm, const int* cnt, int cap, int n_dgm,
                                  const double* dirs, int n_dirs, const long long* slot_off,
                                  double* table, long long table_rows, int* m_clean, void* stream);
tda_status tda_sliced_prepared_pairs_dev(tda_ctx* ctx, const double* table_a, const long long* slot_off_a, const int* m_a,
                                         int n_a, const double* table_b, const long long* slot_off_b, const int* m_b,
                                         int n_b, const int* idx_a, const int* idx_b, int n_pairs, int n_dirs,
                                         double* out, int* status, void* stream);
tda_status tda_sliced_matrix_dev(tda_ctx* ctx, const double* table_a, const long long* slot_off_a, const int* m_a, int n_a,
                                 const int* seg_off_a, int n_seg_a, const int* cls_a,
                                 const double* table_b, const long long* slot_off_b, const int* m_b, int n_b,
                                 const int* seg_off_b, int n_cls, int n_col, const int* status_b, int n_dirs,
                                 double* out, int* pairs, int* flags, void* stream);

/* ---- timing helper ------------------------------------------------------------
 * HIP-event timing on the stream the kernels are launched on (bench.py roofline). */
tda_status tda_event_create(tda_ctx* ctx, void** ev);
tda_status tda_event_record(tda_ctx* ctx, void* ev, void* stream);
tda_status tda_event_elapsed_ms(tda_ctx* ctx, void* ev_start, void* ev_stop, float* ms); /* syncs on stop */
tda_status tda_event_destroy(tda_ctx* ctx, void* ev);
tda_status tda_stream_sync(tda_ctx* ctx, void* stream);
/* Arms a one-shot probe (one slot per `which`; TDA_PROBE_NONE clears all): the NEXT launch of the first-pass kernel of `which` made through this
 * context records ev_start right before and ev_stop right after that ONE kernel on its stream
 * (the retry passes and the row-ordering kernel of the same call are outside the bracket).  This is
 * the per-kernel duration bench.py's roofline uses; rocprofv3 --kernel-trace reports the same kernel.
 * dev_span (optional, TDA_PROBE_RIPS_CLOUD only): device u64[4] preset to 0.  Workgroup 0 (dispatched
 * first) stores the 100 MHz wall-clock time of its start in [0]; finished workgroups are counted in [1];
 * the last one adds (its end - that start) -- the interval a kernel trace shows, i.e. without the time
 * the grid waits for CU slots behind other in-flight batches -- to [2], counts the launch in [3] and
 * resets [1].  A launch captured into a HIP graph with the probe armed therefore measures every replay;
 * average duration = [2] / [3] / 100 MHz.  The events may be NULL when dev_span is given. */
#define TDA_PROBE_NONE       0
#define TDA_PROBE_RIPS_CLOUD 1   /* rips_cloud_kernel, first pass (tda_takens_rips_batch / tda_cloud_rips_batch) */
#define TDA_PROBE_RIPS_DM    2   /* rips_dm_kernel, first pass (tda_rips_dm_batch) */
#define TDA_PROBE_CORR_DIST  3   /* corr_dist_kernel (tda_corr_dist_batch / _sliding) */
tda_status tda_set_kernel_probe(tda_ctx* ctx, int which, void* ev_start, void* ev_stop, void* dev_span);

#ifdef __cplusplus
}
#endif
#endif /* TDAEEG_H */
